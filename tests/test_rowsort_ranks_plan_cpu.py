"""The rule behind the per-handle switch bh_hess_set_cauchy_rows_ranks (csrc/bh_cauchy_rows_plan.h: the trailing field `ranks` of
CauchyRowsIn): a stand-alone program built by the host compiler runs the cross product of tests/test_rowsort_plan_cpu.py times
ranks in {0, 1}.  With a communicator form 6 appears exactly when the ranks switch is on, the handle is implicit, there are no linear
equalities, the width is served and the rows switch holds; with ranks = 0 every line is the one the program of
test_rowsort_plan_cpu.py prints (which never sets the field)."""
import os
import shutil
import subprocess

import pytest

import test_rowsort_plan_cpu as rows_plan

base = rows_plan.base
PROGRAM = r"""
#include "bh_cauchy_rows_plan.h"
#include <cstdio>
int main() {
    const int mAs[] = {0, 1, 17};
    const long long widths[] = {%s};
    for (int ranks = 0; ranks < 2; ++ranks)
    for (int rows = 0; rows < 2; ++rows) for (int gram = 0; gram < 2; ++gram) for (int mA : mAs) for (int comm = 0; comm < 2; ++comm)
    for (long long n : widths) for (int image = 0; image < 2; ++image) for (int fused = 0; fused < 2; ++fused) for (int block = 0; block < 17; block += 16)
    for (int refresh = 0; refresh < 6; refresh += 5) for (int sorted = 0; sorted < 2; ++sorted) {
        bh::CauchySelectIn in{};
        in.gram_handle = gram != 0; in.mA = mA; in.comm = comm != 0; in.lda_is_ld = true; in.multi_panel = n > 16384;
        in.last_cauchy_passes = -1; in.cauchy_image = image; in.cauchy_image_max_ma = 64; in.cauchy_fused = fused; in.cauchy_gram = 1;
        in.cauchy_gram_eq = 0; in.cauchy_image_refresh = refresh; in.n = n; in.cauchy_block = block; in.gram_sorted = sorted != 0;
        const bh::CauchySelection a = bh::cauchy_select(in);
        bh::CauchyRowsIn r{};
        r.rows_sorted = rows != 0; r.gram_handle = in.gram_handle; r.mA = mA; r.comm = in.comm; r.n = n; r.ld = (n + 15) / 16 * 16;
        r.ranks = ranks != 0;
        const bh::CauchySelection b = bh::cauchy_rows_apply(r, a);
        std::printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d\n", (int)a.form, a.fused ? 1 : 0, a.refresh, a.block, (int)b.form, b.fused ? 1 : 0, b.refresh, b.block,
                    bh::cauchy_rows_served(n, r.ld) ? 1 : 0);
    }
    return 0;
}
""" % ", ".join(str(w) for w in rows_plan.WIDTHS)


def _run(tmp, name, program):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp / (name + ".cpp"), tmp / name
    src.write_text(program)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", base.CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    return [tuple(int(x) for x in ln.split()) for ln in out]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("rowsort_ranks_plan")
    return _run(d, "ranks", PROGRAM), _run(d, "rows", rows_plan.PROGRAM)


def test_form_6_with_a_communicator_exactly_when_the_ranks_switch_is_on(lines):
    got, _ = lines
    cases = rows_plan._cases()
    assert len(got) == 2 * len(cases)
    n6_comm = 0
    for ranks in (0, 1):
        for (rows, gram, mA, comm, n, image, fused, block, refresh, sorted_), ln in zip(cases, got[ranks * len(cases):(ranks + 1) * len(cases)]):
            before, after, served = ln[:4], ln[4:8], ln[8]
            assert served == (1 if -(-n // 16) * 16 <= 4096 else 0), (n, served)
            if rows and not gram and mA == 0 and served and (not comm or ranks):
                assert after == (6, 0, 0, 0), (ranks, rows, gram, mA, comm, n, after)  # whatever the Cauchy options are
                n6_comm += 1 if comm else 0
            else:
                assert after == before, (ranks, rows, gram, mA, comm, n, before, after)
            if comm and not ranks:
                assert after[0] != 6
    assert n6_comm == 4 * 2 * 2 * 2 * 2 * 2                          # four served widths x the option and gram_sorted settings


def test_ranks_off_is_the_existing_rule_line_by_line(lines):
    got, existing = lines
    assert len(existing) == len(rows_plan._cases()) and got[:len(existing)] == existing
    no_comm = [i for i, c in enumerate(rows_plan._cases()) if not c[3]]
    assert all(got[len(existing) + i] == existing[i] for i in no_comm)  # no communicator: the switch changes nothing


def test_the_plan_assigns_the_field_and_the_pinned_lines_stand():
    api = open(os.path.join(base.CSRC, "bh_api.hip")).read()
    plan = open(os.path.join(base.CSRC, "bh_cauchy_rows_plan.h")).read()
    assert [ln.strip().split("//")[0].strip() for ln in api.splitlines() if ln.strip().startswith("rin.ranks")] == ["rin.ranks = H->cauchy_rows_ranks != 0;"]
    assert "const CauchySelection sel = cauchy_rows_apply(rin, cauchy_select(in));" in api
    assert "rin.rows_sorted = allow_sorted && H->cauchy_rows == BH_CAUCHY_ROWS_SORTED;" in api
    assert "(!in.comm || in.ranks)" in plan
    body = plan.split("struct CauchyRowsIn {")[1].split("};")[0]
    fields = [ln.split(";")[0].strip() for ln in body.splitlines() if ";" in ln]
    assert fields[-1] == "bool ranks"
