"""The rule behind the per-handle switch bh_hess_set_cauchy_rows (csrc/bh_cauchy_rows_plan.h: cauchy_rows_apply, applied by
cauchy_make_plan after cauchy_select): a stand-alone program built by the host compiler runs the cross product of handle form, mA,
communicator, width, the Cauchy options and the switch.  Form 6 appears exactly where include/benlsip_hip.h says — implicit handle, no
linear equalities, one rank, a served width, the switch on — whatever the options are; every other line is cauchy_select's own."""
import itertools
import os
import shutil
import subprocess

import pytest

import test_cauchy_plan_cpu as base

WIDTHS = (1, 33, 4081, 4096, 4097, 8200, 16400)
PROGRAM = r"""
#include "bh_cauchy_rows_plan.h"
#include <cstdio>
int main() {
    const int mAs[] = {0, 1, 17};
    const long long widths[] = {%s};
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
        const bh::CauchySelection b = bh::cauchy_rows_apply(r, a);
        std::printf("%%d %%d %%d %%d %%d %%d %%d %%d %%d\n", (int)a.form, a.fused ? 1 : 0, a.refresh, a.block, (int)b.form, b.fused ? 1 : 0, b.refresh, b.block,
                    bh::cauchy_rows_served(n, r.ld) ? 1 : 0);
    }
    return 0;
}
""" % ", ".join(str(w) for w in WIDTHS)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("rowsort_plan")
    src, exe = d / "rows.cpp", d / "rows"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", base.CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    return [tuple(int(x) for x in ln.split()) for ln in out]


def _cases():
    B = (0, 1)
    return list(itertools.product(B, B, (0, 1, 17), B, WIDTHS, B, B, (0, 16), (0, 5), B))


def test_form_6_exactly_where_the_header_says(lines):
    cases = _cases()
    assert len(lines) == len(cases)
    n6, forms_off = 0, set()
    for (rows, gram, mA, comm, n, image, fused, block, refresh, sorted_), got in zip(cases, lines):
        before, after, served = got[:4], got[4:8], got[8]
        assert served == (1 if -(-n // 16) * 16 <= 4096 else 0), (n, served)
        if rows and not gram and mA == 0 and not comm and served:
            assert after == (6, 0, 0, 0), (rows, gram, mA, comm, n, after)          # whatever cauchy_image, cauchy_fused, cauchy_block, ... are
            n6 += 1
        else:
            assert after == before, (rows, gram, mA, comm, n, before, after)
        if not rows:
            forms_off.add(after[0])
    assert n6 == 4 * 2 * 2 * 2 * 2 * 2                               # four served widths x the option and gram_sorted settings
    assert 6 not in forms_off and {0, 1, 2, 3, 5} <= forms_off       # the switch off: every line is today's


def test_the_rule_is_applied_behind_cauchy_select_and_the_pinned_lines_stand():
    api = open(os.path.join(base.CSRC, "bh_api.hip")).read()
    plan = open(os.path.join(base.CSRC, "bh_cauchy_plan.h")).read()
    assert "const CauchySelection sel = cauchy_rows_apply(rin, cauchy_select(in));" in api
    assert "rin.rows_sorted = allow_sorted && H->cauchy_rows == BH_CAUCHY_ROWS_SORTED;" in api
    assert "in.gram_sorted = allow_sorted && H->cauchy_search == BH_CAUCHY_SORTED;" in api
    assert "P->last_cauchy_form = (int)p.form;" in api
    assert "CAUCHY_ROWS_SORTED = 6" in plan
    body = plan.split("struct CauchySelectIn {")[1].split("};")[0]
    fields = [ln.split(";")[0].strip() for ln in body.splitlines() if ";" in ln]
    assert fields[-1] == "bool gram_sorted"
