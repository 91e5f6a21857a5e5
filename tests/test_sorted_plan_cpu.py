"""The rule that picks the form of the Cauchy search (csrc/bh_cauchy_plan.h: cauchy_select) with the per-handle switch
bh_hess_set_cauchy_search: a stand-alone program built by the host compiler runs the cross product of tests/test_cauchy_plan_cpu.py
once with gram_sorted = false and once with true.  With the switch off every line is today's rule; with it on form 5 appears exactly
where include/benlsip_hip.h says — Gram-form handle, no linear equalities, one rank — ahead of "cauchy_gram" and whatever the Cauchy
options are, and every other line is the line of the switch off."""
import itertools
import os
import shutil
import subprocess

import pytest

import test_cauchy_plan_cpu as base

PROGRAM = r"""
#include "bh_cauchy_plan.h"
#include <cstdio>
int main() {
    const int mAs[] = {0, 1, 16, 17, 64, 65};
    const long long max_mas[] = {0, 16, 64}, refreshes[] = {0, 5, (1ll << 20) + 1};
    for (int sorted = 0; sorted < 2; ++sorted)
    for (int gram = 0; gram < 2; ++gram) for (int mA : mAs) for (int comm = 0; comm < 2; ++comm) for (int lda = 0; lda < 2; ++lda)
    for (int panel = 0; panel < 2; ++panel) for (int hist = 0; hist < 3; ++hist)
    for (int image = 0; image < 2; ++image) for (int fused = 0; fused < 2; ++fused) for (int og = 0; og < 2; ++og) for (int oge = 0; oge < 2; ++oge)
    for (long long max_ma : max_mas) for (long long refresh : refreshes) {
        bh::CauchySelectIn in{};
        in.gram_handle = gram != 0; in.mA = mA; in.comm = comm != 0; in.lda_is_ld = lda != 0; in.multi_panel = panel != 0;
        in.last_cauchy_passes = hist == 0 ? -1 : 4 * (1 + mA) + (hist - 1);
        in.cauchy_image = image; in.cauchy_image_max_ma = max_ma; in.cauchy_fused = fused; in.cauchy_gram = og; in.cauchy_gram_eq = oge;
        in.cauchy_image_refresh = refresh;
        in.gram_sorted = sorted != 0;
        const bh::CauchySelection s = bh::cauchy_select(in);
        std::printf("%d %d %d %d\n", (int)s.form, s.fused ? 1 : 0, s.refresh, s.block);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("sorted_plan")
    src, exe = d / "select.cpp", d / "select"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", base.CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    return [tuple(int(x) for x in ln.split()) for ln in out]


def _cases():
    return list(itertools.product(base.GRAM_HANDLE, base.MA, base.COMM, base.LDA_IS_LD, base.MULTI_PANEL, base.HISTORY, base.BOOL, base.BOOL,
                                  base.BOOL, base.BOOL, base.MAX_MA, base.REFRESH))


def test_switch_off_is_todays_rule(lines):
    cases = _cases()
    assert len(lines) == 2 * len(cases) == 2 * 41472
    for case, got in zip(cases, lines[:len(cases)]):
        assert got[:3] == base.expected(*case) and got[3] == 0, (case, got)
    assert {g[0] for g in lines[:len(cases)]} == {0, 1, 2, 3, 4}


def test_switch_on_gives_form_5_exactly_where_the_header_says(lines):
    cases = _cases()
    off, on = lines[:len(cases)], lines[len(cases):]
    n5 = 0
    for case, a, b in zip(cases, off, on):
        gram, mA, comm = case[:3]
        if gram and mA == 0 and not comm:                           # whatever cauchy_gram, cauchy_image, cauchy_fused, ... are
            assert b == (5, 0, 0, 0), (case, b)
            n5 += 1
        else:                                                       # implicit handle, equalities, several ranks: the line of the switch off
            assert b == a, (case, a, b)
    assert n5 == len(cases) // (2 * len(base.MA) * 2)


def test_field_is_the_last_of_the_struct_and_the_library_fills_it():
    hdr = open(os.path.join(base.CSRC, "bh_cauchy_plan.h")).read()
    body = hdr.split("struct CauchySelectIn {")[1].split("};")[0]
    fields = [ln.split(";")[0].strip() for ln in body.splitlines() if ";" in ln]
    assert fields[-1] == "bool gram_sorted" and "CAUCHY_GRAM_SORTED = 5" in hdr
    api = open(os.path.join(base.CSRC, "bh_api.hip")).read()
    assert "in.gram_sorted = allow_sorted && H->cauchy_search == BH_CAUCHY_SORTED;" in api
    assert "P->last_cauchy_form = (int)p.form;" in api
