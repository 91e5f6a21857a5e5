"""The rule that picks the form of the Cauchy search (csrc/bh_cauchy_plan.h: cauchy_select, no HIP in it) against the rule as the
option descriptions of include/benlsip_hip.h and README.md state it: a stand-alone program built by the host compiler prints form,
fused and the effective refresh interval over a cross product of handle, constraint set, communicator and options; every line is
compared with `expected` below, which is written from the documents, not from the C++."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")

GRAM_HANDLE = (0, 1)
MA = (0, 1, 16, 17, 64, 65)
COMM = (0, 1)
LDA_IS_LD = (0, 1)
MULTI_PANEL = (0, 1)
HISTORY = (0, 1, 2)                      # last_cauchy_passes = -1, 4 (1 + mA), 4 (1 + mA) + 1
BOOL = (0, 1)                            # cauchy_image, cauchy_fused, cauchy_gram, cauchy_gram_eq
MAX_MA = (0, 16, 64)
REFRESH = (0, 5, 2 ** 20 + 1)

PROGRAM = r"""
#include "bh_cauchy_plan.h"
#include <cstdio>
int main() {
    const int mAs[] = {0, 1, 16, 17, 64, 65};
    const long long max_mas[] = {0, 16, 64}, refreshes[] = {0, 5, (1ll << 20) + 1};
    for (int gram = 0; gram < 2; ++gram) for (int mA : mAs) for (int comm = 0; comm < 2; ++comm) for (int lda = 0; lda < 2; ++lda)
    for (int panel = 0; panel < 2; ++panel) for (int hist = 0; hist < 3; ++hist)
    for (int image = 0; image < 2; ++image) for (int fused = 0; fused < 2; ++fused) for (int og = 0; og < 2; ++og) for (int oge = 0; oge < 2; ++oge)
    for (long long max_ma : max_mas) for (long long refresh : refreshes) {
        bh::CauchySelectIn in{};
        in.gram_handle = gram != 0; in.mA = mA; in.comm = comm != 0; in.lda_is_ld = lda != 0; in.multi_panel = panel != 0;
        in.last_cauchy_passes = hist == 0 ? -1 : 4 * (1 + mA) + (hist - 1);
        in.cauchy_image = image; in.cauchy_image_max_ma = max_ma; in.cauchy_fused = fused; in.cauchy_gram = og; in.cauchy_gram_eq = oge;
        in.cauchy_image_refresh = refresh;
        const bh::CauchySelection s = bh::cauchy_select(in);
        std::printf("%d %d %d\n", (int)s.form, s.fused ? 1 : 0, s.refresh);
    }
    return 0;
}
"""


def expected(gram, mA, comm, lda, panel, hist, image, fused, opt_gram, opt_gram_eq, max_ma, refresh):
    """(form, fused, refresh) by the documents.
    "cauchy_gram": Gram-form handle, no linear equalities, one rank -> form 3; any other handle or constraint set takes the path it
    takes with 0.  "cauchy_gram_eq": Gram-form handle, 1..64 equalities, one rank, lineq image with the handle's leading dimension ->
    form 4, independent of "cauchy_gram", "cauchy_image" and "cauchy_image_max_ma".  "cauchy_image": the row space of J with box
    constraints (several ranks keep it: each its rows, the two sums all-reduced); "cauchy_image_max_ma": also with up to that many
    equalities, and above it up to 64 when the previous search on the bh_proj took more than 4 (1 + mA) passes.  "cauchy_fused": that
    search, box constraints, one rank, one kernel per breakpoint.  "cauchy_image_refresh": the row-space search on one rank (several
    ranks: ignored), n <= 16384 where one kernel per breakpoint runs (a wider J keeps its carried images); the interval lives in the
    20-bit pass counter."""
    last = -1 if hist == 0 else 4 * (1 + mA) + (hist - 1)
    one_rank = not comm
    form = 0
    if image:
        if mA == 0:
            form = 1
        elif mA <= max_ma or (mA <= 64 and last > 4 * (1 + mA)):
            form = 2
    if gram and one_rank:                               # the two options on a Gram-form handle come before the others
        if opt_gram and mA == 0:
            form = 3
        if opt_gram_eq and 1 <= mA <= 64 and lda:
            form = 4
    one_kernel = form == 1 and one_rank and fused == 1
    interval = 0
    if form in (1, 2) and one_rank and not (one_kernel and panel):
        interval = min(refresh, 2 ** 20 - 1)
    return form, int(one_kernel), interval


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("cauchy_plan")
    src, exe = d / "select.cpp", d / "select"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


def test_selection_rule_matches_the_documented_rule(program):
    out = subprocess.run([program], check=True, capture_output=True, text=True).stdout.splitlines()
    cases = list(itertools.product(GRAM_HANDLE, MA, COMM, LDA_IS_LD, MULTI_PANEL, HISTORY, BOOL, BOOL, BOOL, BOOL, MAX_MA, REFRESH))
    assert len(out) == len(cases) == 41472
    forms = set()
    for case, line in zip(cases, out):
        got = tuple(int(x) for x in line.split())
        assert got == expected(*case), (case, got, expected(*case))
        forms.add(got[0])
    assert forms == {0, 1, 2, 3, 4}


def test_library_takes_the_form_from_the_rule():
    """bh_api.hip includes the header, fills the plan from cauchy_select and reports the plan's form."""
    api = open(os.path.join(CSRC, "bh_api.hip")).read()
    assert '#include "bh_cauchy_plan.h"' in api and "cauchy_select(in)" in api
    assert "P->last_cauchy_form = (int)p.form;" in api
    hdr = open(os.path.join(CSRC, "bh_cauchy_plan.h")).read()
    assert "hip" not in "".join(ln for ln in hdr.splitlines() if ln.lstrip().startswith("#include"))
