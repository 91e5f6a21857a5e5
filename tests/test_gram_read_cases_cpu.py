"""CPU proofs for tests/gram_read_cases.py and for the rule of csrc/bh_gram_read_plan.h:

  - the instances are exact (gram_cases.Ledger), dense, with pairwise different rows and a vector that is not periodic;
  - the mirror of gram_symv_kernel's row-group assignment and of its chunk / diagonal rule covers every pair (i, j <= i) exactly
    once and touches nothing above the diagonal, on grids of 8, 64, 256 and 304 compute units; the bytes per workgroup differ by one
    row group at the most; the mirror is held against the source (serpentine formula, load predicate, served widths);
  - every fault kind changes a result on every width at which the faulty element exists;
  - the decision header over all its inputs against a hand-written table, in Python through a stand-alone host program built with
    -fsanitize=address,undefined (as bh_free_image_plan.h is)."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gram_cases as gc
import gram_read_cases as grc
import rs_cases as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")
WIDTHS = grc.SERVED_WIDTHS + (grc.UNSERVED_WIDTH,)


def _src(name):
    return open(os.path.join(CSRC, name)).read()


# ------------------------------------------------------------------------------------------------------------------ instances
@pytest.mark.parametrize("n", WIDTHS)
def test_instances_are_exact_dense_and_tell_rows_apart(n):
    inst = grc.instance(n)
    led = gc.Ledger()
    grc.prove(inst, led)
    assert max(led.bits.values()) <= 53
    assert inst.J.shape == (grc.ROWS, n) and set(np.unique(inst.J)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert inst.C.shape == (1, n) and set(np.unique(inst.C)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert np.all(inst.G != 0.0) and np.array_equal(inst.G, inst.G.T)                    # dense, symmetric, every G_ii != 0
    assert np.unique(inst.G, axis=0).shape[0] == n                                       # no two rows agree
    a = np.abs(inst.v)
    assert np.all((a >= 1) & (a <= 7) & (a == np.rint(a)))
    for period in (2, 64, 256, 512):
        if n > period + 8:
            assert not np.array_equal(inst.v[period:], inst.v[:-period]), period
    assert inst.q == float(inst.v @ inst.y)


def test_the_worst_case_width_stays_below_2_53():
    """n = 16384, the widest Gram handle: the bounds of the issue (about 2^27 for a row, 2^44 for the quadratic form) from the entry
    bounds alone."""
    gmax, vmax, n = grc.ROWS * 4 + 2, 7, 16384
    assert (n * gmax * vmax).bit_length() <= 27 and (2 * n * n * gmax * vmax * vmax).bit_length() <= 53


def test_lower_bytes_formula():
    hdr = _src("bh_gram_read_plan.h")
    assert "16.0 * ((n & 1) ? (m + 1.0) * (m + 1.0) : m * (m + 1.0))" in hdr
    for n in WIDTHS + (5, 6, 7):
        m = n // 2
        assert grc.lower_bytes(n) == 16 * ((m + 1) * (m + 1) if n & 1 else m * (m + 1))


# --------------------------------------------------------------------------------------------------------------------- mirror
def test_the_mirror_is_the_source():
    plan, kern, api = _src("bh_gram_read_plan.h"), _src("bh_gramsym.hip.h"), _src("bh_api.hip")
    assert "return (p & 1) ? (p + 1) * G - 1 - b : p * G + b;" in plan                  # grc.group
    calls = re.findall(r"(?:load_group|process)\([AB], vi[AB], ([^)]*)\);", kern)         # every group handed on is ngroups - 1 - index
    assert sorted(calls) == ["ngroups - 1 - g"] * 3 + ["ngroups - 1 - gn"] * 2
    assert "const int diag = rv ? (int)(row >> 1) : -1;" in kern and "if (tid + k * T <= diag) {" in kern      # chunks 0 .. i / 2
    assert kern.count("__builtin_nontemporal_load") == 1                                 # ... and no other load of G
    assert "X[r][k].y = 0.0;" in kern and "if (!odd) X[r][k].x = 0.0;" in kern           # the diagonal's chunk
    assert "a.nrows = H->n;" in api                                                      # n rows, not ld
    m = re.search(r"constexpr bool kGramSymLastGeomOk = (true|false);", api)
    assert m and (m.group(1) == "true") == grc.served(grc.UNSERVED_WIDTH)
    assert "return nchunks <= max_chunks / 2 || last_geom_spill_free;" in plan
    assert all(grc.served(n) for n in grc.SERVED_WIDTHS)
    # the geometries the widths land in: every one of the served ones, the threshold and one past it
    assert [rs.path_of(n) for n in grc.SERVED_WIDTHS] == [0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert rs.path_of(grc.UNSERVED_WIDTH) == 6


@pytest.mark.parametrize("n_cu", grc.N_CU_DESIGN)
@pytest.mark.parametrize("n", WIDTHS)
def test_every_pair_once_nothing_above_and_balanced(n, n_cu):
    for bpc in (0, 2):
        geo = grc.geometry(n, n_cu, bpc)
        seen = np.zeros(n, dtype=np.int64)
        per_wg = []
        for b in range(geo["grid"]):
            groups = grc.groups_of(b, geo)
            assert groups == sorted(set(groups), reverse=True) and len(groups) >= 1      # strictly decreasing; nobody idles
            # the loop of the kernel stops at the first group out of range: none behind it may be in range again
            assert grc.group(b, len(groups), geo["grid"]) >= geo["ngroups"] and grc.group(b, len(groups) + 1, geo["grid"]) >= geo["ngroups"]
            rows = grc.rows_of(b, n, geo)
            np.add.at(seen, rows, 1)
            per_wg.append(grc.workgroup_bytes(b, n, geo))
        assert np.all(seen == 1)                                                         # every row in exactly one workgroup
        assert sum(per_wg) == grc.lower_bytes(n)
        one_group = max(grc.group_bytes(g, n, geo) for g in range(max(geo["ngroups"] - 2, 0), geo["ngroups"]))   # the heaviest: the last full one
        assert max(per_wg) - min(per_wg) <= one_group
    # per row: the columns of the loaded chunks, less column i + 1 of an even row, are exactly 0 .. i
    for i in list(range(min(n, 40))) + list(range(max(n - 40, 0), n)):
        cols = [2 * c + e for c in range(grc.chunks_loaded(i)) for e in (0, 1)]
        assert max(cols) <= i + 1 and max(cols) < rs.ld_of(n)                            # inside the row of the image
        used = [j for j in cols if not (i % 2 == 0 and j == i + 1)]
        assert used == list(range(i + 1))


@pytest.mark.parametrize("n", WIDTHS)
def test_model_is_the_int64_answer_and_every_fault_shows(n):
    inst = grc.instance(n)
    for n_cu, bpc in ((304, 0), (8, 2)):
        y, q = grc.model(inst, n_cu, bpc)
        assert np.array_equal(y.view(np.uint64), inst.y.view(np.uint64)) and q == inst.q, (n, n_cu, bpc)
    exists = {"diagonal dropped": True, "diagonal twice": True, "above-diagonal element let in": n >= 2, "v_i / v_j mix-up": n >= 2,
              "chunk skipped": n >= 3}
    for fault in grc.FAULTS:
        y, q = grc.model(inst, 64, 0, fault)
        if not exists[fault]:
            assert np.array_equal(y, inst.y) and q == inst.q
            continue
        assert not np.array_equal(y, inst.y), (n, fault)
        if fault != "v_i / v_j mix-up":                                                  # (the quadratic form has no transposed part)
            assert q != inst.q, (n, fault)


# ------------------------------------------------------------------------------------------------------------- decision header
FULL, LOWER, QUAD_FROM_G, SWEEP_J = 0, 1, 2, 3
PRODUCT, QUAD, WHOLE_ROWS = 0, 1, 2
# (mode, gram_form, served) -> path of a product, of a quadratic form, of a whole-row kernel.  Written out by hand.
TABLE = {
    (0, 0, 0): (FULL, SWEEP_J, FULL), (0, 0, 1): (FULL, SWEEP_J, FULL), (0, 1, 0): (FULL, SWEEP_J, FULL), (0, 1, 1): (FULL, SWEEP_J, FULL),
    (1, 0, 0): (FULL, SWEEP_J, FULL), (1, 0, 1): (FULL, SWEEP_J, FULL), (1, 1, 0): (FULL, SWEEP_J, FULL), (1, 1, 1): (LOWER, SWEEP_J, FULL),
    (2, 0, 0): (FULL, SWEEP_J, FULL), (2, 0, 1): (FULL, SWEEP_J, FULL), (2, 1, 0): (FULL, SWEEP_J, FULL), (2, 1, 1): (LOWER, QUAD_FROM_G, FULL),
}

PROGRAM = r"""
#include <cstdio>
#include "bh_gram_read_plan.h"
using namespace bh;
int main() {
    static_assert(GRAM_READ_FULL == 0 && GRAM_READ_LOWER == 1 && GRAM_READ_LOWER_QUAD == 2, "the values of the public header");
    for (int mode = 0; mode <= 2; ++mode)
        for (int form = 0; form <= 1; ++form)
            for (int served = 0; served <= 1; ++served)
                for (int call = 0; call <= 2; ++call) {
                    GramReadIn in{};
                    in.mode = mode; in.gram_form = form != 0; in.served = served != 0; in.call = call;
                    std::printf("P %d %d %d %d %d\n", mode, form, served, call, (int)gram_read_path(in));
                }
    for (long long m = -2; m <= 4; ++m) std::printf("M %lld %d\n", m, gram_read_mode_ok(m) ? 1 : 0);
    const long long chunks[] = {0, 1, 8, 64, 65, 2048, 4096, 4097, 4104, 8192, 8193, 8200};
    for (long long c : chunks) std::printf("S %lld %d %d\n", c, gram_read_served(c, 8192, false) ? 1 : 0, gram_read_served(c, 8192, true) ? 1 : 0);
    const long long widths[] = {1, 2, 3, 15, 16, 17, 4097, 8192, 16384};
    for (long long n : widths) std::printf("B %lld %.17g\n", n, gram_read_lower_bytes(n));
    const long long grids[] = {1, 2, 3, 8, 304};
    for (long long G : grids)
        for (long long b = 0; b < G; b += (G > 8 ? 101 : 1))
            for (long long p = 0; p < 5; ++p) std::printf("G %lld %lld %lld %lld\n", G, b, p, (long long)gram_read_group(b, p, G));
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan_log(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("gram_read_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return [line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]


def test_decision_header_against_the_table(plan_log):
    got = {tuple(int(x) for x in v[1:5]): int(v[5]) for v in plan_log if v[0] == "P"}
    assert len(got) == 3 * 2 * 2 * 3
    for (mode, form, srv), paths in TABLE.items():
        for call in (PRODUCT, QUAD, WHOLE_ROWS):
            assert got[(mode, form, srv, call)] == paths[call], (mode, form, srv, call)
    assert {int(v[1]): int(v[2]) for v in plan_log if v[0] == "M"} == {-2: 0, -1: 0, 0: 1, 1: 1, 2: 1, 3: 0, 4: 0}


def test_decision_header_served_bytes_and_groups(plan_log):
    srv = {int(v[1]): (int(v[2]), int(v[3])) for v in plan_log if v[0] == "S"}
    assert srv == {0: (0, 0), 1: (1, 1), 8: (1, 1), 64: (1, 1), 65: (1, 1), 2048: (1, 1), 4096: (1, 1), 4097: (0, 1), 4104: (0, 1),
                   8192: (0, 1), 8193: (0, 0), 8200: (0, 0)}
    for n in grc.SERVED_WIDTHS + (grc.UNSERVED_WIDTH,):
        assert srv_of(n) == grc.served(n)
    for v in plan_log:
        if v[0] == "B":
            assert float(v[2]) == grc.lower_bytes(int(v[1]))
        if v[0] == "G":
            G, b, p, g = (int(x) for x in v[1:])
            assert g == grc.group(b, p, G)
    # b, 2G-1-b, 2G+b, ... written out for a grid of 3
    assert [[grc.group(b, p, 3) for p in range(4)] for b in range(3)] == [[0, 5, 6, 11], [1, 4, 7, 10], [2, 3, 8, 9]]


def srv_of(n):
    """gram_read_served with the build's verdict on the widest geometry (false), in Python."""
    nc = rs.nchunks_of(n)
    return 1 <= nc <= rs.K_MAX_CHUNKS // 2


def test_the_launchers_ask_the_header():
    api = _src("bh_api.hip")
    assert api.count("gram_read_path(in)") == 1 and "gram_read_served(H->nchunks, kMaxChunks, kGramSymLastGeomOk)" in api
    # one product launcher, one quadratic-form launcher; the whole-row kernels are not touched by the mode
    assert api.count("gram_path(H, GRAM_CALL_PRODUCT)") == 3 and api.count("gram_path(H, GRAM_CALL_QUAD)") == 1
    assert api.count("launch_quad(H, ") == 3                                             # bh_vthv, the line search, the swept model reduction
    for name in ("bh_gramcg.hip.h", "bh_cauchygram.hip.h", "bh_cauchygrameq.hip.h"):
        assert "gram_read" not in _src(name)
    assert len(list(itertools.product(range(3), range(2), range(2)))) == len(TABLE)
