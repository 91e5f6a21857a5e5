"""The runs of tests/free_image_eq_cases.py are what they claim to be: which states the cap nfree > mA leaves out, the actions the Book
mirror takes, integer Gram matrices that are exact in any summation order, their condition, an oracle that alone ends every "wide" cell
solved (by a margin) and every "box" cell on the boundary after at least two products, the compact image Af expected from the mirror's
map against csrc/bh_free_image_plan.h itself (built into a stand-alone program by the host compiler, with the address and
undefined-behaviour sanitizers), and the exact iteration's operands."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import benlsip_ref as R
import free_image_cases as F
import free_image_eq_cases as E
import proj_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")
N_CU = 256

# stdin: per run "Q n steps"; per call "mA", mA lines of n integers (the calling handle's A), one line of n characters 0 / 1 (1: fixed).
# stdout: per call "C ldf nfree | Af[0..mA*ldf)" with Af formed through the header's own map by the rule of free_image_build_kernel.
PROGRAM = r"""
#include "bh_free_image_plan.h"
#include <cstdio>
#include <string>
#include <iostream>
using namespace bh;
int main() {
    std::string tag;
    long long n, steps;
    while (std::cin >> tag >> n >> steps) {
        FreeImageBook b;
        const long long nwords = (n + 63) / 64;
        uint64_t af_epoch = 0, fi_epoch = 0;
        for (long long c = 0; c < steps; ++c) {
            long long mA;
            std::cin >> mA;
            std::vector<long long> A((size_t)(mA * n));
            for (auto& a : A) std::cin >> a;
            std::string bits;
            std::cin >> bits;
            if ((long long)bits.size() != n) { std::printf("X length\n"); return 1; }
            std::vector<uint64_t> want((size_t)nwords, 0ull);
            for (long long i = 0; i < n; ++i) if (bits[(size_t)i] == '1') want[(size_t)(i >> 6)] |= 1ull << (i & 63);
            const long long nfix = free_image_count(want.data(), n);
            int64_t k_new = 0, k_freed = 0;
            if (b.present) free_image_diff(b, want.data(), &k_new, &k_freed);
            const FreeImageAction act = free_image_decide(2, b.present, 4099, n, nfix, k_new, k_freed, b.credit, 10);
            std::vector<int32_t> ops;
            if (act == FI_BUILD) free_image_book_build(b, want.data(), n);
            else if (act == FI_MOVE) free_image_book_move(b, want.data(), ops);
            // every call of these runs pushes a mask under a fresh epoch: the stamp rule must ask for a rebuild, and accept its result
            const uint64_t mask_epoch = (uint64_t)(c + 1);
            fi_epoch = mask_epoch;
            if (free_image_af_valid(af_epoch, fi_epoch, mask_epoch)) { std::printf("X stamp\n"); return 1; }
            af_epoch = fi_epoch;
            if (!free_image_af_valid(af_epoch, fi_epoch, mask_epoch)) { std::printf("X stamp after\n"); return 1; }
            std::printf("C %lld %lld |", (long long)b.ldf, (long long)b.nfree);
            for (long long r = 0; r < mA; ++r)
                for (long long s = 0; s < b.ldf; ++s) {
                    const int m = b.map[(size_t)s];
                    if (m >= n) { std::printf("X map\n"); return 1; }
                    std::printf(" %lld", m >= 0 ? A[(size_t)(r * n + m)] : 0ll);
                }
            std::printf("\n");
        }
    }
    return 0;
}
"""


def test_the_cap_drops_only_the_two_smallest_widths_of_s1():
    dropped = {run: E.dropped_by_the_cap(run) for run in E.RUNS}
    assert dropped["S1_m2_m1"] == [("S1", 2), ("S1", 1)] and dropped["S1_m64"] == [("S1", w) for w in (17, 16, 15, 2, 1)]
    assert all(dropped[run] == [] for run in ("S3_m17", "S2_m64", "S4_m5", "S5_m1"))
    # S1 with mA = 64 is the table's width list, which lies inside the cap; every other run visits every state the cap leaves
    assert [F.states("S1")[k].width for k in E.kept_states("S1_m64")] == [140, 139, 128, 127, 113]
    assert [F.states("S1")[k].width for k in E.kept_states("S1_m2_m1")] == [140, 139, 128, 127, 113, 112, 17, 16, 15]
    for run in ("S3_m17", "S2_m64", "S4_m5", "S5_m1"):
        assert E.kept_states(run) == list(range(len(F.states(E.RUNS[run][0]))))
    for run in E.RUNS:
        for c in E.calls(run):
            assert c.width > c.mA and c.width == c.fix.shape[0] - int(c.fix.sum()) and c.fix.shape[0] <= 2101
            assert np.array_equal(np.sort(c.map[:c.width]), np.flatnonzero(~c.fix)) and np.all(c.map[c.width:] == -1)


def test_what_each_run_exercises():
    s1 = E.calls("S1_m2_m1")
    assert [c.mA for c in s1] == [2] * 9 + [1] * 9 and [c.width for c in s1[:9]] == [c.width for c in s1[9:]]
    # the second pass starts with freed variables: a rebuild, then the moves of the first pass again, the same maps
    assert [c.action for c in s1] == (["build"] + ["move"] * 8) * 2 and s1[9].builds == 2
    assert all(np.array_equal(a.map, b.map) for a, b in zip(s1[:9], s1[9:]))
    # mA = 64: all 16 rows of every row group of proj_apply_linv_kernel, and two of its workgroups (more than 64 chunks) at widths >= 129
    assert [c.nch for c in E.calls("S1_m64")] == [72, 72, 64, 64, 64]
    # S3: n == ld, and 17 = 16 * 1 + 1
    assert F.SEQS["S3"][0] % 16 == 0 and E.RUNS["S3_m17"][1] == (17,)
    # S2: 33 partial blocks of A_free r at the build, a 323-column move
    s2 = E.calls("S2_m64")
    assert (s2[0].nch + 15) // 16 == 33 and any(c.moved == 323 for c in s2)
    # S4: three constraint handles, pairwise different A; the same active set pushed twice by one of them
    s4 = E.calls("S4_m5")
    assert [c.who for c in s4] == ["A/5", "B/5", "A/5", "B/5", "B/5", "Bp/5"] and [c.action for c in s4] == ["build", "move", "build", "move", "use", "build"]
    mats = [E.lineq("S4_m5", w) for w in ("A/5", "B/5", "Bp/5")]
    assert all(not np.array_equal(a, b) for i, a in enumerate(mats) for b in mats[i + 1:])
    # ... so that a stale Af is another matrix, not a permutation of the right one
    assert not np.array_equal(E.expected_af("S4_m5", s4[1]), E.expected_af("S4_m5", s4[1]._replace(who="A/5")))
    assert [c.action for c in E.calls("S5_m1")] == ["build", "build", "move"]


@pytest.mark.parametrize("run", list(E.RUNS))
def test_gram_matrices_are_exact_integers_in_any_order(run):
    """A_free A_free' in 64-bit integers against float64 sums taken column by column, forwards and backwards, in index order (the masked
    full columns) and in slot order (the compact image); and cond <= COND_MAX."""
    for c in E.calls(run):
        A = E.lineq(run, c.who)
        assert A.dtype == np.float64 and np.array_equal(A, np.rint(A)) and np.abs(A).max() <= 3 and 9 * A.shape[1] < 2 ** 53
        Ai = A.astype(np.int64)                                                         # (exact: 64-bit integers cannot overflow at 9 n)
        M_int = Ai[:, ~c.fix] @ Ai[:, ~c.fix].T
        for cols in (np.flatnonzero(~c.fix), c.map[:c.width]):
            for order in (cols, cols[::-1]):
                terms = A[:, None, order] * A[None, :, order]
                M = np.cumsum(terms, axis=2)[:, :, -1]                                  # sequential float64 sums
                assert np.array_equal(M.astype(np.int64), M_int) and np.array_equal(M, M_int.astype(np.float64)), (run, c.width)
        # the zero padding of the compact image adds nothing
        Af = E.expected_af(run, c)
        assert Af.shape == (c.mA, c.ldf) and not Af[:, c.width:].any() and np.array_equal(Af @ Af.T, M_int.astype(np.float64))
        cond = float(np.linalg.cond(M_int.astype(np.float64)))
        assert cond <= E.COND_MAX, (run, c.width, cond)


@pytest.mark.parametrize("run", list(E.RUNS))
def test_the_oracle_alone_satisfies_the_rule_of_the_cells(run):
    """Every call, both bounds settings: the wide run ends solved and never comes within MARGIN of its tolerance; the box run ends on the
    boundary after at least two products (no exception).  First and last call: the oracle decides its own iteration count under every
    re-association of its own H*p."""
    n_calls = len(E.calls(run))
    for i in range(n_calls):
        anchor = i in (0, n_calls - 1)
        wide, box = E.cell(run, N_CU, i, "wide", band=anchor), E.cell(run, N_CU, i, "box", band=anchor)
        assert wide["status"] == int(R.CGStatus.solved) and wide["n_hmul"] == wide["iters"] - 1 and wide["n_hmul"] <= 64
        assert all(x == 0.0 or max(x, 1.0 / x) >= F.MARGIN for x in wide["rtv_over_tol"]), (run, i, wide["rtv_over_tol"])
        assert box["status"] == int(R.CGStatus.bound_hit) and box["n_hmul"] == box["iters"] and box["n_hmul"] >= 2, (run, i, box["n_hmul"])
        assert np.all(np.abs(wide["w"]) < 0.1 * F.WIDE) and box["delta"] < F.XB
        if anchor:
            for c in (wide, box):
                assert set(c["band"].values()) == {(c["status"], c["iters"])}, (run, i, c["band"])
    assert E.seed_is_good(run, N_CU, None)


@pytest.fixture(scope="module")
def header_log(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("free_image_eq_cases")
    src, exe = d / "af.cpp", d / "af"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    text = []
    for run in E.RUNS:
        cs = E.calls(run)
        text.append("Q %d %d" % (cs[0].fix.shape[0], len(cs)))
        for c in cs:
            A = E.lineq(run, c.who)
            text.append(str(c.mA))
            text += [" ".join(str(int(x)) for x in row) for row in A]
            text.append("".join("1" if b else "0" for b in c.fix))
    out = subprocess.run([str(exe)], input="\n".join(text) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert not any(line.startswith("X") for line in out), [line for line in out if line.startswith("X")]
    return out


def test_the_expected_af_is_the_header_map_applied_to_a(header_log):
    lines = iter(header_log)
    for run in E.RUNS:
        for c in E.calls(run):
            head, body = next(lines).split("|")
            assert [int(x) for x in head.split()[1:]] == [c.ldf, c.width], (run, c.width, head)
            assert np.array_equal(np.array(body.split(), dtype=np.float64).reshape(c.mA, c.ldf), E.expected_af(run, c)), (run, c.who, c.width)
    assert next(lines, None) is None


def test_the_exact_iteration_is_exact():
    """A_free = T Q on every one of the three nested free sets (a constraint handle each), J'J = 16 I on any set of columns: the whole
    chain is exact in float64 in any order (sum_bits of proj_cases), w = -P(g) / 16 is dyadic and A w = 0 exactly."""
    cases = E.exact_cases()
    assert [c.n - c.nfix for c in cases] == list(E.EXACT_WIDTHS) and E.EXACT_WIDTHS[1] % 16 == 0 and E.EXACT_WIDTHS[2] == E.EXACT_MA + 1
    assert E.EXACT_N % 16 == 0
    assert all(np.all(b.fix[a.fix]) for a, b in zip(cases, cases[1:]))            # nested: every step only fixes variables
    J = pc.cg_jacobian(E.EXACT_N).astype(np.int64)
    for c in cases:
        cols = np.flatnonzero(~c.fix)
        assert np.array_equal(J[:, cols].T @ J[:, cols], 16 * np.eye(cols.shape[0], dtype=np.int64))
        assert c.sum_bits < 52.0 and c.mA == E.EXACT_MA
        w = 0.0 - c.v / pc.CG_C
        assert np.any(w != 0.0) and not w[c.fix].any() and not (c.A @ w).any()
        Af = c.A[:, ~c.fix]
        assert np.array_equal(Af @ Af.T, c.tri.dense() @ np.diag(c.D.astype(np.float64)) @ c.tri.dense().T)
