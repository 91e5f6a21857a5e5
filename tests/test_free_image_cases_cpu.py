"""The sequences of tests/free_image_cases.py are what they claim to be: the geometry table, the thresholds crossed, the Python mirror of
the move rule against csrc/bh_free_image_plan.h itself (built into a stand-alone program by the host compiler, with the address and
undefined-behaviour sanitizers, as tests/test_free_image_cpu.py does), an oracle that decides its own iteration count in every cell,
and integer operands that stay exact."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import benlsip_ref as R
import free_image_cases as F
from rs_cases import PICK_THRESHOLDS, RS_CONFIGS, ld_of, pick_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")
N_CU = 256                                     # the MI355X; the sequences themselves do not depend on it, only the row count does

# stdin: per sequence "Q n steps", then one line of n characters 0 / 1 (1: fixed) per call.
# stdout: per call "C action k nfree ldf builds moves | map[0..ldf)" and, for a move, "D dst_of_tail[0..k)"
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
        for (long long c = 0; c < steps; ++c) {
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
            std::printf("C %d %lld %lld %lld %lld %lld |", (int)act, (long long)ops.size(), (long long)b.nfree, (long long)b.ldf, (long long)b.builds,
                        (long long)b.moves);
            for (long long s = 0; s < b.ldf; ++s) std::printf(" %d", (int)b.map[(size_t)s]);
            std::printf("\n");
            if (act == FI_MOVE) {
                std::printf("D");
                for (int32_t d : ops) std::printf(" %d", (int)d);
                std::printf("\n");
                for (int32_t d : ops) if (d >= b.nfree) { std::printf("X dst\n"); return 1; }
            }
            if (free_image_state(b, want.data()) != FI_STATE_VALID) { std::printf("X state\n"); return 1; }
        }
    }
    return 0;
}
"""
ACTIONS = {1: "use", 2: "build", 3: "move"}


def test_every_state_has_the_geometry_of_the_table():
    for name, table in F.TABLE.items():
        got = [(s.width, s.ldf, s.nch, s.geometry, s.R, s.action, s.k) for s in F.states(name)]
        assert got == table, (name, got)
        for s in F.states(name):
            assert s.width == s.fix.shape[0] - int(s.fix.sum()) and s.ldf % 16 == 0 and s.ldf >= s.width
            assert s.nch == ld_of(s.width) // 2 and s.geometry == pick_config(s.nch) and s.R == RS_CONFIGS[s.geometry][2]
            assert np.array_equal(np.sort(s.map[:s.width]), np.flatnonzero(~s.fix)) and np.all(s.map[s.width:] == -1)
        assert F.rows_for(name, N_CU) == (1 if name == "S2" else 2) * N_CU * max(RS_CONFIGS[s.geometry][2] for s in F.states(name)) + 3
    n, _, _ = F.SEQS["S3"]
    assert n == ld_of(n)                                                   # the in-place path
    assert all(F.SEQS[k][0] % 2 == 1 for k in ("S1", "S2", "S4", "S5"))


def test_thresholds_move_sizes_and_widths():
    moves = [(a, b) for name in F.SEQS for a, b in zip(F.states(name), F.states(name)[1:]) if b.action == "move"]
    # every pick_config threshold between two of the geometries 0..3 is crossed by a move (from above to exactly on it)
    for g in range(3):
        assert any(a.geometry == g + 1 and b.geometry == g and b.nch == PICK_THRESHOLDS[g] for a, b in moves), g
    assert {s.geometry for name in F.SEQS for s in F.states(name)} == {0, 1, 2, 3}
    assert any(b.k > 256 for a, b in moves)                                # workgroup 0's map loop runs more than once
    widths = {s.width for name in F.SEQS for s in F.states(name)}
    assert {0, 1, 15} <= {w % 16 for w in widths} and {1, 2, 15, 16, 17} <= widths
    # after a move the stride is larger than the width rounded up
    assert any(s.action == "move" and s.ldf > ld_of(s.width) for name in F.SEQS for s in F.states(name))
    # S1: one move fixes the variable in slot 0, one fixes variables in the last slots
    s1 = F.states("S1")
    assert s1[1].fix[s1[0].map[0]] and not s1[0].fix[s1[0].map[0]]
    w = s1[1].width
    assert all(s1[2].fix[s1[1].map[t]] for t in (w - 1, w - 2, w - 5))
    # S4: the set pushed again is bit for bit the one before; B' has B's count and another set; A frees what B fixed
    s4 = F.states("S4")
    assert np.array_equal(s4[4].fix, s4[3].fix) and s4[5].fix.sum() == s4[3].fix.sum() and not np.array_equal(s4[5].fix, s4[3].fix)
    assert [(s.who, s.action, s.k) for s in s4] == [("A", "build", 0), ("B", "move", 5), ("A", "build", 0), ("B", "move", 5), ("B", "use", 0),
                                                     ("Bp", "build", 0)]
    assert np.all(s4[1].fix[s4[0].fix]) and np.all(s4[5].fix[s4[0].fix])


@pytest.fixture(scope="module")
def header_log(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("free_image_cases")
    src, exe = d / "seq.cpp", d / "seq"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    text = []
    for name in F.SEQS:
        st = F.states(name)
        text.append("Q %d %d" % (F.SEQS[name][0], len(st)))
        text += ["".join("1" if b else "0" for b in s.fix) for s in st]
    out = subprocess.run([str(exe)], input="\n".join(text) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert not any(line.startswith("X") for line in out), out
    return out


def test_the_mirror_agrees_with_the_header(header_log):
    lines = iter(header_log)
    for name in F.SEQS:
        book = F.Book()
        for s in F.states(name):
            head, mp = next(lines).split("|")
            v = head.split()
            assert v[0] == "C"
            act, k, nfree, ldf, builds, moves = (int(x) for x in v[1:])
            assert (ACTIONS[act], k, nfree, ldf, builds, moves) == (s.action, s.k, s.width, s.ldf, s.builds, s.moves), (name, v, s[2:11])
            assert np.array_equal(np.array(mp.split(), dtype=np.int32), s.map), (name, s.width)
            # the mirror's own dst_of_tail, replayed next to the header's
            if s.action == "move":
                dst = book.move(s.fix)
                assert np.array_equal(np.array(next(lines).split()[1:], dtype=np.int32), dst), (name, s.width)
            elif s.action == "build":
                book.build(s.fix)
            assert np.array_equal(book.map, s.map)
    assert next(lines, None) is None


@pytest.mark.parametrize("name", list(F.SEQS))
def test_the_oracle_decides_its_own_iteration_count(name):
    """Every state, both bounds settings: the oracle's projected_cg ends at the same iteration with the same status under every
    re-association of its own H*p; the wide run ends solved, the box run on the boundary (after at least two products wherever the
    wide run takes three or more)."""
    for k, s in enumerate(F.states(name)):
        wide, box = F.cell(name, N_CU, k, "wide"), F.cell(name, N_CU, k, "box")
        for c in (wide, box):
            assert set(c["band"].values()) == {(c["status"], c["iters"])}, (name, k, c["band"])
        assert wide["status"] == int(R.CGStatus.solved) and wide["n_hmul"] == wide["iters"] - 1
        # ... and not by a hair: |r.v| stays a factor MARGIN away from the tolerance it is compared with (:747) in every iteration
        assert all(x == 0.0 or max(x, 1.0 / x) >= F.MARGIN for x in wide["rtv_over_tol"]), (name, k, wide["rtv_over_tol"])
        assert box["status"] == int(R.CGStatus.bound_hit) and box["n_hmul"] == box["iters"]
        # (the exception — S1 at widths 2 and 1, S5 at width 3 — is argued next to TABLE in free_image_cases.py)
        assert box["n_hmul"] >= (1 if (name, s.width) in (("S1", 2), ("S1", 1), ("S5", 3)) else 2), (name, k, box["n_hmul"])
        assert np.all(np.abs(wide["w"]) < 0.1 * F.WIDE) and box["delta"] < F.XB
    assert max(F.cell(name, N_CU, k, "wide")["n_hmul"] for k in range(len(F.states(name)))) <= 64       # the trace holds every row


def test_integer_operands_stay_exact():
    """One exact iteration: every intermediate of every product, in any order, is an integer below 2^52."""
    sets, g = F.exact_sets()
    n = F.EXACT_N
    J = F.exact_jacobian(n, n + 5)
    assert np.array_equal(J, np.rint(J)) and np.abs(J).max() == 4 and np.array_equal(g, np.rint(g)) and np.abs(g).max() <= 7 and np.all(g != 0)
    assert F.exact_magnitude_bound() < 2 ** 52
    assert [n - int(f.sum()) for f in sets] == list(F.EXACT_WIDTHS) and F.EXACT_WIDTHS[1] % 16 == 0 and F.EXACT_WIDTHS[2] == 1
    assert all(np.all(b[a]) for a, b in zip(sets, sets[1:]))              # nested: every step only fixes variables
    Ji = J.astype(np.int64)
    for fix in sets:
        cols = np.flatnonzero(~fix)
        assert np.array_equal(Ji[:, cols].T @ Ji[:, cols], 16 * np.eye(cols.shape[0], dtype=np.int64))
        p = np.where(fix, 0, -g.astype(np.int64))
        # the absolute sums bound every partial sum whatever the order
        t = np.abs(Ji) @ np.abs(p)
        assert int(t.max()) <= 4 * 7 * n and int(t @ t) <= F.exact_magnitude_bound() and int((Ji @ p) @ (Ji @ p)) == 16 * int(p @ p)
