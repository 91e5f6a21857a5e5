"""Option free_image_minor on the CPU: the plan rule and the arithmetic of the line search on the compact operands.

1. pcg_select (csrc/bh_pcg_plan.h) with the field hw_free_part_ok, built into a host program as tests/test_pcg_plan_cpu.py does, over
   the whole cross product of the existing inputs x the new bit.  With the bit clear the packed selection is the documented rule of
   test_pcg_plan_cpu.expected; with it set, free_image_eligible loses its "no H*w wanted" term and nothing else changes.

2. free_image_linesearch_kernel (csrc/bh_freeimg.hip.h) restated in NumPy with rational fused multiply-adds: slot i belongs to thread
   i mod 1024, one fma chain per thread in ascending slot order, the butterfly of wave_reduce (a balanced tree over the 64 lanes), the
   16 wave results folded in order from the identity — against R.linesearch on the FULL vectors, w zero on the fixed variables, its
   w'Hw taken as dot(w, H*w) from the full H*w (what linesearch_kernel gets under ls_from_cg = 1).  The compact form reads g, w, the
   bounds and H*w through the slot -> column map and knows no mask.  The two are the same function of the free part: equal bits on
   dyadic data (every sum exact in any order), within 4 ulps on the real-valued instances of free_image_cases.py (they differ by
   the order of two sums of at most 1030 terms)."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import benlsip_ref as R
import free_image_cases as F
from test_pcg_plan_cpu import BITS, CG_FUSED, CSRC, MA, expected

CG_T = 1024
N_CU = 256                                     # the MI355X (only the row count of the instances depends on it)

PROGRAM = r"""
#include "bh_pcg_plan.h"
#include <cstdio>
#include <vector>
int main() {
    const long long mAs[] = {0, 1, 2, 64, 65};
    std::vector<unsigned short> out;
    out.reserve(30u << 20);
    for (long long mA : mAs) for (long long cg_fused = 0; cg_fused < 3; ++cg_fused) for (unsigned b = 0; b < (1u << 21); ++b) {
        auto bit = [&](int i) { return ((b >> i) & 1u) != 0; };
        bh::PcgSelectIn in{};
        in.mA = mA; in.cg_fused = cg_fused;
        in.gram_handle = bit(0); in.gram_cg_fused = bit(1); in.linv_refine = bit(2); in.fold_init = bit(3);
        in.comm = bit(4); in.peer_path = bit(5); in.reduced = bit(6); in.tpart = bit(7); in.W = bit(8); in.M_valid = bit(9);
        in.lda_is_ld = bit(10); in.rs_cfg_ok = bit(11); in.cgp3_ok = bit(12); in.peer_blocks_fit = bit(13); in.iterates = bit(14);
        in.g_padded = bit(15); in.vectors_in_regs = bit(16); in.hw_wanted = bit(17); in.atol_f2b_positive = bit(18);
        in.allow_free_image = bit(19);
        in.hw_free_part_ok = bit(20);
        const bh::PcgSelection s = bh::pcg_select(in);
        out.push_back((unsigned short)((int)s.shape | s.fuse_gen << 2 | s.gen_linv << 3 | s.linv_refine << 4 | s.peer_fused << 5 |
                                       s.rccl_gen << 6 | s.free_image_eligible << 7 | s.fold_init << 8 | s.cg_kernels << 9));
    }
    return std::fwrite(out.data(), sizeof(unsigned short), out.size(), stdout) == out.size() ? 0 : 1;
}
"""
FREE_IMAGE_BIT = np.uint16(1 << 7)


@pytest.fixture(scope="module")
def selections(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("pcg_plan_minor")
    src, exe = d / "select.cpp", d / "select"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    raw = subprocess.run([str(exe)], check=True, capture_output=True).stdout
    out = np.frombuffer(raw, dtype=np.uint16)
    assert out.size == len(MA) * len(CG_FUSED) << 21
    return out.reshape(len(MA), len(CG_FUSED), 2, 1 << 20)


def test_the_new_input_only_lifts_the_hw_term_of_free_image_eligible(selections):
    assert len(BITS) == 20
    b = np.arange(1 << 20, dtype=np.uint32)
    v = {name: ((b >> i) & 1).astype(bool) for i, name in enumerate(BITS)}
    no_hw = dict(v, hw_wanted=np.zeros_like(v["hw_wanted"]))
    lifted = 0
    for i, mA in enumerate(MA):
        for j, cg_fused in enumerate(CG_FUSED):
            rule = expected(mA, cg_fused, v)
            clear, with_bit = selections[i, j, 0], selections[i, j, 1]
            bad = np.flatnonzero(clear != rule)
            assert bad.size == 0, ("bit clear", mA, cg_fused, {n: int(v[n][bad[0]]) for n in BITS}, int(clear[bad[0]]), int(rule[bad[0]]))
            # bit set: everything but the eligibility as before, the eligibility as for a call that wants no H*w
            want = (rule & ~FREE_IMAGE_BIT) | (expected(mA, cg_fused, no_hw) & FREE_IMAGE_BIT)
            bad = np.flatnonzero(with_bit != want)
            assert bad.size == 0, ("bit set", mA, cg_fused, {n: int(v[n][bad[0]]) for n in BITS}, int(with_bit[bad[0]]), int(want[bad[0]]))
            changed = np.flatnonzero(with_bit != clear)
            assert np.all(v["hw_wanted"][changed]) and np.all((with_bit[changed] ^ clear[changed]) == FREE_IMAGE_BIT)
            lifted += changed.size
            assert (changed.size > 0) == (mA == 0 and cg_fused != 0), (mA, cg_fused, changed.size)
    assert lifted > 0


def test_the_default_of_the_new_input_is_false():
    hdr = open(os.path.join(CSRC, "bh_pcg_plan.h")).read()
    assert "bool hw_free_part_ok;" in hdr and "(!in.hw_wanted || in.hw_free_part_ok)" in hdr


# ------------------------------------------------------------------------------------------------ the line search, restated
def _fl(x):
    return float(x)            # Fraction -> float64 is correctly rounded


def _fma(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))          # (no finite rounding to get wrong)
    return _fl(Fraction(a) * Fraction(b) + Fraction(c))


def _julia_min(a, b):
    """OpMinNan of csrc/bh_reduce.hip.h."""
    return a if a != a else (b if b != b else (a if a < b else b))


def _block_reduce(x, op, identity):
    """block_reduce<1024, 1>: wave_reduce is a butterfly — with a commutative op, a balanced tree over the lanes in their order —
    and the 16 wave results are folded in order, starting from the identity."""
    waves = []
    for w in range(CG_T // 64):
        level = list(x[64 * w:64 * (w + 1)])
        while len(level) > 1:
            level = [op(level[2 * k], level[2 * k + 1]) for k in range(len(level) // 2)]
        waves.append(level[0])
    t = identity
    for s in waves:
        t = op(t, s)
    return t


def compact_linesearch(gc, wc, wlc, wuc, hwc):
    """free_image_linesearch_kernel's first pass and alpha on nfree = len(wc) slots: (alpha, g.w, w.hw)."""
    nfree = wc.shape[0]
    gw, whw, amin = [0.0] * CG_T, [0.0] * CG_T, [np.inf] * CG_T
    with np.errstate(all="ignore"):
        for t in range(min(CG_T, nfree)):
            for i in range(t, nfree, CG_T):
                wi = float(wc[i])
                gw[t] = _fma(float(gc[i]), wi, gw[t])
                whw[t] = _fma(wi, float(hwc[i]), whw[t])
                if wi < 0.0:
                    amin[t] = _julia_min(amin[t], float(np.float64(wlc[i]) / np.float64(wi)))
                elif wi > 0.0:
                    amin[t] = _julia_min(amin[t], float(np.float64(wuc[i]) / np.float64(wi)))
        add = lambda a, b: float(np.float64(a) + np.float64(b))
        s_gw = _block_reduce(gw, add, 0.0)
        s_min = _block_reduce(amin, _julia_min, np.inf)
        s_whw = _block_reduce(whw, add, 0.0)
        alpha_opt = float(np.float64(-s_gw) / np.float64(s_whw)) if s_whw > 0.0 else np.inf
    return _julia_min(alpha_opt, s_min), s_gw, s_whw


def _full_linesearch(g, Ho, w, w_l, w_u, fix, hw):
    """R.linesearch on the full vectors, w'Hw = dot(w, H*w) with the full H*w."""
    return R.linesearch(g, Ho, w, w_l, w_u, fix, vthv_fn=lambda H, v: float(np.dot(v, hw)))


def _ulps(a, b):
    if a == b:
        return 0
    ia, ib = (int(np.float64(x).view(np.int64)) for x in (a, b))
    assert (ia < 0) == (ib < 0), (a, b)
    return abs(ia - ib)


def test_compact_line_search_equals_the_full_one_on_dyadic_data():
    """Integers over a power of two: every product and every sum is exact in any order, so the two forms give the same bits.  Widths one
    slot short of and six slots past CG_T, a handful of slots, and one; bounds that do and do not bind; w'Hw = 0 (alpha from the
    bounds alone); a NaN bound on a free variable (NaN-propagating min)."""
    rng = np.random.default_rng(5)
    for n, width, variant in [(2101, 1030, "free"), (2101, 1023, "binds"), (301, 17, "binds"), (301, 1, "free"), (77, 3, "flat"),
                              (301, 140, "nan")]:
        fix = np.ones(n, dtype=bool)
        fix[rng.choice(n, width, replace=False)] = False
        m = rng.permutation(np.flatnonzero(~fix))                       # slot -> column, any order
        w = np.where(fix, 0.0, rng.integers(1, 9, n) / 8.0 * np.where(rng.random(n) < 0.5, -1.0, 1.0))
        g = rng.integers(-16, 17, n) / 4.0
        hw = rng.integers(-32, 33, n) / 16.0                            # non-zero on the fixed variables too: w is zero there
        hw[~fix] = np.abs(hw[~fix]) * np.sign(w[~fix])                  # w.hw >= 0
        if variant == "flat":
            hw[~fix] = 0.0
        w_l, w_u = np.full(n, -np.inf), np.full(n, np.inf)
        w_l[fix], w_u[fix] = -0.5, 0.25                                  # (the full form masks them, the compact one never sees them)
        if variant in ("binds", "flat", "nan"):
            w_l[~fix], w_u[~fix] = -rng.integers(1, 9, width) / 64.0, rng.integers(1, 9, width) / 64.0
        if variant == "nan":
            k = m[np.flatnonzero(w[m] != 0.0)[3]]
            w_l[k] = w_u[k] = np.nan
        Ho = R.AlHessian(np.zeros((1, n)), np.zeros((0, n)), 0.0)
        a_full = _full_linesearch(g, Ho, w, w_l, w_u, fix, hw)
        a_c, gw, whw = compact_linesearch(g[m], w[m], w_l[m], w_u[m], hw[m])
        assert gw == float(np.dot(g, w)) and whw == float(np.dot(w, hw)), (n, width, variant)
        if variant == "nan":
            assert np.isnan(a_full) and np.isnan(a_c)
        else:
            assert np.float64(a_c).view(np.uint64) == np.float64(a_full).view(np.uint64), (n, width, variant, a_c, a_full)
            assert np.isfinite(a_c) and (variant != "flat" or a_c > 0.0)


@pytest.mark.parametrize("name", list(F.SEQS))
def test_compact_line_search_is_within_4_ulps_of_the_full_one_on_the_sequences(name):
    """Every state of a sequence of free_image_cases.py, the oracle's CG direction for the wide and for the box bounds of the cell (the box
    run ends on a bound of a free variable: the quotient minimum decides alpha there), operands gathered through the state's map."""
    I = F.instance(name, N_CU)
    g, Ho = I["g"], I["Ho"]
    worst = 0
    for k, st in enumerate(F.states(name)):
        m = st.map[:st.width].astype(np.int64)
        for setting in ("wide", "box"):
            c = F.cell(name, N_CU, k, setting, band=False)
            w = c["w"]
            assert not w[st.fix].any()
            hw = R.hmul(Ho, w)
            a_full = _full_linesearch(g, Ho, w, c["w_l"], c["w_u"], st.fix, hw)
            a_c, _, _ = compact_linesearch(g[m], w[m], c["w_l"][m], c["w_u"][m], hw[m])
            u = _ulps(a_c, a_full)
            worst = max(worst, u)
            print("[%s state %d width %d %s] alpha compact %r full %r: %d ulps" % (name, k, st.width, setting, a_c, a_full, u))
            assert u <= 4, (name, k, setting, a_c, a_full, u)
    print("[%s] worst distance %d ulps" % (name, worst))
