"""Option free_image_chain on the CPU: the decision rule and the arithmetic of the carried model value.

1. step_acc_select and model_select (csrc/bh_step_chain_plan.h), built with the host compiler into a stand-alone program, over every
   input: both options, step_from_cg, which note names the call (full, compact, none, and — never produced by the library — both),
   whether gm_note matches, and its two flags.  The expected table is restated here from the rule's text.  In particular a g_minor
   whose fixed part is stale never reaches model_from_gminor_kernel, and with the option at 0 and the flags clear the table is the one
   the library had before the option existed.

2. The recurrence q(s + w) = q(s) + sum_free w_i gm_i + (sum_free w_i (Hw)_i) / 2 with fractions.Fraction on the integer instance of
   free_image_cases.py (J'J = 16 I, the three nested active sets of exact_sets): gm is brought up to date on the free variables only,
   its fixed part goes stale as on the device, and after 1, 2 and 3 steps q equals g.s + s'Hs / 2 exactly.

3. free_image_step_accumulate_kernel (csrc/bh_freeimg.hip.h) restated in float64 in the kernel's order — slot c on thread c mod 1024, one
   fma chain per thread in ascending slot order, block_reduce as restated in test_free_image_minor_cpu.py, then
   q + (d1 + 0.5 d2) in three roundings — on every state of S1 ... S5.  It agrees with the same expression evaluated in rationals ON THE
   SAME float64 OPERANDS within gamma_k * sum |terms|, k = the number of roundings on the longest path through the sums (computed
   below from the width), gamma_k = k u / (1 - k u), u = 2^-53."""
import itertools
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import benlsip_ref as R
import free_image_cases as F
from test_free_image_minor_cpu import CG_T, N_CU, _block_reduce, _fma
from test_pcg_plan_cpu import CSRC

SWEEP, FULL, FULL_CARRY, COMPACT, COMPACT_CARRY = range(5)
MODEL_JV, MODEL_FROM_GMINOR, MODEL_CARRIED = range(3)

PROGRAM = r"""
#include "bh_step_chain_plan.h"
#include <cstdio>
int main() {
    for (unsigned b = 0; b < (1u << 7); ++b) {
        auto bit = [&](int i) { return ((b >> i) & 1u) != 0; };
        bh::StepAccIn in{};
        in.step_from_cg = bit(0); in.free_image_chain = bit(1); in.full_note = bit(2); in.compact_note = bit(3);
        in.gm_note_match = bit(4); in.fixed_part_stale = bit(5); in.q_valid = bit(6);
        const bh::StepAccPlan p = bh::step_acc_select(in);
        std::printf("A %u %d %d %d %d %d\n", b, (int)p.path, (int)p.q_init, (int)p.gm_note_set, (int)p.fixed_part_stale, (int)p.q_valid);
    }
    for (unsigned b = 0; b < (1u << 4); ++b) {
        auto bit = [&](int i) { return ((b >> i) & 1u) != 0; };
        std::printf("M %u %d\n", b, (int)bh::model_select(bit(0), bit(1), bit(2), bit(3)));
    }
    // (the options are integers: only 1 switches free_image_chain on, any non-zero value step_from_cg)
    bh::StepAccIn in{};
    in.step_from_cg = 1; in.free_image_chain = 2; in.compact_note = true; in.gm_note_match = true;
    std::printf("X %d\n", (int)bh::step_acc_select(in).path);
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("step_chain_plan")
    src, exe = d / "select.cpp", d / "select"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    acc = {int(f[1]): tuple(int(x) for x in f[2:]) for f in (ln.split() for ln in lines) if f and f[0] == "A"}
    model = {int(f[1]): int(f[2]) for f in (ln.split() for ln in lines) if f and f[0] == "M"}
    extra = [int(f[1]) for f in (ln.split() for ln in lines) if f and f[0] == "X"]
    assert len(acc) == 128 and len(model) == 16 and len(extra) == 1
    return acc, model, extra


def _expected_acc(sfc, chain, full, compact, match, stale, q):
    """(path, q_init, gm_note_set, fixed_part_stale, q_valid), from the text of the rule: the flags count only when gm_note matches."""
    stale, q = stale and match, q and match
    if not sfc:
        return (SWEEP, 0, 1, 0, 0)
    if compact and chain:
        if match and (q or not stale):                       # a q exists, or g_minor is still fully valid: q0 from it
            return (COMPACT_CARRY, int(not q), 1, 1, 1)
        return (COMPACT, 0, 1, 1, 0)                          # the free part only; the model value will cost its J v sweep
    if full:
        if q and chain:
            return (FULL_CARRY, 0, 1, int(stale), 1)
        return (FULL, 0, 1, int(stale), 0)
    return (SWEEP, 0, 1, 0, 0)


def _expected_model(sfc, match, stale, q):
    if not sfc or not match:
        return MODEL_JV
    if q:
        return MODEL_CARRIED
    return MODEL_JV if stale else MODEL_FROM_GMINOR


def test_the_decision_table_over_all_inputs(table):
    acc, model, extra = table
    for b in range(128):
        bits = tuple(bool((b >> i) & 1) for i in range(7))
        assert acc[b] == _expected_acc(*bits), (bits, acc[b], _expected_acc(*bits))
    for b in range(16):
        bits = tuple(bool((b >> i) & 1) for i in range(4))
        assert model[b] == _expected_model(*bits), (bits, model[b])
    assert extra == [SWEEP]                                   # free_image_chain = 2 is not "on" (bh_set_option rejects it anyway)


def test_a_stale_g_minor_never_reaches_model_from_gminor(table):
    acc, model, _ = table
    for sfc, match, stale, q in itertools.product((False, True), repeat=4):
        got = model[sfc | match << 1 | stale << 2 | q << 3]
        if stale and match:
            assert got != MODEL_FROM_GMINOR, (sfc, match, stale, q)
        if stale and match and not q:
            assert got == MODEL_JV
    # ... and whatever accumulate follows on a stale g_minor, the flag survives unless a sweep rewrites all of it
    for b, (path, _, _, stale_out, q_out) in acc.items():
        sfc, chain, full, compact, match, stale, q = (bool((b >> i) & 1) for i in range(7))
        if match and stale and path != SWEEP:
            assert stale_out == 1, (b, path)
        if path in (COMPACT, COMPACT_CARRY):
            assert stale_out == 1
        if q_out:
            assert path in (FULL_CARRY, COMPACT_CARRY) and chain and sfc
        if path == SWEEP:
            assert (stale_out, q_out) == (0, 0)


def test_with_the_option_off_the_table_is_the_one_before_it(table):
    """free_image_chain = 0: a compact note is never written and the flags are never set; the rule is then `step_from_cg and the full
    note matches ? two vector launches : sweep`, and `step_from_cg and gm_note matches ? model_from_gminor : J v`."""
    acc, model, _ = table
    for sfc, full, match in itertools.product((False, True), repeat=3):
        got = acc[sfc | full << 2 | match << 4]
        assert got == ((FULL if sfc and full else SWEEP), 0, 1, 0, 0), (sfc, full, match, got)
        assert model[sfc | match << 1] == (MODEL_FROM_GMINOR if sfc and match else MODEL_JV)


# ------------------------------------------------------------------------------------------------------ the recurrence, exact
def test_the_recurrence_is_exact_on_the_integer_instance():
    sets, g = F.exact_sets()                                  # nested: 140, 128 and 1 free variables; g integer, non-zero everywhere
    n = F.EXACT_N
    J = F.exact_jacobian(n, n)
    assert np.array_equal(J.T @ J, 16.0 * np.eye(n))
    rng = np.random.default_rng(F.EXACT_SEED + 1)
    frac = lambda v: [Fraction(float(x)) for x in v]
    s = frac(rng.integers(-8, 9, n) / 16.0)                   # non-zero on the fixed variables too
    assert any(s[i] != 0 for i in np.flatnonzero(sets[0]))
    gq = frac(g)
    H = lambda v: [16 * x for x in v]
    model = lambda sv: sum(a * b for a, b in zip(gq, sv)) + Fraction(1, 2) * sum(a * b for a, b in zip(sv, H(sv)))
    gm = [a + b for a, b in zip(H(s), gq)]                    # H s + g, valid everywhere
    q = model(s)                                              # q0, while it is
    stale = np.zeros(n, dtype=bool)
    for step, fix in enumerate(sets):
        free = np.flatnonzero(~fix)
        assert not stale[free].any()                          # the active set only grows: no free variable has a stale g_minor
        w = [Fraction(0)] * n
        for i in free:
            w[i] = Fraction(int(rng.integers(1, 9)) * (-1 if rng.random() < 0.5 else 1), 8)
        hw = H(w)
        q = q + sum(w[i] * gm[i] for i in free) + Fraction(1, 2) * sum(w[i] * hw[i] for i in free)
        for i in free:
            gm[i] += hw[i]                                    # the free part only
        stale |= fix
        s = [a + b for a, b in zip(s, w)]
        assert q == model(s), (step, q, model(s))
        exact_gm = [a + b for a, b in zip(H(s), gq)]
        assert all(gm[i] == exact_gm[i] for i in free)
        assert float(q) == float(model(s))                    # (dyadic: the float64 values are the exact ones)


# --------------------------------------------------------------------------------- the kernel's order in float64, S1 ... S5
U = 2.0 ** -53


def kernel_q_update(q, wc, gmc, hwc):
    """free_image_step_accumulate_kernel, q_mode = carry: the new q from the compact operands (gmc = gm[map[c]])."""
    nfree = wc.shape[0]
    d1, d2 = [0.0] * CG_T, [0.0] * CG_T
    for t in range(min(CG_T, nfree)):
        for c in range(t, nfree, CG_T):
            wi = float(wc[c])
            d1[t] = _fma(wi, float(gmc[c]), d1[t])
            d2[t] = _fma(wi, float(hwc[c]), d2[t])
    add = lambda a, b: float(np.float64(a) + np.float64(b))
    s1 = _block_reduce(d1, add, 0.0)
    s2 = _block_reduce(d2, add, 0.0)
    return add(q, add(s1, float(np.float64(0.5) * np.float64(s2))))


def roundings(nfree):
    """Roundings on the longest path: the fma chain of a thread, 6 levels of the wave butterfly, 16 folds, and d1 + d2/2, q + (...)
    (0.5 * d2 is exact)."""
    return -(-nfree // CG_T) + 6 + CG_T // 64 + 2


@pytest.mark.parametrize("name", list(F.SEQS))
def test_the_kernel_order_agrees_with_the_exact_update_on_the_sequences(name):
    I = F.instance(name, N_CU)
    g, Ho, n = I["g"], I["Ho"], I["n"]
    rng = np.random.default_rng(101)
    for k, st in enumerate(F.states(name)):
        m = st.map[:st.width].astype(np.int64)
        s = 0.01 * rng.standard_normal(n)                     # non-zero on the fixed variables too
        gm = R.hmul(Ho, s) + g
        q = float(g @ s) + 0.5 * R.vthv(Ho, s)
        w = np.where(st.fix, 0.0, 0.01 * rng.standard_normal(n))
        hw = R.hmul(Ho, w)
        got = kernel_q_update(q, w[m], gm[m], hw[m])
        t1 = [Fraction(float(w[i])) * Fraction(float(gm[i])) for i in m]
        t2 = [Fraction(float(w[i])) * Fraction(float(hw[i])) / 2 for i in m]
        exact = Fraction(q) + sum(t1) + sum(t2)
        mass = abs(Fraction(q)) + sum(abs(t) for t in t1) + sum(abs(t) for t in t2)
        kk = roundings(st.width)
        gamma = Fraction(kk * U) / (1 - Fraction(kk * U))
        err = abs(Fraction(got) - exact)
        print("[%s state %d width %d] q %r, |error| %.3e, bound gamma_%d * sum|terms| = %.3e" % (name, k, st.width, got, float(err), kk,
                                                                                              float(gamma * mass)))
        assert err <= gamma * mass, (name, k, float(err), float(gamma * mass))
        # the free part of g_minor after the update is vec_add_kernel's: one rounding per element
        assert np.array_equal((gm + hw)[m], np.array([float(np.float64(gm[i]) + np.float64(hw[i])) for i in m]))
