"""Proof, without a device, that the cases of proj_cases.py are what they claim: exact in any order of summation, in agreement with
the oracle, able to see structural errors, and with a `tol` far below their granularity; and what the Newton iteration of
chol_small_body does with an exact and with an inexact seed."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import benlsip_ref as R
import proj_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCED = pc.reduced_cases() + [pc.identity_case()] + pc.sequence_cases() + [pc.cg_case(mA, n) for mA in pc.CG_MA for n in pc.CG_N]
AUGMENTED = pc.augmented_cases()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_mirrors_of_the_source():
    api = open(os.path.join(ROOT, "benlsip.jl_amd", "csrc", "bh_api.hip")).read()
    assert re.search(r"kLdsPerCu = 160 \* 1024;", api) and pc.TRSV_LDS_BYTES == 160 * 1024
    assert re.search(r"return \(5 \* m2 \+ 64 \* 65\) \* sizeof\(double\) <= kLdsPerCu \? 4 : 1;", api)
    assert (pc.trsv_split_for(3264), pc.trsv_split_for(3265)) == (4, 1)       # the last split order and the first single-slice one
    assert sorted(c.mpp for c in AUGMENTED) == sorted(pc.AUG_ORDERS)


def test_the_cases_the_issue_names_are_there():
    red = {(c.mA, c.n) for c in pc.reduced_cases()}
    assert {(m, 131 if m <= 33 else 203) for m in pc.SMALL_MA} <= red and {(m, 523) for m in pc.LARGE_MA} <= red
    assert {(3, 4112), (1, 16), (3, 527)} <= red
    for c in pc.reduced_cases():
        assert c.n % 2 == 1 or c.n in (4112, 16), c
        assert not c.fix[c.n - 1] and np.any(c.A[:, c.n - 1] != 0), "the last column is free and carries data"
    assert [c.nfix for c in pc.reduced_cases() if "nofix" in c.name] == [0, 0]
    assert [(c.mA + c.nfix == c.n) for c in pc.reduced_cases() if "full" in c.name] == [True, True]
    c1, c2, c3 = pc.sequence_cases()
    assert np.all(c2.fix[c1.fix]) and c2.nfix > c1.nfix and np.array_equal(c1.fix, c3.fix) and c1.A is c2.A
    assert np.all(c1.D == 64) and np.all(c2.D == 16)
    assert not same_bits(c1.v, c2.v)


@pytest.mark.parametrize("c", REDUCED, ids=repr)
def test_reduced_cases_are_exact_in_the_kernels_orders(c):
    """T D T' is the masked Gram matrix in integers; the float64 restatements in kernel order (blocked right-looking Cholesky, column
    substitutions or the blocked pair, and the explicit-inverse form) give the rational answer bit for bit; the factor is T sqrt(D) bit
    for bit; A_free v is exactly zero; every accumulated sum of the chain stays below 2^53 units of its terms' granularity."""
    Af = (c.A * ~c.fix[None, :]).astype(np.int64)
    T = c.tri.dense().astype(np.int64)
    assert np.array_equal(Af @ Af.T, (T * c.D[None, :]) @ T.T)
    assert np.all(np.log2(c.D) % 2 == 0) and np.all(np.diag(T) > 0) and np.all(np.log2(np.diag(T)) % 1 == 0)
    L, dinv = pc.chol_blocked((c.A * ~c.fix) @ (c.A * ~c.fix).T)
    assert same_bits(L, c.factor()) and same_bits(dinv, 1.0 / np.diag(c.factor()))
    assert same_bits(pc.restate_reduced(c), c.v)
    if c.mA <= 64:
        assert same_bits(pc.restate_reduced(c, linv=True), c.v)
        assert same_bits(pc.tri_inv(L, dinv), pc.exact_linv(c))
    else:
        assert same_bits(pc.trsv_pair(L, (c.A * ~c.fix) @ c.r, 1), pc.trsv_pair(L, (c.A * ~c.fix) @ c.r, 4))
    assert not np.any(Af.astype(np.float64) @ c.v) and not np.any(c.v[c.fix])
    assert c.sum_bits < 53 and np.all(c.v / c.granularity == np.rint(c.v / c.granularity))
    assert same_bits(c.lm[:c.mA], c.A @ c.x_lm) and same_bits(c.lm[c.mA:], c.x_lm[c.fix])
    ref = c.A.T @ c.y_lmt[:c.mA]
    ref[c.fix] += c.y_lmt[c.mA:]
    assert same_bits(c.lmt, ref)


@pytest.mark.parametrize("c", AUGMENTED, ids=repr)
def test_augmented_cases_are_exact_in_the_kernels_orders(c):
    """v = r - B'(L L')^-1 B r for the factor handed over: the blocked substitution with the trailing update in four slices and in
    one gives the rational answer bit for bit, and that answer solves the system exactly."""
    L = c.factor()
    assert np.all(np.log2(np.diag(L)) % 1 == 0) and not np.any(np.triu(L, 1))
    assert same_bits(pc.restate_augmented(c, split=4), c.v) and same_bits(pc.restate_augmented(c, split=1), c.v)
    t = np.concatenate([c.A @ c.r, c.r[c.fix]])
    assert same_bits(L @ (L.T @ c.y), t)                                 # dyadic operands of a few bits: exact
    assert c.sum_bits < 53
    assert pc.trsv_split_for(c.mpp) == (1 if c.mpp > 3264 else 4)
    assert np.isnan(c.factor_with_nan()[0, -1]) or c.mpp == 1


@pytest.mark.parametrize("c", REDUCED + [a for a in AUGMENTED if a.mpp <= pc.AUG_ORACLE_MAX], ids=repr)
def test_the_oracle_agrees(c):
    """R.projection on the same inputs lies within 1e-10 ||r|| of the exact answer (augmented form: on the factor handed over)."""
    if c.form == 1:
        cons = R.make_mixed_constraints(c.A, R.chol_lower(c.A @ c.A.T), c.fix if c.nfix else None)
    else:
        cons = R.MixedConstraints(c.A, np.full(c.n, -np.inf), np.full(c.n, np.inf), c.fix.copy(), c.factor())
    err = np.linalg.norm(R.projection(cons, c.r) - c.v)
    assert err <= 1e-10 * np.linalg.norm(c.r), (c, err)
    assert np.allclose(R.left_mul(cons, c.x_lm), c.lm, rtol=0, atol=1e-9) and np.allclose(R.left_mul_tr(cons, c.y_lmt), c.lmt, rtol=0, atol=1e-9)


def _moved(a, b):
    return float(np.max(np.abs(a - b), initial=0.0))


@pytest.mark.parametrize("c", REDUCED + AUGMENTED, ids=repr)
def test_the_cases_can_see_structural_errors(c):
    """Each structural change to the restatement moves at least one expected entry by at least the case's granularity (the slice or
    quarter that loses its column is the one that moves the result most: a column whose unknown is zero cannot show).  Not applicable: unmasking without a fixed column (and in the augmented form, which masks nothing), a row swap with one row, a swap in r
    where the free columns are one whole block (the projection is zero whatever r is), a sub-diagonal entry of a diagonal factor, a slice
    of a trailing update where the factor has a single block."""
    g = c.granularity
    free = np.flatnonzero(~c.fix)
    restate = pc.restate_reduced if c.form == 1 else pc.restate_augmented
    if c.form == 1 and c.nfix:
        col = int(np.flatnonzero(c.fix & np.any(c.A != 0, axis=0))[0])
        assert _moved(pc.restate_reduced(c, unmask=col), c.v) >= g, "unmasked column %d" % col
    if c.mA >= 2:
        i, k = [(i, k) for i in range(c.mA) for k in range(i + 1, c.mA) if c.lm[i] != c.lm[k]][0]
        P = np.arange(c.mA)
        P[[i, k]] = k, i
        assert _moved((c.A[P] @ c.x_lm), c.lm[:c.mA]) >= g                     # rows swapped: left_mul moves (the projection cannot)
    if c.form == 0 or c.mA + c.nfix < c.n:
        moved = 0.0
        for a, b in zip(free[:-1], free[1:]):
            if c.r[a] != c.r[b]:
                moved = max(moved, _moved(restate(c, swap_r=(int(a), int(b))), c.v))
                if moved >= g:
                    break
        assert moved >= g
    if pc.zero_sub_diagonal(c.factor()) is not None:
        assert _moved(restate(c, zero_sub=True), c.v) >= g
    if c.form == 1 and c.mA <= 64:
        assert max(_moved(pc.restate_reduced(c, linv=True, drop=q), c.v) for q in range((c.mA + 15) // 16)) >= g
    elif c.order > 64:
        split = pc.trsv_split_for(c.order)
        assert max(_moved(restate(c, drop=(0, q)), c.v) for q in range(split)) >= g


@pytest.mark.parametrize("c", REDUCED, ids=repr)
def test_tol_is_far_below_the_granularity(c):
    print("%s: granularity %g tol %.3e = granularity * %.3e" % (c, c.granularity, c.tol, c.tol / c.granularity))
    assert 0.0 <= c.tol <= c.granularity / 1024.0


def _fl(x):
    return float(x)            # Fraction -> float64 is correctly rounded


def _newton(piv, seed):
    """chol_small_body: rinv <- rinv * fma(-0.5 * piv * rinv, rinv, 1.5), twice, every operation rounded once."""
    rinv = seed
    for _ in range(2):
        h = _fl(Fraction(-0.5 * piv) * Fraction(rinv))
        rinv = _fl(Fraction(rinv) * Fraction(_fl(Fraction(h) * Fraction(rinv) + Fraction(1.5))))
    return rinv


def test_newton_iteration_of_the_reciprocal_square_root():
    """With rational fma: an exact seed 2^-k for a pivot 4^k stays exact through both steps, for every pivot the cases produce; a seed
    with a relative error up to 2^-20 ends exact or one unit in the last place off, and it does end off in a good share of draws."""
    pivots = set()
    for c in REDUCED:
        pivots |= set((np.diag(c.factor()) ** 2).tolist())
    assert pivots and all(np.log2(p) % 2 == 0 for p in pivots)
    for p in sorted(pivots):
        exact = 1.0 / np.sqrt(p)
        assert _newton(p, exact) == exact
    rng = np.random.default_rng(5)
    off = 0
    draws = 400
    for _ in range(draws):
        p = float(rng.choice(sorted(pivots)))
        exact = 1.0 / np.sqrt(p)
        got = _newton(p, exact * (1.0 + float(rng.uniform(-1.0, 1.0)) * 2.0 ** -20))
        assert abs(got - exact) <= np.spacing(exact)
        off += got != exact
    print("inexact seed (|e| <= 2^-20): %d of %d draws end one unit off" % (off, draws))
    assert off > 0


@pytest.mark.parametrize("mA,n", [(mA, n) for mA in pc.CG_MA for n in pc.CG_N])
def test_exact_cg_iteration_on_the_oracle(mA, n):
    """J'J = 16 I: the oracle's projected_cg takes one product, alpha = 1/16, w = -P(g)/16, the residual g - v lies in the row space of
    A_free so the second projection vanishes: solved with iter = 2 and the trace row {16 ||v||^2, 1/16, Inf, ~0}."""
    c = pc.cg_case(mA, n)
    J = pc.cg_jacobian(n)
    assert np.array_equal(J.T @ J, pc.CG_C * np.eye(n))
    cons = R.make_mixed_constraints(c.A, R.chol_lower(c.A @ c.A.T), c.fix)
    tr = R.CGTrace()
    inf = np.full(n, np.inf)
    w, st, it = R.projected_cg(c.r, R.AlHessian(J, np.zeros((0, n)), 1.0), -inf, inf, cons, 0.1, trace=tr)
    vv = float(c.v @ c.v)
    assert vv / c.granularity ** 2 < 2 ** 53
    assert (st, it, tr.n_hmul) == (R.CGStatus.solved, 2, 1)
    assert np.max(np.abs(w + c.v / pc.CG_C)) <= 1e-12
    assert abs(tr.rows[0][0] - pc.CG_C * vv) <= 1e-9 * vv and abs(tr.rows[0][1] - 1.0 / pc.CG_C) <= 1e-12 and tr.rows[0][2] == np.inf
