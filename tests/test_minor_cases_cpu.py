"""tests/minor_cases.py against the source it mirrors, against float64 arithmetic and against the oracle — without a device.

A stale or mistaken generator could hide a kernel bug from the device-side comparison, so everything the cases claim is
checked here: the thread ranges of active_update_kernel / canon_mask_kernel (CG_T and the range rule parsed out of csrc/), the
side of `<= 2^-26` on which every threshold component lies when the reference's expressions are evaluated in float64, the
branch-boundary counts, the ranges each placement lands in, the size of every integer sum, and — case by case — that the
oracle (R.active_bounds, then add_active or active_bounds_inplace; R.linesearch; R.hmul ...) returns the expected results.

It also pins the oracle's own line search to answers derived by hand from src/basic_tralcnlss.jl:776-790 (Julia's `min`
propagates NaN in either position; Python's built-in drops one that comes second)."""
import math
import os
import re

import numpy as np
import pytest

import benlsip_ref as R
import minor_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def same_bits(a, b):
    return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


# ------------------------------------------------------------------------------------------------------- mirror of the source
def test_thread_ranges_mirror_the_kernels():
    m = re.search(r"constexpr\s+int\s+CG_T\s*=\s*(\d+)\s*;", _src("bh_cg.hip.h"))
    assert m and int(m.group(1)) == mc.CG_T
    minor = " ".join(re.sub(r"//[^\n]*", "", _src("bh_minor.hip.h")).split())
    rule = "const int per = (n + CG_T - 1) / CG_T; const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);"
    assert minor.count(rule) == 2, "active_update_kernel / canon_mask_kernel no longer split [0, n) the way minor_cases.thread_range does"
    assert "__launch_bounds__(CG_T) void active_update_kernel" in minor and "__launch_bounds__(CG_T) void canon_mask_kernel" in minor
    assert math.sqrt(np.finfo(np.float64).eps) == mc.ATOL == R.SQRT_EPS


def test_sizes_give_the_range_lengths_they_are_chosen_for():
    assert set(mc.RANGE_LEN) == set(mc.N_EDGE) and max(mc.N_EDGE) == 16384
    for n in mc.N_EDGE:
        lens = [hi - lo for lo, hi in (mc.thread_range(n, t) for t in range(mc.CG_T))]
        assert max(lens) == mc.RANGE_LEN[n] == mc.per_thread(n) and sum(lens) == n
        # the ranges tile [0, n) in thread order
        assert [mc.thread_range(n, t)[0] for t in range(mc.CG_T)] == [min(n, t * mc.per_thread(n)) for t in range(mc.CG_T)]
    assert sorted(set(mc.RANGE_LEN.values())) == [1, 2, 3, 5, 16]
    partial = {n for n in mc.N_EDGE if any(0 < hi - lo < mc.per_thread(n) for lo, hi in (mc.thread_range(n, t) for t in range(mc.CG_T)))}
    empty = {n for n in mc.N_EDGE if mc.thread_range(n, mc.CG_T - 1)[0] == n}
    assert partial == {1025, 2047} and {1, 63, 1023, 1025, 2049, 4100} <= empty and 16384 not in empty and 1024 not in empty
    words = {(n + 63) // 64 for n in mc.N_EDGE}
    assert {1, 2, 16, 17, 256} <= words                      # one word, a word boundary crossed by one, whole and partial last words


# ------------------------------------------------------------------------------------------------------- active-set cases
ACTIVE = mc.active_cases()


def test_active_set_cases_cover_what_they_name():
    names = [c.name for c in ACTIVE]
    assert len(set(names)) == len(names)
    for p in mc.PLACEMENTS:
        assert any(c.placement == p for c in ACTIVE), p
    assert {c.n for c in ACTIVE if c.placement in mc.PLACEMENTS} == set(mc.N_EDGE)
    assert {c.bounds for c in ACTIVE} == set(mc.BOUNDS)
    got = {}
    for c in ACTIVE:
        got.setdefault(c.mA, set()).add(c.n)
    for mA, sizes in mc.MA_SIZES.items():
        assert mA in got and (sizes is None or set(sizes) <= got[mA]), mA
    assert all(np.array_equal(c.A, np.rint(c.A)) and np.abs(c.A).max(initial=0) <= 3 for c in ACTIVE)


@pytest.mark.parametrize("case", [c for c in ACTIVE if c.placement in mc.PLACEMENTS], ids=repr)
def test_placement_lands_in_the_ranges_it_names(case):
    n, per, st = case.n, mc.per_thread(case.n), case.steps[0]
    new, t = st.new, case.thread
    assert np.array_equal(new, case.placed)                    # exactly the placed indices are newly fixed, in index order
    assert not case.fix0[new].any()
    lo, hi = mc.thread_range(n, t) if t >= 0 else (0, 0)
    if case.placement == "none":
        assert new.size == 0
    elif case.placement == "first_last":
        assert set(new.tolist()) == {0, n - 1} and mc.owner(n, 0) == 0 and mc.thread_range(n, mc.owner(n, n - 1))[1] == n
    elif case.placement == "all_free":
        assert np.array_equal(new, np.flatnonzero(~case.fix0))
    elif case.placement == "both_of_range":
        assert per >= 2 and new.tolist() == [lo, lo + 1] and hi - lo >= 2
    elif case.placement == "straddle":
        assert new.tolist() == [hi - 1, hi] and mc.owner(n, hi - 1) == t and mc.owner(n, hi) == t + 1
    elif case.placement == "whole_range":
        assert per >= 2 and new.tolist() == list(range(lo, hi)) and hi - lo == per
    elif case.placement == "partial_last":
        assert hi == n and 0 < hi - lo < per and new.tolist() == list(range(lo, hi))
    # initially fixed variables on their bound count in n_at_bound and are not new
    on_bound = case.fix0 & st.at
    assert st.n_at == new.size + int(on_bound.sum())
    if case.bounds != "inf_bounds" and case.fix0.any():
        assert on_bound.sum() == case.fix0.sum() > 0
    # the second step finds the first step's variables at the bound again, and two others as new
    assert case.steps[1].at[new].all() and not np.isin(case.steps[1].new, new).any()


@pytest.mark.parametrize("case", ACTIVE, ids=repr)
def test_threshold_components_lie_on_their_side_in_float64(case):
    """poly:227-231 in float64, operation by operation: a component said to be at the threshold gives exactly 2^-26, one said to
    be a step outside gives more, and the flags are those of the exact evaluation."""
    with np.errstate(invalid="ignore"):
        for st in case.steps:
            s_l = np.maximum(case.xlow - case.x, -st.delta)
            s_u = np.minimum(case.xupp - case.x, st.delta)
            dl, du = st.s - s_l, s_u - st.s
            k = st.kinds
            assert np.all(dl[k == mc.L_ON] == 0.0) and np.all(du[k == mc.U_ON] == 0.0)
            assert np.all(dl[k == mc.L_THR] == mc.ATOL) and np.all(du[k == mc.U_THR] == mc.ATOL)
            assert np.all(dl[k == mc.L_OUT] == mc.ATOL + mc.STEP) and np.all(du[k == mc.U_OUT] == mc.ATOL + mc.STEP)
            assert np.all(dl[k == mc.L_BELOW] == -(mc.ATOL + 2 * mc.STEP)) and np.all(du[k == mc.U_ABOVE] == -(mc.ATOL + 2 * mc.STEP))
            free_in = (k == mc.IN) & ~case.fix0
            assert np.all(dl[free_in] >= 0.125) and np.all(du[free_in] >= 0.125)
            at = (dl <= mc.ATOL) | (du <= mc.ATOL)
            assert np.array_equal(at, st.at)
            assert np.array_equal(at[~case.fix0], np.isin(k, mc.AT_KINDS)[~case.fix0])
    if case.placement == "threshold" and case.bounds != "inf_both":
        st = case.steps[0]
        kinds = set(st.kinds.tolist())
        assert kinds == set(range(9))
        # every variant against a true bound and against a trust-region face
        true_b = np.where(np.isin(st.kinds, (mc.L_ON, mc.L_THR, mc.L_OUT, mc.L_BELOW)), case.xlow - case.x >= -st.delta, case.xupp - case.x <= st.delta)
        for kk in range(1, 9):
            sel = st.kinds == kk
            if case.bounds == "finite":
                assert true_b[sel].any() and (~true_b[sel]).any(), kk
    if case.bounds == "inf_both":
        assert all(st.n_at == 0 for st in case.steps)


def test_branch_boundary_counts():
    b = [c for c in ACTIVE if c.placement == "boundary"]
    assert len(b) >= 4
    seen = set()
    for c in b:
        assert c.mA >= 1
        for st in c.steps:
            total = c.mA + st.n_at
            assert total in (c.n, c.n + 1) and st.branch == (0 if total == c.n else 1)
            seen.add(total - c.n)
            assert c.mA + int(st.fix.sum()) <= c.n
        if c.steps[0].branch == 1:
            assert c.steps[0].fix.sum() < c.steps[0].n_at         # variables on a trust-region face only are released (:452)
    assert seen == {0, 1}
    assert all(c.mA + st.n_at < c.n for c in ACTIVE if c.placement != "boundary" and c.mA > 0 for st in c.steps)


def oracle_update(cons_o, L0, x, s, delta):
    """src/basic_tralcnlss.jl:439-453 on the oracle: (n_at_bound, branch)."""
    idx = R.active_bounds(cons_o, x, s, delta)
    if cons_o.lineq.shape[0] + idx.shape[0] <= x.shape[0]:
        R.add_active(cons_o, L0, idx)
        return idx.shape[0], 0
    R.active_bounds_inplace(cons_o, x + s, L0)
    return idx.shape[0], 1


@pytest.mark.parametrize("case", ACTIVE, ids=repr)
def test_oracle_gives_the_expected_flags(case):
    L0 = R.chol_lower(case.A @ case.A.T)
    cons_o = R.make_mixed_constraints(case.A, L0, case.fix0 if case.fix0.any() else None, l=case.xlow, u=case.xupp)
    for st in case.steps:
        if st.error:
            with pytest.raises(np.linalg.LinAlgError):
                oracle_update(cons_o, L0, case.x, st.s, st.delta)
            continue
        n_at, branch = oracle_update(cons_o, L0, case.x, st.s, st.delta)
        assert (n_at, branch) == (st.n_at, st.branch)
        assert np.array_equal(cons_o.fixvars, st.fix)
        assert np.all(np.isfinite(cons_o.chol_L))


def test_mask_patterns():
    for n in mc.N_EDGE:
        pats = mc.mask_patterns(n)
        assert set(pats) == {"all_free", "all_fixed", "alternating", "bit63", "bit0", "last_only", "last_word"}
        assert pats["all_fixed"].all() and not pats["all_free"].any() and pats["last_only"].sum() == 1 and pats["last_only"][-1]
        assert pats["bit63"].sum() == n // 64 and pats["bit0"].sum() == (n + 63) // 64
        assert pats["last_word"].sum() == (n - 1) % 64 + 1 and pats["last_word"][-1] and (n <= 64 or not pats["last_word"][0])


# ------------------------------------------------------------------------------------------------------- line search
def _H(J):
    return R.AlHessian(J, np.zeros((0, J.shape[1])), 0.0)


def _quiet(fn, *args):
    with np.errstate(all="ignore"):
        return fn(*args)


def test_oracle_linesearch_answers_derived_by_hand():
    """src/basic_tralcnlss.jl:776-790 with H = I, g = (-1, -1), w = (1, 1): wHw = 2, alpha_opt = 2 / 2 = 1; the loop folds
    w_u[i] / w[i] into alpha_allowed with Julia's min, which returns NaN when either argument is NaN."""
    H = _H(np.eye(2))
    g, w, wl = np.array([-1.0, -1.0]), np.array([1.0, 1.0]), np.array([-1.0, -1.0])
    free = np.zeros(2, dtype=bool)
    nan, inf = math.nan, math.inf
    ls = lambda g, w, wl, wu, fix, H=H: _quiet(R.linesearch, np.asarray(g, float), H, np.asarray(w, float), np.asarray(wl, float), np.asarray(wu, float), np.asarray(fix))
    # NaN first: min(Inf, NaN) = NaN, min(NaN, 1) = NaN, min(1, NaN) = NaN.  NaN second: min(Inf, 1) = 1, min(1, NaN) = NaN
    assert math.isnan(ls(g, w, wl, [nan, 1.0], free))
    assert math.isnan(ls(g, w, wl, [1.0, nan], free))
    # fixed variable: :781 skips it.  alpha_allowed = 4 / 1, alpha_opt = 1
    assert ls(g, w, wl, [nan, 4.0], [True, False]) == 1.0
    assert ls(g, w, [nan, -1.0], [nan, 0.5], [True, False]) == 0.5
    # w_i = +0 / -0: neither `w[i] < 0` nor `w[i] > 0`.  w = (0, 1): wHw = 1, alpha_opt = 1; alpha_allowed = 0.25
    assert ls(g, [0.0, 1.0], [nan, -1.0], [nan, 0.25], free) == 0.25
    assert ls(g, [-0.0, 1.0], [nan, -1.0], [nan, 0.25], free) == 0.25
    # w_l = -Inf, w_i = -Inf: the quotient is NaN (w'Hw = Inf, g.w = NaN: alpha_opt NaN as well)
    assert math.isnan(ls(g, [-inf, 1.0], [-inf, -1.0], [1.0, 1.0], free))
    # wHw == 0 (:776): alpha_opt = Inf, the bound decides: 3 / 1
    assert ls(g, [1.0, 0.0], wl, [3.0, 1.0], free, _H(np.array([[0.0, 1.0]]))) == 3.0
    # w == 0: wHw = 0 and no quotient: min(Inf, Inf)
    assert ls(g, [0.0, 0.0], wl, [1.0, 1.0], free) == inf
    # tie: alpha_opt = 1 and alpha_allowed = 1 / 1: min(1, 1) = 1
    assert ls(g, w, wl, [1.0, 7.0], free) == 1.0
    # finite cases are what they were: alpha_opt = 1 below the bounds, and a bound below alpha_opt
    assert ls(g, w, wl, [2.0, 3.0], free) == 1.0 and ls(g, w, wl, [2.0, 0.125], free) == 0.125
    assert ls(g, [-1.0, -1.0], [-0.5, -3.0], [1.0, 1.0], free) == -1.0     # g.w = 2 > 0: alpha_opt = -1


LS_ALL = [c for n in mc.N_EDGE for c in mc.linesearch_cases(n)]


def test_linesearch_cases_are_what_they_claim():
    by_kind = {}
    for c in LS_ALL:
        by_kind.setdefault(c.name.split("-n")[0], []).append(c)
        assert c.J.shape == (mc.LS_D, c.n) and mc.LS_D <= 16 and np.array_equal(c.J, np.rint(c.J))
        assert abs(c.wHw) < 2 ** 53 and c.gw % (2 ** 40 if abs(c.gw) >= 2 ** 53 else 1) == 0 and abs(c.gw) < 2 ** 59
        with np.errstate(all="ignore"):
            a = R.linesearch(c.g, _H(c.J), c.w, c.w_l, c.w_u, c.fix)
        assert same_bits(a, c.alpha), (c.name, a, c.alpha)
        if c.argmin >= 0:
            k = c.argmin
            q = (c.w_l[k] if c.w[k] < 0 else c.w_u[k]) / c.w[k]
            assert not c.fix[k] and c.w[k] != 0 and q == c.allowed == c.alpha
    assert {c.argmin for c in by_kind["argmin1023"]} == {1023} and {c.argmin for c in by_kind["argmin1024"]} == {1024}
    assert {c.n for c in by_kind["argmin0"]} == set(mc.N_EDGE)
    assert all(c.argmin == c.n - 1 for n in mc.N_EDGE for c in by_kind["argmin%d" % (n - 1)] if c.n == n)
    for c in by_kind["alpha_opt"]:
        assert c.alpha == c.alpha_opt and (c.alpha_opt < c.allowed or c.wHw == 0)
    for c in by_kind["smaller_on_fixed"]:
        k = int(np.flatnonzero(c.fix)[0])
        assert c.w_u[k] / c.w[k] < c.alpha == 1.0 / 3.0
    for c in by_kind["smaller_on_zero_w"]:
        k = c.n // 2                                        # w = +0 at k, -0 at k - 1; either quotient would be -Inf
        assert c.w[k] == 0 and c.w[k - 1] == 0 and math.copysign(1.0, c.w[k]) == 1.0 and math.copysign(1.0, c.w[k - 1]) == -1.0
        with np.errstate(divide="ignore"):
            assert c.w_u[k] / c.w[k] == -math.inf and c.w_l[k - 1] / c.w[k - 1] == -math.inf and c.alpha == 1.0 / 3.0
    for c in by_kind["two_equal"]:
        assert c.w_u[0] / c.w[0] == c.w_u[-1] / c.w[-1] == c.alpha
    for c in by_kind["tie_opt_allowed"]:
        assert c.alpha_opt == c.allowed == c.alpha == 1.0
    for c in by_kind["wHw_zero"]:
        assert c.wHw == 0 and c.alpha_opt == math.inf and np.count_nonzero(c.w) == 1 and c.alpha == 1.0 / 21.0
    assert all(c.alpha == math.inf for c in by_kind["w_zero"])
    for kind in ("nan_on_fixed", "nan_on_zero_w"):
        assert all(math.isfinite(c.alpha) and np.isnan(c.w_u).any() for c in by_kind[kind])
    for c in LS_ALL:
        if c.name.startswith(("nan_bound_at", "inf_over_inf")):
            assert math.isnan(c.alpha) and not np.isfinite([c.w_u[-1], c.w_u[0], c.w[-1]]).all()


# ------------------------------------------------------------------------------------------------------- integer vectors
def test_integer_vector_cases_stay_exact():
    for c in mc.vector_cases():
        assert c.d <= 64 and c.q in (0, 2) and c.max_abs < mc.SUM_LIMIT
        for a in (c.J, c.C, c.s, c.w, c.g, c.r, c.ybar):
            assert np.array_equal(a, np.rint(a))
        assert (2 * c.mu) == int(2 * c.mu)
        Ho = R.AlHessian(c.J, c.C, c.mu)
        # the oracle's own float64 products are exact on these operands: the expected results are the reference's bits
        assert np.array_equal(R.hmul(Ho, c.s) + c.g, c.hs_g) and np.array_equal(R.hmul(Ho, c.s + c.w) + c.g, c.hsw_g)
        assert float(c.g @ c.s) + 0.5 * R.vthv(Ho, c.s) == c.model
        assert np.array_equal(c.J.T @ c.r + c.C.T @ c.ybar, c.grad)
    assert {c.n for c in mc.vector_cases()} == set(mc.VEC_N) and set(mc.VEC_N) <= set(mc.N_EDGE)
    for n in mc.VEC_N:
        cases = mc.norm_cases(n)
        assert any(c.exact for c in cases) and (n < 4 or any(np.isnan(c.g).any() for c in cases))
        for c in cases:
            assert c.S < mc.SUM_LIMIT and not np.isnan(c.g[~c.fix]).any()
            big = c.g[c.fix & ~np.isnan(c.g)] / 2.0 ** 40
            assert np.all(np.abs(big) % 2 == 1)
            Ho = R.make_mixed_constraints(np.zeros((0, n)), np.zeros((0, 0)), c.fix if c.fix.any() else None)
            if not np.isnan(c.g).any():
                assert abs(R.norm_reduced_gradient(c.g, Ho) - math.sqrt(c.S)) <= np.spacing(math.sqrt(c.S))
    for d in mc.N_EDGE:
        r, S = mc.resid_case(d)
        assert S < mc.SUM_LIMIT and float(r @ r) == S
