"""Operands and expected results for the exact checks of the minor-loop device steps (pure NumPy, no device, no oracle).

tests/test_minor_cases_cpu.py proves that the cases are what they claim; a device-side test feeds the same operands to the
library (bh_proj_update_active_dev, bh_linesearch(_dev), bh_hmul_add(_dev), bh_step_accumulate_dev, bh_model_reduction_dev,
bh_grad(_dev), bh_resid_sqnorm, bh_reduced_gradient_norm_dev) and compares bit for bit.

Every expected result is computed here in integers:

* active-set cases: all of x, s, the bounds and delta are multiples of 2^-53 below 2 in magnitude, so they are scaled by 2^53
  into int64 and src/polyhedral_constraints.jl:226-231 / :211 are evaluated exactly (+-Inf is a sentinel of +-2^62);
* line-search cases: g.w and ||J w||^2 in int64, alpha_opt is then Python's correctly rounded int / int, every quotient
  w_u[i] / w[i] a single IEEE division, and the `min` is Julia's (NaN propagates) — src/basic_tralcnlss.jl:776-790 literally;
* integer vector cases: int64 throughout.

CG_T mirrors csrc/bh_cg.hip.h (checked by the CPU test): active_update_kernel and canon_mask_kernel give thread t the
contiguous range [t * per, (t + 1) * per) of indices, per = ceil(n / CG_T)."""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

CG_T = 1024
ATOL = 2.0 ** -26                     # sqrt(eps(Float64)): the reference's default atol
STEP = 2.0 ** -53                     # the representable step used next to a threshold
N_EDGE = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 4100, 16384)
RANGE_LEN = {1: 1, 63: 1, 64: 1, 65: 1, 1023: 1, 1024: 1, 1025: 2, 2047: 2, 2049: 3, 4100: 5, 16384: 16}
MA_SIZES = {0: None, 1: (63, 1025), 5: (65, 2049), 64: (1023,), 65: (1024,), 100: (2047, 4100)}

_SCALE = 53
_INF = 1 << 62
_ATOL_I = 1 << (_SCALE - 26)


def per_thread(n):
    return (n + CG_T - 1) // CG_T


def thread_range(n, t):
    per = per_thread(n)
    lo = min(n, t * per)
    return lo, min(n, lo + per)


def owner(n, i):
    """The thread whose range holds index i."""
    return i // per_thread(n)


# --------------------------------------------------------------------------------------------------------- exact arithmetic
def to_fixed(v):
    """float64 array -> int64 multiples of 2^-53 (+-Inf -> +-2^62); asserts that nothing is lost."""
    v = np.asarray(v, dtype=np.float64)
    fin = np.isfinite(v)
    out = np.where(v > 0, _INF, -_INF).astype(np.int64)
    scaled = np.ldexp(np.where(fin, v, 0.0), _SCALE)
    assert np.all(np.abs(scaled) < 2.0 ** 60) and np.all(scaled == np.rint(scaled)), "not a multiple of 2^-53"
    out[fin] = scaled[fin].astype(np.int64)
    return out


def from_fixed(V):
    s = np.ldexp(V.astype(np.float64), -_SCALE)
    assert np.array_equal(np.ldexp(s, _SCALE).astype(np.int64), V), "value is not representable in float64"
    return s


def step_limits_fixed(x, xlow, xupp, delta):
    """s_l = max(xlow - x, -delta), s_u = min(xupp - x, delta) (poly:227-228) in fixed point."""
    X, LO, UP = to_fixed(x), to_fixed(xlow), to_fixed(xupp)
    D = int(to_fixed([delta])[0])
    return np.maximum(LO - X, -D), np.minimum(UP - X, D)


def exact_active(x, s, xlow, xupp, delta):
    """at_bound of active_bounds (poly:231), exactly."""
    SL, SU = step_limits_fixed(x, xlow, xupp, delta)
    S = to_fixed(s)
    return ((S - SL) <= _ATOL_I) | ((SU - S) <= _ATOL_I)


def exact_active_inplace(x, s, xlow, xupp):
    """fixvars of active_bounds!(lincons, x + s, ...) (poly:211), exactly."""
    XS = to_fixed(x) + to_fixed(s)
    return ((XS - to_fixed(xlow)) <= _ATOL_I) | ((to_fixed(xupp) - XS) <= _ATOL_I)


# --------------------------------------------------------------------------------------------------------- active-set cases
# what a component of s is, relative to the nearer-named limit of its variable
IN, L_ON, L_THR, L_OUT, L_BELOW, U_ON, U_THR, U_OUT, U_ABOVE = range(9)
AT_KINDS = (L_ON, L_THR, L_BELOW, U_ON, U_THR, U_ABOVE)
BOUNDS = ("finite", "inf_bounds", "inf_delta", "inf_both")


@dataclass
class Step:
    s: np.ndarray
    delta: float
    kinds: np.ndarray
    at: np.ndarray = None              # expected at_bound
    n_at: int = 0
    branch: int = 0
    fix: np.ndarray = None             # expected fixvars after the step
    new: np.ndarray = None             # expected newly fixed indices, index order (branch 0)
    error: bool = False                # the remaining A_free is rank deficient: the reference's cholesky throws


@dataclass
class ActiveCase:
    name: str
    n: int
    mA: int
    bounds: str
    placement: str
    A: np.ndarray
    x: np.ndarray
    xlow: np.ndarray
    xupp: np.ndarray
    fix0: np.ndarray
    steps: List[Step] = field(default_factory=list)
    placed: Optional[np.ndarray] = None      # indices the placement names (step 1)
    thread: int = -1                         # the thread the placement is about

    def __repr__(self):
        return self.name


def _geometry(n, bounds, fixed_idx):
    """x cycles through 0, 0.75, -0.75 (so with delta = 0.5 the limits are a face on both sides, a true upper bound, a true
    lower bound); an initially fixed variable sits on its bound: x = +-1."""
    x = np.array([0.0, 0.75, -0.75])[np.arange(n) % 3]
    fix0 = np.zeros(n, dtype=bool)
    for k, i in enumerate(fixed_idx):
        fix0[i] = True
        x[i] = 1.0 if k % 2 == 0 else -1.0
    inf_b = bounds in ("inf_bounds", "inf_both")
    xlow = np.full(n, -np.inf if inf_b else -1.0)
    xupp = np.full(n, np.inf if inf_b else 1.0)
    delta = np.inf if bounds in ("inf_delta", "inf_both") else 0.5
    return x, xlow, xupp, fix0, delta


def _side(x_i, i):
    """The limit of magnitude <= 1 next to which a component is placed: the true bound where there is one."""
    if x_i > 0:
        return "U"
    if x_i < 0:
        return "L"
    return "U" if (i // 3) % 2 == 0 else "L"


def make_step(x, xlow, xupp, fix0, delta, variants):
    """variants: {index: 'on' | 'thr' | 'out' | 'past'}; every other free component is strictly inside (0 or +-1/8), every
    initially fixed one has s = 0."""
    n = x.shape[0]
    SL, SU = step_limits_fixed(x, xlow, xupp, delta)
    S = (((np.arange(n) % 3) - 1).astype(np.int64)) << (_SCALE - 3)
    S[fix0] = 0
    kinds = np.full(n, IN)
    one = 1
    for i, var in variants.items():
        side = _side(x[i], i)
        lim = SL[i] if side == "L" else SU[i]
        assert abs(lim) < _INF // 2, "no finite limit on that side"
        sign = 1 if side == "L" else -1          # inward direction
        off = {"on": 0, "thr": _ATOL_I, "out": _ATOL_I + one, "past": -(_ATOL_I + 2 * one)}[var]
        S[i] = lim + sign * off
        kinds[i] = {"L": {"on": L_ON, "thr": L_THR, "out": L_OUT, "past": L_BELOW},
                    "U": {"on": U_ON, "thr": U_THR, "out": U_OUT, "past": U_ABOVE}}[side][var]
    return Step(s=from_fixed(S), delta=delta, kinds=kinds)


def _finish(case):
    """Expected counts, branch and fixvars of every step, by the reference's rule on the exact flags."""
    fix = case.fix0.copy()
    for st in case.steps:
        st.at = exact_active(case.x, st.s, case.xlow, case.xupp, st.delta)
        st.n_at = int(st.at.sum())
        if case.mA + st.n_at <= case.n:                               # src/basic_tralcnlss.jl:441
            st.branch = 0
            st.new = np.flatnonzero(st.at & ~fix)
            fix = fix | st.at
        else:
            st.branch = 1
            st.new = np.zeros(0, dtype=np.int64)
            fix = exact_active_inplace(case.x, st.s, case.xlow, case.xupp)
        st.fix = fix.copy()
    return case


def int_matrix(mA, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, size=(mA, n)).astype(np.float64)


def _placement_indices(n, placement, fix0):
    """(indices, thread) of a named placement, or None where n cannot hold it."""
    per = per_thread(n)
    nthreads = (n + per - 1) // per               # threads with a non-empty range
    free = ~fix0
    t = min(nthreads - 1, max(0, nthreads // 2))
    lo, hi = thread_range(n, t)
    if placement == "none":
        return np.zeros(0, dtype=np.int64), -1
    if placement == "first_last":
        return np.unique([0, n - 1]), -1
    if placement == "all_free":
        return np.flatnonzero(free), -1
    if placement == "both_of_range":
        if hi - lo < 2:
            return None
        return np.array([lo, lo + 1]), t
    if placement == "straddle":
        if nthreads < 2:
            return None
        t = max(0, t - 1)
        lo, hi = thread_range(n, t)
        return np.array([hi - 1, hi]), t
    if placement == "whole_range":
        if per < 2:
            return None
        return np.arange(lo, hi), t
    if placement == "partial_last":
        lo, hi = thread_range(n, nthreads - 1)
        if hi - lo == per:
            return None
        return np.arange(lo, hi), nthreads - 1
    raise ValueError(placement)


PLACEMENTS = ("none", "first_last", "all_free", "both_of_range", "straddle", "whole_range", "partial_last")


def _initially_fixed(n):
    """A few initially fixed variables, clear of the ranges the placements use (thread nthreads // 2 and its left neighbour)."""
    if n < 8:
        return []
    per = per_thread(n)
    return sorted({2, min(n - 2, 5 * per + 1), n - 3})


def placement_cases():
    """Every placement at every n of N_EDGE that can hold it; the bounds rotate through the three settings with finite limits.
    Step 1 fixes the placed indices (alternately exactly on the limit and at the threshold); two free neighbours sit one step
    outside the threshold.  Step 2 runs on the device-side state: it fixes two more variables next to already fixed ones and
    keeps the first step's components where they are (they count in n_at_bound, not as new)."""
    out = []
    k = 0
    for n in N_EDGE:
        for placement in PLACEMENTS:
            if placement == "all_free" and n > 1025:
                continue                                  # the oracle refactors a p x p matrix: keep p small
            fixed_idx = _initially_fixed(n)
            bounds = BOUNDS[k % 3]
            x, xlow, xupp, fix0, delta = _geometry(n, bounds, fixed_idx)
            got = _placement_indices(n, placement, fix0)
            if got is None:
                continue
            k += 1
            idx, t = got
            idx = np.array([i for i in idx if not fix0[i]], dtype=np.int64)
            var = {int(i): ("on" if j % 2 else "thr") for j, i in enumerate(idx)}
            decoys = [i for i in (1, n // 3, n - 2) if 0 <= i < n and not fix0[i] and i not in var][:2]
            if placement != "all_free":
                for j, i in enumerate(decoys):
                    var[int(i)] = "out"
            case = ActiveCase("%s-n%d-%s" % (placement, n, bounds), n, 0, bounds, placement, np.zeros((0, n)), x, xlow, xupp, fix0,
                              placed=idx, thread=t)
            case.steps.append(make_step(x, xlow, xupp, fix0, delta, var))
            var2 = {i: ("past" if v == "thr" else v) for i, v in var.items() if v != "out"}
            more = [i for i in (3, n // 2 + 1, n - 4) if 0 <= i < n and not fix0[i] and i not in var][:2]
            for i in more:
                var2[int(i)] = "thr"
            case.steps.append(make_step(x, xlow, xupp, fix0, delta, var2))
            out.append(_finish(case))
    return out


def threshold_cases():
    """All four variants (on the limit, at 2^-26, one step outside, past the limit) against a true bound and against a
    trust-region face, on both sides, for each bound setting; with both infinite nothing can be placed and nothing is at
    the bound."""
    out = []
    for n in (65, 2049):
        for bounds in BOUNDS:
            x, xlow, xupp, fix0, delta = _geometry(n, bounds, _initially_fixed(n))
            var = {}
            if bounds != "inf_both":
                free = [i for i in range(6, n) if not fix0[i]]
                names = ("on", "thr", "out", "past")
                for j, i in enumerate(free[:24]):               # 24 consecutive: every (x type, side, variant) twice
                    var[i] = names[(j // 6) % 4]
            case = ActiveCase("threshold-n%d-%s" % (n, bounds), n, 0, bounds, "threshold", np.zeros((0, n)), x, xlow, xupp, fix0)
            case.steps.append(make_step(x, xlow, xupp, fix0, delta, var))
            case.steps.append(make_step(x, xlow, xupp, fix0, delta, {i: ("out" if v == "past" else "thr") for i, v in var.items()}))
            out.append(_finish(case))
    return out


def matrix_cases():
    """Linear equalities: integer A, so A_free A_free' and its downdate over the newly fixed columns are exact in any order."""
    out = []
    for mA, sizes in MA_SIZES.items():
        if mA == 0:
            continue
        for n in sizes:
            x, xlow, xupp, fix0, delta = _geometry(n, "finite", _initially_fixed(n))
            got = _placement_indices(n, "straddle", fix0) or _placement_indices(n, "first_last", fix0)
            idx = [int(i) for i in got[0] if not fix0[i]]
            idx += [i for i in (7, n // 4, n // 4 + 1, n - 5) if not fix0[i] and i not in idx]
            var = {i: ("on" if j % 2 else "thr") for j, i in enumerate(idx)}
            var[9] = "out"
            case = ActiveCase("matrix-mA%d-n%d" % (mA, n), n, mA, "finite", "matrix", int_matrix(mA, n, 100 * mA + n), x, xlow, xupp, fix0,
                              placed=np.array(idx))
            case.steps.append(make_step(x, xlow, xupp, fix0, delta, var))
            var2 = {i: v for i, v in var.items() if v != "out"}
            for i in (11, n // 2, n - 6):
                if not fix0[i] and i not in var2:
                    var2[i] = "thr"
            case.steps.append(make_step(x, xlow, xupp, fix0, delta, var2))
            out.append(_finish(case))
    return out


def _unit_lower(m, seed):
    L = np.tril(np.random.default_rng(seed).integers(-1, 2, size=(m, m)), -1).astype(np.float64)
    return L + np.eye(m)


def boundary_cases():
    """mA >= 1 with mA + |active| == n (branch 0: add_active!) and == n + 1 (branch 1: active_bounds!(x + s)).  The columns of
    the variables that stay free hold a unit lower triangular block, so the remaining A_free has full row rank whatever the
    other columns are.  Step 2 repeats the step on the device-side state."""
    out = []
    for n, mA in ((64, 1), (65, 5), (1025, 5)):
        for extra in (0, 1):
            x, xlow, xupp, fix0, delta = _geometry(n, "finite", _initially_fixed(n))
            free = np.flatnonzero(~fix0)
            if extra == 0:
                stay = free[free % 3 == 0][3:3 + mA]         # branch 0: the mA variables that are not at a bound
                not_at = stay
            else:
                not_at = free[free % 3 == 0][3:3 + mA - 1]    # branch 1: one more at the bound
                # ... and active_bounds!(x + s) then frees every variable that is only on a trust-region face (x = 0)
                stay = free[free % 3 == 0]
            var = {int(i): ("on" if j % 2 else "thr") for j, i in enumerate(free) if i not in set(not_at.tolist())}
            A = int_matrix(mA, n, 7 * n + extra)
            A[:, stay[:mA]] = _unit_lower(mA, n)
            case = ActiveCase("boundary-n%d-mA%d-%s" % (n, mA, "n+1" if extra else "n"), n, mA, "finite", "boundary", A, x, xlow, xupp, fix0)
            case.steps.append(make_step(x, xlow, xupp, fix0, delta, var))
            case.steps.append(make_step(x, xlow, xupp, fix0, delta, var))
            out.append(_finish(case))
    return out


def rank_deficient_case():
    """Row 0 of A is 2 e_j and column j is zero below it: once j is fixed, row 0 of A_free is zero, A_free A_free' has an
    exact zero on its diagonal (4 - 2*2), and in the reference I - G'G has the exact zero row j (G[0, j] = 2 / sqrt(4) = 1):
    cholesky throws in both."""
    n, mA, j = 65, 5, 21
    x, xlow, xupp, fix0, delta = _geometry(n, "finite", _initially_fixed(n))
    A = int_matrix(mA, n, 4242)
    A[:, j] = 0.0
    A[0, :] = 0.0
    A[0, j] = 2.0
    case = ActiveCase("rank-deficient-n65-mA5", n, mA, "finite", "rank_deficient", A, x, xlow, xupp, fix0, placed=np.array([j]))
    case.steps.append(make_step(x, xlow, xupp, fix0, delta, {j: "on", 30: "thr", 31: "out"}))
    _finish(case)
    case.steps[0].error = True
    return case


_ACTIVE = None


def active_cases():
    global _ACTIVE
    if _ACTIVE is None:
        _ACTIVE = placement_cases() + threshold_cases() + matrix_cases() + boundary_cases() + [rank_deficient_case()]
    return _ACTIVE


# --------------------------------------------------------------------------------------------------------- mask patterns
def mask_patterns(n):
    """name -> fixvars for the set_active / update_active round trip."""
    i = np.arange(n)
    last_word = i >= 64 * ((n - 1) // 64)
    return {"all_free": np.zeros(n, dtype=bool), "all_fixed": np.ones(n, dtype=bool), "alternating": i % 2 == 0,
            "bit63": i % 64 == 63, "bit0": i % 64 == 0, "last_only": i == n - 1, "last_word": last_word}


MASK_MA = {65: 5, 1025: 5}             # the patterns that leave enough free columns also run with linear equalities here


# --------------------------------------------------------------------------------------------------------- line search
def julia_min(a, b):
    if a != a or b != b:
        return math.nan
    return min(a, b)


def literal_linesearch(gw, wHw, w, w_l, w_u, fix):
    """src/basic_tralcnlss.jl:776-790 word for word; gw, wHw exact (Python numbers)."""
    if wHw > 0:
        alpha_opt = (-gw / wHw) if isinstance(gw, int) and isinstance(wHw, int) else float(np.float64(-gw) / np.float64(wHw))
    else:
        alpha_opt = math.inf
    allowed = math.inf
    with np.errstate(all="ignore"):
        for i in range(len(w)):
            if not fix[i]:
                if w[i] < 0:
                    allowed = julia_min(allowed, float(np.float64(w_l[i]) / np.float64(w[i])))
                elif w[i] > 0:
                    allowed = julia_min(allowed, float(np.float64(w_u[i]) / np.float64(w[i])))
    return julia_min(alpha_opt, allowed), alpha_opt, allowed


@dataclass
class LsCase:
    name: str
    n: int
    J: np.ndarray
    g: np.ndarray
    w: np.ndarray
    w_l: np.ndarray
    w_u: np.ndarray
    fix: np.ndarray
    alpha: float = math.nan
    alpha_opt: float = math.nan
    allowed: float = math.nan
    gw: int = 0
    wHw: int = 0
    argmin: int = -1                   # where the minimising quotient sits (-1: alpha_opt decides, or no quotient)

    def __repr__(self):
        return self.name


LS_D = 16
_LS_J = {}


def ls_matrix(n, zero_col=None):
    """Integer J (LS_D x n, entries in [-2, 2]); zero_col: that column is zero."""
    key = (n, zero_col)
    if key not in _LS_J:
        J = np.random.default_rng(900 + n).integers(-2, 3, size=(LS_D, n)).astype(np.float64)
        if zero_col is not None:
            J[:, zero_col] = 0.0
        _LS_J[key] = J
    return _LS_J[key]


def _ls_base(n, seed):
    """Integer w with few zeros, g = -2^40 w (alpha_opt is far above every quotient, and g.w stays exact: a multiple of 2^40
    below 2^59), bounds whose quotients lie in [3, 8)."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-2, 3, size=n).astype(np.float64)
    i = np.arange(n)
    w_u = 6.0 + (i % 7) / 3.0 + (i % 5)
    w_l = -(6.0 + (i % 11) / 7.0 + (i % 3))
    return w, -(2.0 ** 40) * w, w_l, w_u


def _ls_finish(name, n, J, g, w, w_l, w_u, fix, argmin=-1, force_nan=False):
    c = LsCase(name, n, J, g, w, w_l, w_u, fix, argmin=argmin)
    if np.all(np.isfinite(w)):
        wi = w.astype(np.int64)
        Jw = J.astype(np.int64) @ wi
        c.wHw = int(Jw @ Jw)
        gw = 0
        for a, b in zip(g.tolist(), wi.tolist()):          # g may hold multiples of 2^40: Python integers
            gw += int(a) * int(b)
        c.gw = gw
        c.alpha, c.alpha_opt, c.allowed = literal_linesearch(c.gw, c.wHw, w, w_l, w_u, fix)
    else:
        assert force_nan
        c.alpha = math.nan
    return c


def linesearch_cases(n):
    """The line-search cases that a vector of length n can hold."""
    out = []
    nofix = np.zeros(n, dtype=bool)
    J = ls_matrix(n)
    # alpha_opt decides: small integer g, one correctly rounded division of two exact sums
    w, _, w_l, w_u = _ls_base(n, 11 * n)
    g = -np.abs(np.random.default_rng(n).integers(1, 4, size=n)).astype(np.float64) * np.sign(w)
    if n == 1:
        w[0], g[0] = 2.0, -3.0
    out.append(_ls_finish("alpha_opt-n%d" % n, n, J, g, w, w_l * 2.0 ** 30, w_u * 2.0 ** 30, nofix))
    # the minimising quotient at a named index
    for k in sorted({0, n - 1, 1023, 1024}):
        if k >= n:
            continue
        w, g, w_l, w_u = _ls_base(n, 13 * n + k)
        if k % 2 == 0:
            w[k], w_u[k] = 2.0, 1.0 / 3.0                   # quotient 1/6, rounded once
        else:
            w[k], w_l[k] = -2.0, -1.0 / 3.0
        out.append(_ls_finish("argmin%d-n%d" % (k, n), n, J, g, w, w_l, w_u, nofix, argmin=k))
    if n >= 3:
        k = n // 2
        # a smaller quotient on a fixed variable: ignored (:781)
        w, g, w_l, w_u = _ls_base(n, 17 * n)
        fix = nofix.copy()
        fix[k] = True
        w[k], w_u[k] = 2.0, 1.0 / 64.0
        w[0], w_u[0] = 1.0, 1.0 / 3.0
        out.append(_ls_finish("smaller_on_fixed-n%d" % n, n, J, g, w, w_l, w_u, fix, argmin=0))
        # a smaller (infinite, negative) quotient where w_i = +0 and where w_i = -0: neither branch of :782-785 is taken
        w, g, w_l, w_u = _ls_base(n, 19 * n)
        w[k], w_u[k], w_l[k] = 0.0, -1.0, 1.0
        w[k - 1], w_u[k - 1], w_l[k - 1] = -0.0, -1.0, 1.0
        w[n - 1], w_l[n - 1] = -1.0, -1.0 / 3.0
        out.append(_ls_finish("smaller_on_zero_w-n%d" % n, n, J, g, w, w_l, w_u, nofix, argmin=n - 1))
        # two equal quotients
        w, g, w_l, w_u = _ls_base(n, 23 * n)
        w[0], w_u[0] = 2.0, 2.0 / 3.0
        w[n - 1], w_u[n - 1] = 1.0, 1.0 / 3.0               # fl(fl(2/3) / 2) == fl(1/3): a power-of-two factor
        out.append(_ls_finish("two_equal-n%d" % n, n, J, g, w, w_l, w_u, nofix, argmin=0))
        # NaN bound on a fixed variable / where w_i = +-0: ignored
        w, g, w_l, w_u = _ls_base(n, 29 * n)
        fix = nofix.copy()
        fix[n - 1] = True
        w[n - 1], w_u[n - 1], w_l[n - 1] = 1.0, np.nan, np.nan
        out.append(_ls_finish("nan_on_fixed-n%d" % n, n, J, g, w, w_l, w_u, fix))
        w, g, w_l, w_u = _ls_base(n, 31 * n)
        w[n - 1], w_u[n - 1], w_l[n - 1] = 0.0, np.nan, np.nan
        w[n - 2], w_u[n - 2], w_l[n - 2] = -0.0, np.nan, np.nan
        out.append(_ls_finish("nan_on_zero_w-n%d" % n, n, J, g, w, w_l, w_u, nofix))
    # tie between alpha_opt and alpha_allowed: `min(alpha_opt, alpha_allowed)` (:790) of two equal numbers is that number.
    # w = 2 e_0, g_0 = -||J e_0||^2 * 2: g.w = -wHw, alpha_opt = 1 = w_u[0] / w[0] = 2 / 2
    w = np.zeros(n)
    w[0] = 2.0
    g = np.zeros(n)
    col = J[:, 0].astype(np.int64)
    g[0] = -2.0 * float(int(col @ col))
    if int(col @ col) > 0:
        out.append(_ls_finish("tie_opt_allowed-n%d" % n, n, J, g, w, np.full(n, -2.0), np.full(n, 2.0), nofix, argmin=0))
    # wHw == 0: a zero column of J under the only non-zero w_i -> alpha_opt = Inf (:776), the bound decides
    zc = n // 2
    Jz = ls_matrix(n, zc)
    w = np.zeros(n)
    w[zc] = -3.0
    g = np.arange(n, dtype=np.float64) % 5 - 2.0
    out.append(_ls_finish("wHw_zero-n%d" % n, n, Jz, g, w, np.full(n, -1.0 / 7.0), np.full(n, 1.0), nofix, argmin=zc))
    # w == 0: Inf
    out.append(_ls_finish("w_zero-n%d" % n, n, J, g, np.zeros(n), np.full(n, -1.0), np.full(n, 1.0), nofix))
    # NaN bound of a free, moving variable: NaN, whether it comes first or last in the chain of min
    for k in sorted({0, n - 1}):
        w, g, w_l, w_u = _ls_base(n, 37 * n + k)
        w[k], w_u[k] = 1.0, np.nan
        out.append(_ls_finish("nan_bound_at%d-n%d" % (k, n), n, J, g, w, w_l, w_u, nofix))
    # w_l = -Inf with w_i = -Inf: the quotient is NaN.  (w_i = -Inf also makes g.w and ||J w||^2 non-finite, so alpha_opt may be NaN
    # by itself: this case pins the result, it does not isolate the quotient path — nan_bound_at* do that)
    w, g, w_l, w_u = _ls_base(n, 41 * n)
    w[n - 1], w_l[n - 1] = -np.inf, -np.inf
    out.append(_ls_finish("inf_over_inf-n%d" % n, n, J, g, w, w_l, w_u, nofix, force_nan=True))
    return out


# --------------------------------------------------------------------------------------------------------- integer vectors
VEC_N = (1, 63, 65, 1023, 1025, 2049, 4100, 16384)
GRAM_N_MAX = 4100                      # the Gram form holds n^2 doubles
SUM_LIMIT = 2 ** 53


@dataclass
class VecCase:
    name: str
    n: int
    d: int
    q: int
    mu: float
    J: np.ndarray
    C: np.ndarray
    s: np.ndarray
    w: np.ndarray
    g: np.ndarray
    r: np.ndarray
    ybar: np.ndarray
    hs_g: np.ndarray = None            # H*s + g
    hsw_g: np.ndarray = None           # H*(s + w) + g
    model: float = 0.0                 # g.s + s'Hs / 2
    grad: np.ndarray = None            # J'r + C'ybar
    max_abs: int = 0                   # the largest |partial sum| any order of summation can meet

    def __repr__(self):
        return self.name


def _h2(J, C, m2, v):
    """2 H v = 2 J'(J v) + (2 mu) C'(C v) in int64."""
    return 2 * (J.T @ (J @ v)) + m2 * (C.T @ (C @ v))


def vector_case(n, q):
    d = min(64, 7 + n % 61)
    mu = 0.5 if q and n % 2 else 2.0
    rng = np.random.default_rng(5000 + 10 * n + q)
    J = rng.integers(-3, 4, size=(d, n))
    C = rng.integers(-3, 4, size=(q, n))
    s, w, g = (rng.integers(-3, 4, size=n) for _ in range(3))
    r, ybar = rng.integers(-3, 4, size=d), rng.integers(-3, 4, size=q)
    m2 = int(2 * mu)
    f = lambda a: a.astype(np.float64)
    c = VecCase("vec-n%d-q%d" % (n, q), n, d, q, mu, f(J), f(C), f(s), f(w), f(g), f(r), f(ybar))
    c.hs_g = (_h2(J, C, m2, s) + 2 * g) / 2.0
    c.hsw_g = (_h2(J, C, m2, s + w) + 2 * g) / 2.0
    Js, Cs = J @ s, C @ s
    c.model = float(4 * int(g @ s) + 2 * int(Js @ Js) + m2 * int(Cs @ Cs)) / 4.0
    c.grad = f(J.T @ r + C.T @ ybar)
    aJ, aC = np.abs(J), np.abs(C)
    a = np.abs(s) + np.abs(w)
    Ja, Ca = aJ @ a, aC @ a
    c.max_abs = max(int((2 * (aJ.T @ Ja) + m2 * (aC.T @ Ca) + 2 * np.abs(g)).max()),
                    4 * int(np.abs(g) @ a) + 2 * int(Ja @ Ja) + m2 * int(Ca @ Ca),
                    int((aJ.T @ np.abs(r) + aC.T @ np.abs(ybar)).max()))
    return c


_VEC = {}


def vector_cases():
    for n in VEC_N:
        for q in (0, 2):
            if (n, q) not in _VEC:
                _VEC[(n, q)] = vector_case(n, q)
    return [_VEC[(n, q)] for n in VEC_N for q in (0, 2)]


@dataclass
class NormCase:
    name: str
    n: int
    g: np.ndarray
    fix: np.ndarray
    S: int                             # exact sum of squares over the free variables
    exact: bool                        # S is a perfect square: the result is math.isqrt(S) exactly

    def __repr__(self):
        return self.name


def norm_cases(n):
    """||mask(g)||: integers on the free variables, 2^40 * odd (or one NaN) on the fixed ones, which must not reach the sum."""
    out = []
    rng = np.random.default_rng(7000 + n)
    fix = np.zeros(n, dtype=bool)
    if n >= 4:
        fix[rng.choice(n, max(2, n // 5), replace=False)] = True
        fix[[1, n - 1]] = True
    big = (2.0 ** 40) * (2 * rng.integers(1, 50, size=n) + 1) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    for tag in ("int", "nan", "square"):
        g = rng.integers(-9, 10, size=n).astype(np.float64)
        if tag == "square":
            m = math.isqrt(int((~fix).sum()))
            g[:] = 0.0
            g[np.flatnonzero(~fix)[:m * m]] = 1.0 if n > 1 else 3.0
        g[fix] = big[fix]
        if tag == "nan":
            if not fix.any():
                continue
            g[np.flatnonzero(fix)[-1]] = np.nan
        gi = g[~fix].astype(np.int64)
        S = int(gi @ gi)
        out.append(NormCase("norm-%s-n%d" % (tag, n), n, g, fix.copy(), S, math.isqrt(S) ** 2 == S))
    return out


def resid_case(d):
    r = np.random.default_rng(8000 + d).integers(-9, 10, size=d)
    return r.astype(np.float64), int(r @ r)
