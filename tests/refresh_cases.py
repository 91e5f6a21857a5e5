"""Instances and CPU restatements for the tests of option cauchy_image_refresh (tests/test_cauchy_refresh_cpu.py, _gpu.py).

The row-space Cauchy search carries t_d = J~ d and t_s = J~ s_c over a breakpoint by one rank-one update; the option forms them again
from J every R-th pass.  `bad_instance` is the family on which the carried form loses the step: the large components of d = -g reach
tiny bounds first, one by one over `span` decades, so ||d|| shrinks by 10^span while the carried t_d keeps an absolute error of
k eps ||t_d,0||; the variables that stay free have wide bounds, so the search ends at an interior minimiser whose length
-phi'/phi'' (formed from the damaged t_d) is most of the step."""
import numpy as np

import benlsip_ref as R


def bad_instance(d, n=160, nhit=120, span=8.0, seed=7, jscale=1e-6, theta0=1.0, wide=1e4):
    """J (d x n), x = 0, g, bounds, delta.  Variable i < nhit: d_i = -g_i = 10^(-span i / nhit) (1 + u_i), upper bound at theta_i d_i
    with theta_i = theta0 (i + 1) — every theta_i d_i >= 1e-8 theta0 nhit lies above the sqrt(eps) of active_bounds! (poly:211), so
    no bound is active at the start; variable i >= nhit: d_i at the 10^-span level, bounds +-wide, delta = 1e12 (reached at
    theta = 1e12).  J = jscale N(0, 1): a segment's minimiser lies near ||d||^2 / d'Hd ~ 1 / (d jscale^2) ~ 1e10, orders beyond
    every theta_i and below 1e12 — the search passes all nhit breakpoints and ends inside the next segment, whose length
    -phi'/phi'' times d is a visible share of the step."""
    rng = np.random.default_rng(seed)
    J = jscale * rng.standard_normal((d, n))
    i = np.arange(n)
    dvec = 10.0 ** (-span * np.minimum(i, nhit) / nhit) * (1.0 + rng.random(n))
    g = -dvec
    x = np.zeros(n)
    xlow = -wide * np.ones(n)
    xupp = wide * np.ones(n)
    xupp[:nhit] = theta0 * (i[:nhit] + 1) * dvec[:nhit]
    return J, x, g, xlow, xupp, 1e12


def bad_equalities(mA, n=160, nhit=120, seed=5):
    """Linear equalities for bad_instance: mA rows supported on the variables that stay free (columns nhit..n-1).  With a dense A the
    oracle's own projection (augmented form, -g with components eight decades apart) leaves the step infeasible at 8e-10 ||A|| ||s|| —
    an oracle that is itself 1e-9 off cannot carry a bound of 1e-13; with this support the rows of A are orthogonal to the rows of the
    fixed variables and the oracle is feasible to 1e-16."""
    A = np.zeros((mA, n))
    A[:, nhit:] = np.random.default_rng(seed).standard_normal((mA, n - nhit))
    return A


def hmul_longdouble_rows(H, v):
    """The oracle's H*v with both products accumulated in long double."""
    Jl, Cl, vl = H.J.astype(np.longdouble), H.C.astype(np.longdouble), v.astype(np.longdouble)
    return (Jl.T @ (Jl @ vl) + Cl.T @ ((np.longdouble(H.mu) * Cl) @ vl)).astype(np.float64)


def oracle_step(J, C, mu, A, x, g, xlow, xupp, delta, longdouble=False):
    """The oracle's cauchy_step: (s, final active set, H*d products)."""
    n = J.shape[1]
    C = np.zeros((0, n)) if C is None else C
    A = np.zeros((0, n)) if A is None else A
    L0 = R.chol_lower(A @ A.T)
    Ho = R.AlHessian(J, C, mu)
    cons = R.make_mixed_constraints(A, L0, l=xlow, u=xupp)
    calls = [0]

    class Ops(R.NumpyOps):
        def hmul(self, H, v):
            calls[0] += 1
            return hmul_longdouble_rows(H, v) if longdouble else R.hmul(H, v)
    s = R.cauchy_step(x, g, Ho, L0, cons, delta, Ops())
    return s, np.asarray(cons.fixvars, dtype=bool).copy(), calls[0]


def step_bound(s_oracle, s_oracle_longdouble):
    """b = max(1e-13, 64 sigma) ||s_oracle||, sigma = the oracle's own relative sensitivity (its step with H*d accumulated in long
    double against its float64 step) — the form of the project's bound on w (_util.w_tolerance)."""
    nrm = float(np.linalg.norm(s_oracle))
    sigma = float(np.linalg.norm(s_oracle_longdouble - s_oracle)) / max(nrm, 1e-300)
    return max(1e-13, 64.0 * sigma) * nrm, sigma


def carried_search(J, C, mu, x, g, xlow, xupp, delta, refresh=0):
    """float64 restatement of the device's box-constrained row-space search: t_d, t_s carried by rank-one updates, the two sums from
    them, the decision by the oracle's own next_breakpoint and branch (src/basic_tralcnlss.jl:615-636), and with refresh = R >= 1 both
    images formed again from J at every pass index that is a positive multiple of R.  Returns (s, active set, passes)."""
    n = J.shape[1]
    Jt = J if C is None or C.shape[0] == 0 else np.vstack([J, C])
    w = np.ones(Jt.shape[0])
    w[J.shape[0]:] = mu
    atol = np.sqrt(np.finfo(float).eps)
    fix = ((x - xlow) <= atol) | ((xupp - x) <= atol)                   # active_bounds! (poly:211)
    d = np.where(fix, 0.0, -g)
    d_u = np.minimum(xupp - x, delta)
    d_l = np.maximum(xlow - x, -delta)
    s = np.zeros(n)
    td = Jt @ d
    ts = np.zeros(Jt.shape[0])
    passes = 0
    while True:
        if refresh > 0 and passes > 0 and passes % refresh == 0:
            td = Jt @ d
            ts = Jt @ s
        phi_p = float(np.dot(w * ts, td) + np.dot(g, d))
        phi_pp = float(np.dot(w * td, td))
        passes += 1
        if not (int(fix.sum()) < n):
            break
        theta, ind = R.next_breakpoint(d, s, d_l, d_u, fix)
        delta_t = (-phi_p / phi_pp) if phi_pp > 0 else 0.0
        if phi_p >= 0:
            break
        if phi_p < 0 and phi_pp > 0 and delta_t < theta:
            s = s + delta_t * d
            break
        assert ind >= 0
        s = s + theta * d
        ts = ts + theta * td
        td = td - d[ind] * Jt[:, ind]
        d[ind] = 0.0
        fix[ind] = True
    return s, fix, passes


# ------------------------------------------------------------------------------------------------------------------------------
# Exact instances: integer / dyadic data, every product, sum and quotient on the way exact in fp64 — the step is the same to the
# last bit whatever the order of summation and however often the images are formed again.
# ------------------------------------------------------------------------------------------------------------------------------
def exact_instance(rows, n, q, npass, mu=0.5, mA=0, seed=0, order=None, theta_exp=13):
    """J~ = [J; C] with rows = d + q rows and entries in {-1, 0, 1} 2^-e, 2^e ~ sqrt(rows) (the q rows of C weighted by mu = 1/2);
    x = 0; g_i = -2^(-(i mod 3)), so d_i = 1, 1/2 or 1/4.  npass - 1 variables (a random choice) meet upper bounds one after the other
    at theta = 2^-13 (k + 1) <= 2^-6; every other bound is +-1024 and delta = 64, reached at theta >= 64.  The minimiser of a segment
    lies near ||d||^2 / d'Hd ~ 1/2 — between the two — so the search passes the npass - 1 breakpoints and ends inside the next
    segment (the CPU test checks the count with the oracle).  Every t_d, t_s, phi', phi'' is a dyadic rational of fewer than 50 bits:
    exact in fp64 in any order; the last step -phi'/phi'' is one correctly rounded quotient of two exact numbers.
    With mA > 0 a matrix A with entries in {-1, 0, 1} is returned too (its projection is not dyadic).
    `order`: the explicit hitting order of the npass - 1 bounded variables (default: the random choice above, drawn either way so
    that J~ does not depend on it).  `theta_exp` = t: breakpoints at 2^-t (k + 1), at most 2^(t - 6) - 1 of them so that the last
    one stays at or below 2^-6 (the default 13 allows 127; tests/test_gram_cases_cpu.py proves 14 with 129 exact)."""
    assert npass - 1 <= min(2 ** (theta_exp - 6) - 1, n)
    rng = np.random.default_rng(1000 + seed)
    d = rows - q
    e = int(round(0.5 * np.log2(rows)))
    Jt = rng.integers(-1, 2, size=(rows, n)).astype(np.float64) * 2.0 ** -e
    J, C = Jt[:d], Jt[d:]
    g = -(2.0 ** -(np.arange(n) % 3).astype(np.float64))
    x = np.zeros(n)
    xlow, xupp = -1024.0 * np.ones(n), 1024.0 * np.ones(n)
    drawn = rng.permutation(n)[:max(npass - 1, 0)]
    if order is None:
        order = drawn
    order = np.asarray(order, dtype=np.int64)
    assert order.shape == (max(npass - 1, 0),) and np.unique(order).size == order.size and (order.size == 0 or (0 <= order.min() and order.max() < n))
    for k, i in enumerate(order):
        xupp[i] = (2.0 ** -theta_exp) * (k + 1) * (-g[i])
    A = rng.integers(-1, 2, size=(mA, n)).astype(np.float64) if mA else np.zeros((0, n))
    return J, C, mu, A, x, g, xlow, xupp, 64.0


def exact_equality_instance(rows, n, q, npass, mA, per_row=4, mu=0.5, seed=0, theta_exp=13):
    """exact_instance with mA linear equalities that keep every quantity dyadic: the rows of A have disjoint supports of per_row (a
    power of 4) entries +-1 on variables that never reach a bound, so A_free A_free' = per_row I for the whole search — its Cholesky
    factor sqrt(per_row) I, the two solves, y = A(-g) / per_row, d = -D g - D A'y, a = J~ D g, B = J~ D A' and t_d = -a - B y are
    exact in fp64 whatever form (augmented or reduced projector, per-thread or tiled row body, GEMM or sweeps) computes them."""
    assert per_row in (4, 16) and mA * per_row + npass - 1 <= n
    J, C, mu, _, x, g, xlow, xupp, delta = exact_instance(rows, n, q, npass, mu=mu, seed=seed, theta_exp=theta_exp)
    rng = np.random.default_rng(2000 + seed)
    never_hit = np.flatnonzero(xupp == 1024.0)
    cols = rng.permutation(never_hit)[:mA * per_row].reshape(mA, per_row)
    A = np.zeros((mA, n))
    for r in range(mA):
        A[r, cols[r]] = rng.choice([-1.0, 1.0], per_row)
    return J, C, mu, A, x, g, xlow, xupp, delta
