"""GPU tests of the explicit Gram form of the Gauss-Newton Hessian (bh_hess_set_form / AlHessian.set_form("gram")):
G = J'J + mu C'C built on the fp64 matrix cores, every product H*v = G v.  Against the CPU oracle, with the oracle's own
Gram-form variant ((J'J + mu C'C) @ v) added to its iteration band where iteration counts are compared."""
import ctypes as ct
import json
import os

import numpy as np
import pytest

import benlsip_ref as R
import sphere_problem as sp
from _util import (assert_iters_in_oracle_band, assert_w_close, note_tol, oracle_iteration_band, relnorm, w_tolerance)
from hip_ops import HipOpsDeviceAll

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL1 = 1e-12


def _flt(xs):
    return np.array([float(x) for x in xs], dtype=np.float64)


def gram_dense(H):
    """The oracle-side explicit Gram matrix of an oracle AlHessian."""
    return H.J.T @ H.J + H.mu * (H.C.T @ H.C)


def hmul_gram(H, v):
    """Oracle H*v in the Gram form: (J'J + mu C'C) @ v, the matrix formed first (cached per J, C, mu)."""
    key = (id(H.J), id(H.C), float(H.mu))
    if getattr(H, "_gram_key", None) != key:
        H._gram = gram_dense(H)
        H._gram_key = key
    return H._gram @ v


def gram_band(g, Ho, w_l, w_u, cons_o, kappa2):
    """The oracle's iteration band (tests/_util.py) with its Gram-form H*v added as one more variant."""
    band = oracle_iteration_band(g, Ho, w_l, w_u, cons_o, kappa2, variants=["reference", "long double", "C-order sums", "rows reversed"])
    w, st, it = R.projected_cg(g, Ho, w_l, w_u, cons_o, kappa2, hmul_fn=hmul_gram)
    band["explicit Gram"] = (int(st), int(it))
    return band


def product_bar(J, C, mu, v):
    return float(np.linalg.norm(np.abs(J).T @ (np.abs(J) @ np.abs(v)) + mu * np.abs(C).T @ (np.abs(C) @ np.abs(v))))


def _gram(bh, J, C=None, mu=0.0):
    H = bh.AlHessian(J, C, mu)
    H.set_form("gram")
    return H


# ----------------------------------------------------------------------------------------------------------------- products
@pytest.mark.parametrize("d,n,q", [(4, 3, 1), (1, 1, 0), (0, 5, 2), (5, 5, 5), (37, 5, 2), (64, 128, 0), (300, 130, 0), (257, 129, 1),
                                   (1000, 1024, 3), (513, 2049, 0), (256, 4096, 2), (100, 4095, 0), (130, 8000, 1),
                                   (8192, 1024, 0), (3, 600, 0), (40, 16384, 1)])
def test_gram_products(bh, d, n, q):
    """H*v, bh_hmul_dev and bh_hmul_add in the Gram form against the oracle's H*v, within 1e-12 |J|'|J||v| + mu |C|'|C||v|;
    again after a change of mu (one rebuild)."""
    rng = np.random.default_rng(2000 + d + n)
    J, C, mu = rng.standard_normal((d, n)), rng.standard_normal((q, n)), 0.75
    v, g = rng.standard_normal(n), rng.standard_normal(n)
    H, Ho = _gram(bh, J, C, mu), R.AlHessian(J, C, mu)
    assert H.form == "gram" and H.gram_builds == 0
    for step in range(2):
        bar = product_bar(J, C, Ho.mu, v)
        ref = R.hmul(Ho, v)
        hv = H * v
        note_tol("Gram form: H*v vs oracle (1e-12 of |J|'|J||v| + mu |C|'|C||v|)", np.linalg.norm(hv - ref), TOL1 * bar, "d=%d n=%d q=%d" % (d, n, q))
        assert np.linalg.norm(hv - ref) <= TOL1 * bar
        dv, dout = bh.DeviceVector(n, v), bh.DeviceVector(n)
        bh._lib.check(bh._lib.lib().bh_hmul_dev(H.handle, dv.ptr, dout.ptr), "bh_hmul_dev")
        assert np.array_equal(dout.download(), hv)
        hg = bh.hmul_add(H, v, g)
        assert np.linalg.norm(hg - (ref + g)) <= TOL1 * bar + 1e-15 * np.linalg.norm(g)
        assert H.gram_builds == 1 + step
        H.mu = 2.5
        Ho.mu = 2.5
    assert H.stats()["bytes_per_hmul"] == 8.0 * n * ((n + 15) // 16 * 16) + 16.0 * n
    H.close()


def test_gram_matrix_is_exactly_symmetric_and_reproducible(bh):
    rng = np.random.default_rng(7)
    for d, n, q in [(50, 37, 2), (3000, 130, 1), (70000, 70, 0)]:
        J, C = rng.standard_normal((d, n)), rng.standard_normal((q, n))
        H = _gram(bh, J, C, 1.7)
        G = np.stack([H * e for e in np.eye(n)], axis=1)        # column i = G e_i
        assert np.array_equal(G, G.T), (d, n, q)
        assert np.linalg.norm(G - gram_dense(R.AlHessian(J, C, 1.7))) <= TOL1 * np.linalg.norm(np.abs(J).T @ np.abs(J) + 1.7 * np.abs(C).T @ np.abs(C))
        v = rng.standard_normal(n)
        a = H * v
        H.time_kernel(9, reps=1)                                  # two more builds (warm-up + 1)
        assert H.gram_builds == 3
        assert np.array_equal(H * v, a)                           # fixed-order reductions: a rebuild reproduces G bit for bit
        H.close()


def test_set_mu_rebuilds_only_for_a_new_mu(bh):
    rng = np.random.default_rng(8)
    J, C = rng.standard_normal((500, 200)), rng.standard_normal((3, 200))
    v = rng.standard_normal(200)
    H = _gram(bh, J, C, 0.5)
    H * v
    assert H.gram_builds == 1
    for _ in range(3):
        H.mu = 0.5                                                # the Julia shim's handle(H) does this before every call
        H * v
    assert H.gram_builds == 1
    H.mu = 4.0
    assert H.gram_builds == 1                                     # stale, rebuilt by the next product only
    H * v
    H * v
    assert H.gram_builds == 2
    H.close()


def test_switching_back_to_implicit_matches_a_fresh_handle(bh):
    rng = np.random.default_rng(9)
    J, C = rng.standard_normal((2000, 300)), rng.standard_normal((2, 300))
    v = rng.standard_normal(300)
    fresh = bh.AlHessian(J, C, 3.0)
    H = _gram(bh, J, C, 3.0)
    H.set_form("gram")                                            # the current form again: no-op
    g1 = H * v
    H.set_form("implicit")
    assert H.form == "implicit"
    assert np.array_equal(H * v, fresh * v)
    assert H.stats()["bytes_per_hmul"] == fresh.stats()["bytes_per_hmul"]
    H.set_form("gram")
    assert np.array_equal(H * v, g1) and H.gram_builds == 2
    H.close()
    fresh.close()


def test_async_create_then_gram_form(bh):
    rng = np.random.default_rng(10)
    J = rng.standard_normal((20000, 700))
    v = rng.standard_normal(700)
    H = bh.AlHessian.create_async(J, None, 2.0)
    H.set_form("gram")                                            # the upload may still be running: the build waits for it
    hv = H * v
    Ho = R.AlHessian(J, np.zeros((0, 700)), 2.0)
    assert np.linalg.norm(hv - R.hmul(Ho, v)) <= TOL1 * product_bar(J, Ho.C, 2.0, v)
    H.close()


def test_form_errors(bh):
    lib = bh._lib.lib()
    rng = np.random.default_rng(11)
    H = bh.AlHessian(rng.standard_normal((10, 20)), None, 1.0)
    assert lib.bh_hess_set_form(H.handle, 2) == bh._lib.BH_ERR_INVALID_ARG
    assert lib.bh_hess_set_form(H.handle, -1) == bh._lib.BH_ERR_INVALID_ARG
    assert lib.bh_hess_set_form(None, 1) == bh._lib.BH_ERR_INVALID_ARG
    assert H.form == "implicit"
    ms = ct.c_double(0.0)
    assert lib.bh_time_kernel(H.handle, 9, 1, ct.byref(ms)) == bh._lib.BH_ERR_PRECONDITION
    assert lib.bh_time_kernel(H.handle, 10, 1, ct.byref(ms)) == bh._lib.BH_ERR_PRECONDITION
    with pytest.raises(ValueError):
        H.set_form("dense")
    H.close()
    W = bh.AlHessian(rng.standard_normal((2, 16385)), None, 1.0)
    assert lib.bh_hess_set_form(W.handle, 1) == bh._lib.BH_ERR_UNSUPPORTED
    assert W.form == "implicit"
    v = rng.standard_normal(16385)
    assert np.isfinite(W * v).all()                               # still usable in the implicit form
    W.close()


# ------------------------------------------------------------------------------------------------------------- projected_cg
def _load_case(c):
    d, n, q, mA, mpp = c["d"], c["n"], c["q"], c["mA"], c["mpp"]
    J = _flt(c["J"]).reshape((d, n), order="F")
    C = _flt(c["C"]).reshape((q, n), order="F")
    A = _flt(c["A"]).reshape((mA, n), order="F")
    L = _flt(c["L"]).reshape((mpp, mpp), order="F")
    fix = np.array(c["fixvars"], dtype=bool)
    return J, C, A, L, fix, _flt(c["g"]), _flt(c["w_l"]), _flt(c["w_u"])


def test_pcg_golden_fixtures_gram_form(bh):
    """The committed oracle fixtures with a Gram-form handle: status, w, iteration count (identical or inside the oracle's band
    with the Gram variant), and the scalar trace — whose pHp the oracle forms as dot(p, H*p), as the separate-kernel shape does."""
    cases = json.load(open(os.path.join(GOLD, "pcg_cases.json")))["cases"]
    for c in cases:
        J, C, A, L, fix, g, wl, wu = _load_case(c)
        n = c["n"]
        H = _gram(bh, J, C, c["mu"])
        cons = bh.MixedConstraints(A, L, fix)
        w, status, info = bh.projected_cg(g, H, wl, wu, cons, c["kappa2"], trace_cap=64, full_output=True)
        assert H.stats()["cg_kernels"] == 0
        assert int(status) == c["status"], c["name"]
        Ho = R.AlHessian(J, C, c["mu"])
        cons_o = R.MixedConstraints(A, -np.ones(n), np.ones(n), fix, L)
        if info["iters"] != c["iters"]:
            assert_iters_in_oracle_band(info["iters"], gram_band(g, Ho, wl, wu, cons_o, c["kappa2"]), "Gram form: CG iterations vs oracle band",
                                        c["name"])
        w_ref = _flt(c["w"])
        tol = w_tolerance(g, Ho, wl, wu, cons_o, c["kappa2"], w_ref)
        if c["name"] == "maxiter_exhaust":
            tol = 1e-6
        if np.all(np.isfinite(w_ref)):
            assert_w_close(w, w_ref, tol, "Gram form: golden fixtures w", c["name"])
        else:
            assert np.array_equal(np.isnan(w), np.isnan(w_ref)) and np.array_equal(w[np.isfinite(w_ref)], w_ref[np.isfinite(w_ref)])
        tr_ref = np.array([[float(x) for x in row] for row in c["trace"]]).reshape(-1, 4)
        tr = info["trace"]
        if c["name"] != "maxiter_exhaust" and tr.size and info["iters"] == c["iters"]:
            assert tr.shape == tr_ref.shape
            m = np.isfinite(tr_ref)
            assert np.array_equal(np.isnan(tr), np.isnan(tr_ref)), c["name"]
            rt = max(1e-9, tol)
            np.testing.assert_allclose(tr[m], tr_ref[m], rtol=rt, atol=1e-10)
            np.testing.assert_allclose(tr[:, 0], tr_ref[:, 0], rtol=rt, atol=1e-10)      # pHp = dot(p, H*p)
        H.close()
        cons.close()


@pytest.mark.parametrize("d,n,q,mA,nfix,seed", [(50, 20, 0, 0, 4, 1), (300, 100, 0, 0, 0, 3), (1024, 512, 0, 0, 64, 5), (200, 64, 1, 3, 10, 2),
                                                (2000, 1000, 2, 8, 100, 6), (900, 300, 0, 64, 12, 7), (900, 300, 1, 65, 0, 8)])
def test_pcg_random_instances_gram_form(bh, d, n, q, mA, nfix, seed):
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((d, n)) / np.sqrt(d)
    C = rng.standard_normal((q, n))
    A = rng.standard_normal((mA, n))
    L0 = R.chol_lower(A @ A.T)
    fix = np.zeros(n, dtype=bool)
    fix[rng.choice(n, nfix, replace=False)] = True
    cons_o = R.make_mixed_constraints(A, L0, fix if nfix else None, l=-np.ones(n), u=np.ones(n))
    x_minor = np.clip(0.3 * rng.standard_normal(n), -0.9, 0.9)
    x_minor[fix] = 1.0
    g = rng.standard_normal(n)
    w_l, w_u = R.build_step_bounds(x_minor, cons_o, 0.1 * np.linalg.norm(g))
    Ho = R.AlHessian(J, C, 10.0)
    w_ref, s_ref, it_ref = R.projected_cg(g, Ho, w_l, w_u, cons_o, 0.1)
    H = _gram(bh, J, C, 10.0)
    cons = bh.MixedConstraints(A, cons_o.chol_L, fix)
    w, status, info = bh.projected_cg(g, H, w_l, w_u, cons, 0.1, full_output=True)
    assert H.stats()["cg_kernels"] == 0
    assert int(status) == int(s_ref)
    if info["iters"] != it_ref:
        assert_iters_in_oracle_band(info["iters"], gram_band(g, Ho, w_l, w_u, cons_o, 0.1), "Gram form: CG iterations vs oracle band",
                                    "random d=%d n=%d mA=%d" % (d, n, mA))
    # w against the oracle run in the same form (its H*p = (J'J + mu C'C) @ p): the explicit product alone moves the oracle's own w by
    # more than w_tolerance of its implicit run on some instances (3.0e-9 against 1.95e-9 at d=200 n=64 mA=3)
    w_g, s_g, it_g = R.projected_cg(g, Ho, w_l, w_u, cons_o, 0.1, hmul_fn=hmul_gram)
    assert int(s_g) == int(s_ref)
    assert_w_close(w, w_g, w_tolerance(g, Ho, w_l, w_u, cons_o, 0.1, w_g), "Gram form: projected_cg w vs the oracle's Gram form",
                   "random instance d=%d n=%d q=%d mA=%d" % (d, n, q, mA))
    if mA:
        assert np.linalg.norm(A @ w) <= 1e-9 * np.linalg.norm(A) * np.linalg.norm(w)
    assert np.max(np.abs(w[fix]), initial=0.0) <= 1e-12 * np.linalg.norm(w)
    H.close()


def test_pcg_ill_conditioned_synthetic_gram_form(bh):
    """The bench's "ic" Jacobian (columns scaled 10^(-3j/n)) at moderate size: long CG runs in both forms."""
    syn = bh.synthetic
    d, n = 8192, 512
    k = np.arange(d)[:, None] + np.arange(n)[None, :] * d
    J = syn.splitmix_uniform(1, k) / np.sqrt(d) * syn.column_scale(n, 1)[None, :]
    x, x_l, x_u, fix = syn.box_vectors(n, fix_every=8)
    g = J.T @ syn.residual_rows(0, d)
    w_l, w_u = syn.step_bounds(x, x_l, x_u, fix, syn.initial_tr(g))
    Ho = R.AlHessian(J, np.zeros((0, n)), 10.0)
    cons_o = R.make_mixed_constraints(np.zeros((0, n)), R.chol_lower(np.zeros((0, 0))), fix, l=x_l, u=x_u)
    w_ref, s_ref, it_ref = R.projected_cg(g, Ho, w_l, w_u, cons_o, 0.1)
    assert it_ref > 10
    H = _gram(bh, J, None, 10.0)
    cons = bh.MixedConstraints(np.zeros((0, n)), None, fix, l=x_l, u=x_u)
    w, status, info = bh.projected_cg(g, H, w_l, w_u, cons, 0.1, full_output=True)
    assert int(status) == int(s_ref)
    assert_iters_in_oracle_band(info["iters"], gram_band(g, Ho, w_l, w_u, cons_o, 0.1), "Gram form: CG iterations vs oracle band", "ic d=8192 n=512")
    w_g, s_g, it_g = R.projected_cg(g, Ho, w_l, w_u, cons_o, 0.1, hmul_fn=hmul_gram)
    assert_w_close(w, w_g, w_tolerance(g, Ho, w_l, w_u, cons_o, 0.1, w_g), "Gram form: projected_cg w vs the oracle's Gram form", "ic d=8192 n=512")
    H.close()


# -------------------------------------------------------------------------------------------------------------- cauchy_step
@pytest.mark.parametrize("d,n,mA,nact,delta_scale,seed", [(80, 30, 0, 4, 0.5, 1), (500, 200, 0, 0, 5.0, 3), (2000, 512, 0, 40, 2.0, 5),
                                                          (900, 300, 96, 12, 1.0, 7), (1500, 400, 96, 30, 3.0, 8)])
def test_cauchy_step_gram_form(bh, d, n, mA, nact, delta_scale, seed):
    """The H*d form of the Cauchy search (cauchy_image = 0 with box constraints; mA = 96 > 64 always) with a Gram-form handle:
    same breakpoints, same active set, step within 1e-9."""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((d, n)) / np.sqrt(d)
    A = rng.standard_normal((mA, n))
    L0 = R.chol_lower(A @ A.T)
    xlow, xupp = -np.ones(n), np.ones(n)
    x = np.clip(0.5 * rng.standard_normal(n), -0.95, 0.95)
    act = rng.choice(n, nact, replace=False)
    x[act] = np.where(rng.random(nact) < 0.5, -1.0, 1.0)
    g = rng.standard_normal(n)
    delta = delta_scale * 0.1 * np.linalg.norm(g)
    Ho = R.AlHessian(J, np.zeros((0, n)), 10.0)
    cons_o = R.make_mixed_constraints(A, L0, l=xlow, u=xupp)
    n_hmul_ref = [0]

    class Ops(R.NumpyOps):
        def hmul(self, H, v):
            n_hmul_ref[0] += 1
            return R.hmul(H, v)
    s_ref = R.cauchy_step(x, g, Ho, L0, cons_o, delta, Ops())
    bh.set_option("cauchy_image", 0)
    try:
        H = _gram(bh, J, None, 10.0)
        cons = bh.MixedConstraints(A, L0, l=xlow, u=xupp)
        s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
    finally:
        bh.set_option("cauchy_image", 1)
    assert H.gram_builds == 1
    assert np.array_equal(cons.fixvars, cons_o.fixvars), (np.flatnonzero(cons.fixvars), np.flatnonzero(cons_o.fixvars))
    assert info["n_hmul"] == n_hmul_ref[0]
    note_tol("Gram form: cauchy_step vs oracle, 1e-9", np.linalg.norm(s - s_ref), 1e-9 * max(np.linalg.norm(s_ref), 1e-300), "d=%d n=%d mA=%d" % (d, n, mA))
    assert np.linalg.norm(s - s_ref) <= 1e-9 * max(np.linalg.norm(s_ref), 1e-300), relnorm(s, s_ref)
    H.close()


# --------------------------------------------------------------------------------------------------------- config 3, full size
def test_config3_gram_against_implicit(bh):
    """The bench instance (synthetic J 65536 x 4096, 2 GiB): Gram-form H*v against the implicit form within the bar, and
    projected_cg with the same status and iteration count in both forms."""
    syn = bh.synthetic
    d, n = 65536, 4096
    H = bh.AlHessian.synthetic(d, n, seed=1, mu=10.0)
    rng = np.random.default_rng(12)
    v = rng.standard_normal(n)
    # bar: || |J|'|J||v| ||, J regenerated on the host in row chunks (element (i, j) = u(1, i + j d) / sqrt(d))
    absJv = np.empty(d)
    acc = np.zeros(n)
    for lo in range(0, d, 4096):
        Jb = np.abs(syn.splitmix_uniform(1, np.arange(lo, lo + 4096)[:, None] + np.arange(n)[None, :] * d)) / np.sqrt(d)
        absJv[lo:lo + 4096] = Jb @ np.abs(v)
        acc += Jb.T @ absJv[lo:lo + 4096]
    bar = float(np.linalg.norm(acc))
    x, x_l, x_u, fix = syn.box_vectors(n, fix_every=8)
    g = H.jtv(syn.residual_rows(0, d))
    w_l, w_u = syn.step_bounds(x, x_l, x_u, fix, syn.initial_tr(g))
    cons = bh.MixedConstraints(np.zeros((0, n)), None, fix, l=x_l, u=x_u)
    hv_imp = H * v
    w_imp, st_imp, info_imp = bh.projected_cg(g, H, w_l, w_u, cons, 0.1, full_output=True)
    H.set_form("gram")
    hv = H * v
    note_tol("Gram form: config 3 H*v vs implicit (1e-12 of |J|'|J||v|)", np.linalg.norm(hv - hv_imp), TOL1 * bar)
    assert np.linalg.norm(hv - hv_imp) <= TOL1 * bar
    w, st, info = bh.projected_cg(g, H, w_l, w_u, cons, 0.1, full_output=True)
    assert int(st) == int(st_imp) and info["iters"] == info_imp["iters"]
    assert relnorm(w, w_imp) <= 1e-9
    assert H.gram_builds == 1
    H.close()
    cons.close()


# ------------------------------------------------------------------------------------------------------------- whole solves
class HipOpsGram(HipOpsDeviceAll):
    """HipOpsDeviceAll (H*v, projected_cg, minor_iterate, H*s+g, Cauchy search on the device) with every AlHessian in the
    Gram form, as julia/BEnlsipHIP.jl does under gram_hessian!(true)."""

    def new_hessian(self, J, C, mu):
        H = self.bh.AlHessian(J, C, mu)
        H.set_form("gram")
        return H


def test_sphere_regression_gram_form(bh, capsys):
    """BASELINE config 1 through the restated driver with Gram-form handles: the acceptance inequalities of
    test/problems/sphere_regression.jl:63-65 under the rule of test_sphere_regression_through_c_abi."""
    from _util import assert_rounding_dominated, first_decision_difference, sphere_oracle_band
    ops = HipOpsGram(bh)
    log = []
    xs, ys = R.tralcnllss(sp.x0, sp.r, sp.jac_r, sp.c, sp.jac_c, sp.A, sp.b, sp.x_l, sp.x_u,
                          max_outer_iter=100, max_inner_iter=250, ops=ops, log=log)
    assert ops.n_pcg > 10
    grad = sp.jac_r(xs).T @ sp.r(xs) + sp.jac_c(xs).T @ ys
    opt_measure = float(np.linalg.norm(xs - R.projection_polyhedron_small(xs - grad, sp.A, sp.b, sp.x_l, sp.x_u)))
    assert np.linalg.norm(sp.c(xs)) < R.SQRT_EPS
    assert R.is_feasible(xs, sp.A, sp.x_l, sp.x_u, sp.b)
    log_ref = []
    R.tralcnllss(sp.x0, sp.r, sp.jac_r, sp.c, sp.jac_c, sp.A, sp.b, sp.x_l, sp.x_u, max_outer_iter=100, max_inner_iter=250, log=log_ref)
    diff = first_decision_difference(log_ref, log)
    band = sphere_oracle_band()
    with capsys.disabled():
        print("[sphere regression, Gram form] opt_measure = %.3e (%s the reference's 1e-7); oracle band %.2e .. %.2e"
              % (opt_measure, "meets" if opt_measure < 1e-7 else "MISSES", min(band.values()), max(band.values())))
    if diff is not None:
        assert_rounding_dominated(diff)
    assert opt_measure < 2.0 * max(band.values())


def test_full_solve_medium_nls_gram_form(bh, capsys):
    """The 48-parameter constrained NLS of test_full_solve_medium_nls_through_c_abi with Gram-form handles, under its rule for a
    free-running solve: identical driver decisions up to a first, rounding-dominated difference; the same solution."""
    from _util import assert_rounding_dominated, first_decision_difference
    from nls_problem import NLSProblem
    P = NLSProblem(256, 48, 2, seed=1)
    kw = dict(max_outer_iter=30, max_inner_iter=60)
    log_ref = []
    x_ref, y_ref = R.tralcnllss(P.x0, P.r, P.jac_r, P.c, P.jac_c, P.A, P.b, P.x_l, P.x_u, log=log_ref, **kw)
    log = []
    x, y = R.tralcnllss(P.x0, P.r, P.jac_r, P.c, P.jac_c, P.A, P.b, P.x_l, P.x_u, ops=HipOpsGram(bh), log=log, **kw)
    obj = lambda z: 0.5 * float(P.r(z) @ P.r(z))
    diff = first_decision_difference(log_ref, log)
    with capsys.disabled():
        print("[full solve n=48 d=256, Gram form] %d minor iterates (oracle %d); first differing decision: %s"
              % (sum(e[0] == "minor" for e in log), sum(e[0] == "minor" for e in log_ref), "none" if diff is None else diff[0]))
    if diff is None:
        assert len(log) == len(log_ref)
    else:
        assert_rounding_dominated(diff)
        assert diff[0] >= 100
    assert np.linalg.norm(P.c(x)) < 1e-6 and np.linalg.norm(P.A @ x - P.b) < 1e-10
    assert np.all(x >= P.x_l - 1e-12) and np.all(x <= P.x_u + 1e-12)
    assert obj(x) == pytest.approx(obj(x_ref), rel=1e-5)
    assert np.linalg.norm(x - x_ref) <= 1e-4 * np.linalg.norm(x_ref)
