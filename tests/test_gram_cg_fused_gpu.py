"""GPU tests of the fused CG iteration on a Gram-form handle (option gram_cg_fused, gram_cg_kernel): two kernels per
iteration with box constraints, three with up to 64 linear equalities, the separate-kernel shape everywhere else.  Against answers
derived by hand, the committed fixtures, the oracle's own Gram-form run ((J'J + mu C'C) @ p) and the same handle with the option off.
Every tolerance is the project's own (w_tolerance, the oracle's iteration band, 1e-12 of the operands' scale), computed here from the
oracle."""
import ctypes as ct
import json
import os

import numpy as np
import pytest

import benlsip_ref as R
from _util import assert_iters_in_oracle_band, assert_w_close, closed_form_cases, note_tol, w_tolerance
from test_gn_gram_gpu import GOLD, TOL1, _flt, _gram, _load_case, gram_band, gram_dense, hmul_gram

pytestmark = pytest.mark.gpu


@pytest.fixture
def fused(bh):
    """Option gram_cg_fused = 1 for the duration of one test; no other test sees it."""
    bh.set_option("gram_cg_fused", 1)
    try:
        yield bh
    finally:
        bh.set_option("gram_cg_fused", 0)


def expected_kernels(n, mA, nfix):
    """stats.cg_kernels of a Gram-form handle under the option, reduced projection form, g staged by the host entry point."""
    if 2 * (n - mA - nfix) < 1 or mA > 64:
        return 0
    return 2 if mA == 0 else 3


# --------------------------------------------------------------------------------------------------------- hand-derived answers
def test_answers_derived_by_hand(fused):
    bh = fused
    for c in closed_form_cases():
        n = c["g"].shape[0]
        H = _gram(bh, c["J"], c["C"], c["mu"])
        cons = bh.MixedConstraints(c["A"], None, c["fix"])
        w, st, info = bh.projected_cg(c["g"], H, c["wl"], c["wu"], cons, c["kappa2"], full_output=True)
        assert H.stats()["cg_kernels"] == expected_kernels(n, c["A"].shape[0], int(c["fix"].sum())), (c["name"], H.stats()["cg_kernels"])
        assert (int(st), info["iters"], info["n_hmul"]) == (c["status"], c["iters"], c["n_hmul"]), (c["name"], int(st), info)
        if c["rtol"]:
            assert np.max(np.abs(w - c["w"])) <= c["rtol"] * np.max(np.abs(c["w"])), (c["name"], w, c["w"])
        else:
            assert np.array_equal(w, c["w"]), (c["name"], w, c["w"])
        H.close()
        cons.close()


# ------------------------------------------------------------------------------------------------------------- golden fixtures
def test_golden_fixtures(fused):
    """tests/golden/pcg_cases.json under the checks of test_pcg_golden_fixtures_gram_form: status, w, iteration count (identical or
    inside the oracle's band with its Gram variant) and the scalar trace, column 0 included: pHp is dot(p, H*p) here too."""
    bh = fused
    shapes = set()
    for c in json.load(open(os.path.join(GOLD, "pcg_cases.json")))["cases"]:
        J, C, A, L, fix, g, wl, wu = _load_case(c)
        n = c["n"]
        H = _gram(bh, J, C, c["mu"])
        cons = bh.MixedConstraints(A, L, fix)
        w, status, info = bh.projected_cg(g, H, wl, wu, cons, c["kappa2"], trace_cap=64, full_output=True)
        assert H.stats()["cg_kernels"] == expected_kernels(n, c["mA"], int(fix.sum())), (c["name"], H.stats()["cg_kernels"])
        shapes.add(H.stats()["cg_kernels"])
        assert int(status) == c["status"], c["name"]
        Ho = R.AlHessian(J, C, c["mu"])
        cons_o = R.MixedConstraints(A, -np.ones(n), np.ones(n), fix, L)
        if info["iters"] != c["iters"]:
            assert_iters_in_oracle_band(info["iters"], gram_band(g, Ho, wl, wu, cons_o, c["kappa2"]), "Gram fused CG: golden fixtures, iterations vs oracle band",
                                        c["name"])
        w_ref = _flt(c["w"])
        tol = w_tolerance(g, Ho, wl, wu, cons_o, c["kappa2"], w_ref)
        if c["name"] == "maxiter_exhaust":
            tol = 1e-6
        if np.all(np.isfinite(w_ref)):
            assert_w_close(w, w_ref, tol, "Gram fused CG: golden fixtures w", c["name"])
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
    assert 2 in shapes


# --------------------------------------------------------------------------------------- one shape per geometry, against the oracle
def _instance(d, n, q, mA, nfix, seed, wide):
    """J / sqrt(d), g = J'r (so p'Hp = ||J p||^2 + mu ||C p||^2 > 0 also where d < n), some fixed variables; `wide`: bounds far away (the
    loop runs until solved), else the trust region of the random-instance tests (a bound is usually hit)."""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((d, n)) / np.sqrt(d)
    C = rng.standard_normal((q, n))
    A = rng.standard_normal((mA, n))
    fix = np.zeros(n, dtype=bool)
    fix[rng.choice(n, nfix, replace=False)] = True
    bound = 1e3 if wide else 1.0
    cons_o = R.make_mixed_constraints(A, R.chol_lower(A @ A.T), fix if nfix else None, l=-bound * np.ones(n), u=bound * np.ones(n))
    x_minor = np.clip(0.3 * rng.standard_normal(n), -0.9, 0.9)
    x_minor[fix] = bound
    g = J.T @ rng.standard_normal(d)
    w_l, w_u = R.build_step_bounds(x_minor, cons_o, (1e3 if wide else 0.1) * np.linalg.norm(g))
    return J, C, A, fix, cons_o, g, w_l, w_u


def _check_against_oracle_and_option_off(bh, J, C, A, fix, cons_o, g, w_l, w_u, kappa2, mu, detail, min_iters=1):
    n, mA = g.shape[0], A.shape[0]
    Ho = R.AlHessian(J, C, mu)
    w_g, s_g, it_g = R.projected_cg(g, Ho, w_l, w_u, cons_o, kappa2, hmul_fn=hmul_gram)
    assert it_g - 1 >= min_iters, (detail, it_g)
    tol = w_tolerance(g, Ho, w_l, w_u, cons_o, kappa2, w_g)
    H = _gram(bh, J, C, mu)
    cons = bh.MixedConstraints(A, cons_o.chol_L, fix)
    out = {}
    for opt in (0, 1, 1):                                          # the second fused call starts from the first one's iteration count
        bh.set_option("gram_cg_fused", opt)
        try:
            w, status, info = bh.projected_cg(g, H, w_l, w_u, cons, kappa2, full_output=True)
        finally:
            bh.set_option("gram_cg_fused", 0)
        assert H.stats()["cg_kernels"] == (expected_kernels(n, mA, int(fix.sum())) if opt else 0), (detail, opt, H.stats()["cg_kernels"])
        assert int(status) == int(s_g), (detail, opt, status, s_g)
        if info["iters"] != it_g:
            assert_iters_in_oracle_band(info["iters"], gram_band(g, Ho, w_l, w_u, cons_o, kappa2), "Gram fused CG: iterations vs oracle band",
                                        "%s option %d" % (detail, opt))
        assert_w_close(w, w_g, tol, "Gram fused CG: w vs the oracle's Gram form" if opt else "Gram form: projected_cg w vs the oracle's Gram form", detail)
        if mA:
            assert np.linalg.norm(A @ w) <= 1e-9 * np.linalg.norm(A) * np.linalg.norm(w), (detail, opt)
        assert np.all(w[fix] == 0.0), (detail, opt)
        if opt and opt in out:
            assert np.array_equal(w, out[opt][0]) and info["iters"] == out[opt][1], detail       # deterministic, whatever the launch schedule
        out[opt] = (w, info["iters"])
    assert H.gram_builds == 1
    H.close()
    cons.close()


# n = 2050: ld = 2064, R = 4 -> 516 row groups over a 256-workgroup grid (3 and 2 passes, the last group short); n = 4099: odd, geometry 5,
# 8-9 passes; n = 8200: geometry 6 (one row per step, v and p in two halves), d = 64 keeps the oracle's long-double run to seconds.
@pytest.mark.parametrize("d,n,q,nfix,kappa2,wide", [(300, 100, 0, 7, 1e-3, True), (600, 500, 1, 40, 0.1, False), (400, 1000, 0, 64, 1e-3, True),
                                                    (300, 2000, 1, 100, 0.1, True), (256, 2050, 0, 33, 1e-3, True), (128, 4099, 1, 200, 1e-3, True),
                                                    (64, 8200, 0, 100, 1e-3, True)])
def test_box_shapes_per_geometry(bh, d, n, q, nfix, kappa2, wide):
    J, C, A, fix, cons_o, g, w_l, w_u = _instance(d, n, q, 0, nfix, 100 + n, wide)
    _check_against_oracle_and_option_off(bh, J, C, A, fix, cons_o, g, w_l, w_u, kappa2, 10.0, "box d=%d n=%d q=%d" % (d, n, q),
                                         min_iters=3 if wide else 1)


@pytest.mark.parametrize("n,mA", [(300, 1), (300, 3), (300, 8), (300, 64), (2050, 1), (2050, 3), (2050, 8), (2050, 64), (300, 65)])
def test_equality_shapes(bh, n, mA):
    """mA = 1: no refinement behind the explicit inverse; 64: the full tile; 65: one row too many — the separate-kernel shape."""
    d, q = (600, 1) if n == 300 else (256, 0)
    J, C, A, fix, cons_o, g, w_l, w_u = _instance(d, n, q, mA, n // 12, 200 + n + mA, mA % 2 == 1)
    _check_against_oracle_and_option_off(bh, J, C, A, fix, cons_o, g, w_l, w_u, 0.1 if mA == 8 else 1e-3, 10.0, "equalities n=%d mA=%d q=%d" % (n, mA, q))


# ------------------------------------------------------------------------------------------------------ launch-ahead and repeat
def _ic_instance(bh, d, n, seed):
    syn = bh.synthetic
    k = np.arange(d)[:, None] + np.arange(n)[None, :] * d
    J = syn.splitmix_uniform(seed, k) / np.sqrt(d) * syn.column_scale(n, 1)[None, :]
    x, x_l, x_u, fix = syn.box_vectors(n, fix_every=8)
    return J, x, x_l, x_u, fix


def test_launch_ahead_across_differing_calls(fused):
    """Six subproblems on ONE handle in rotation, twice: consecutive calls differ in their iteration counts, so the first batch (sized by
    the previous call) is wrong every time — too long (gated launches past the exit) or too short (the progress word decides).  Every
    call must return bit for bit what a fresh handle returns for it."""
    bh = fused
    syn = bh.synthetic
    d, n = 2048, 300
    J, x, x_l, x_u, fix = _ic_instance(bh, d, n, 1)
    rng = np.random.default_rng(5)
    gs = [J.T @ syn.residual_rows(0, d), J.T @ rng.standard_normal(d), rng.standard_normal(n)]
    subs = [(gs[i % 3], (0.1, 1e-3)[i % 2]) for i in range(6)]
    cons = bh.MixedConstraints(np.zeros((0, n)), None, fix, l=x_l, u=x_u)
    bounds = [syn.step_bounds(x, x_l, x_u, fix, syn.initial_tr(g)) for g, _ in subs]
    fresh = []
    for (g, kappa2), (w_l, w_u) in zip(subs, bounds):
        Hf = _gram(bh, J, None, 10.0)
        w, st, info = bh.projected_cg(g, Hf, w_l, w_u, cons, kappa2, full_output=True)
        assert Hf.stats()["cg_kernels"] == 2
        fresh.append((w, int(st), info["iters"], info["n_hmul"]))
        Hf.close()
    assert len({f[3] for f in fresh}) >= 3, [f[3] for f in fresh]
    H = _gram(bh, J, None, 10.0)
    prev = None
    for rnd in range(2):
        for k, ((g, kappa2), (w_l, w_u)) in enumerate(zip(subs, bounds)):
            w, st, info = bh.projected_cg(g, H, w_l, w_u, cons, kappa2, full_output=True)
            assert (int(st), info["iters"], info["n_hmul"]) == fresh[k][1:], (rnd, k, int(st), info, fresh[k][1:])
            assert np.array_equal(w, fresh[k][0]), (rnd, k)
            assert prev != info["n_hmul"], (rnd, k, prev)           # the prediction from the previous call was wrong
            prev = info["n_hmul"]
    assert H.gram_builds == 1
    H.close()
    cons.close()


def test_repeated_subproblem_is_bit_identical(fused):
    bh = fused
    J, C, A, fix, cons_o, g, w_l, w_u = _instance(256, 2050, 0, 3, 100, 77, True)
    H = _gram(bh, J, C, 10.0)
    cons = bh.MixedConstraints(A, cons_o.chol_L, fix)
    runs = [bh.projected_cg(g, H, w_l, w_u, cons, 1e-3, full_output=True) for _ in range(5)]
    assert H.stats()["cg_kernels"] == 3 and runs[0][2]["n_hmul"] >= 3
    for w, st, info in runs[1:]:
        assert np.array_equal(w, runs[0][0]) and int(st) == int(runs[0][1]) and info["n_hmul"] == runs[0][2]["n_hmul"]
    H.close()
    cons.close()


# --------------------------------------------------------------------------------------------------------------------- callers
@pytest.mark.parametrize("d,n,q,mA,nfix,seed", [(300, 128, 0, 0, 0, 4), (1500, 700, 2, 0, 90, 3), (200, 65, 0, 3, 9, 2), (600, 2050, 1, 8, 60, 5)])
def test_minor_iterate_and_accumulated_hw(bh, d, n, q, mA, nfix, seed):
    """bh_minor_iterate on a Gram handle, option 1 against option 0: same status, step within the CG tolerance of the oracle; and the
    H*w the fused loop accumulates next to w (consumed by bh_step_accumulate_dev without another product) against a fresh H*w."""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((d, n)) / np.sqrt(d)
    C = rng.standard_normal((q, n))
    A = rng.standard_normal((mA, n))
    fix = np.zeros(n, dtype=bool)
    fix[rng.choice(n, nfix, replace=False)] = True
    xlow, xupp = -np.ones(n), np.ones(n)
    cons_o = R.make_mixed_constraints(A, R.chol_lower(A @ A.T), fix if nfix else None, l=xlow, u=xupp)
    x = np.clip(0.4 * rng.standard_normal(n), -0.9, 0.9)
    x[fix] = 1.0
    s = np.zeros(n)
    Ho = R.AlHessian(J, C, 10.0)
    gm = J.T @ rng.standard_normal(d)
    delta = 0.3 * np.linalg.norm(gm)
    wl2, wu2 = R.build_step_bounds(x + s, cons_o, delta)
    w_cg, s_cg, it_cg = R.projected_cg(gm, Ho, wl2, wu2, cons_o, 0.1, hmul_fn=hmul_gram)
    tol = w_tolerance(gm, Ho, wl2, wu2, cons_o, 0.1, w_cg)
    H = _gram(bh, J, C, 10.0)
    cons = bh.MixedConstraints(A, cons_o.chol_L, fix, l=xlow, u=xupp)
    lib = bh._lib.lib()
    res = {}
    for opt in (0, 1):
        bh.set_option("gram_cg_fused", opt)
        try:
            res[opt] = bh.minor_iterate(x, s, gm, H, cons, delta, 0.1, full_output=True)
            assert H.stats()["cg_kernels"] == (expected_kernels(n, mA, nfix) if opt else 0)
        finally:
            bh.set_option("gram_cg_fused", 0)
    (w0, st0, info0), (w1, st1, info1) = res[0], res[1]
    assert int(st1) == int(st0) == int(s_cg)
    assert_w_close(w1, w0, tol, "Gram fused CG: minor_iterate step vs option 0", "d=%d n=%d mA=%d" % (d, n, mA))
    # the device-pointer chain: minor iterate, then g_minor += H*w from what the loop accumulated (no product: asserted on the counter)
    G = gram_dense(Ho)
    bh.set_option("gram_cg_fused", 1)
    bh.set_option("step_from_cg", 1)
    try:
        dv = {k: bh.DeviceVector(n, v) for k, v in (("x", x), ("s", s), ("g", gm), ("gm", gm), ("xl", xlow), ("xu", xupp))}
        dv["w"] = bh.DeviceVector(n)
        st, it, nh, al = ct.c_int32(), ct.c_int32(), ct.c_int32(), ct.c_double()
        bh._lib.check(lib.bh_minor_iterate_dev(H.handle, cons.handle, dv["x"].ptr, dv["s"].ptr, dv["gm"].ptr, dv["xl"].ptr, dv["xu"].ptr, delta, 0.1,
                                               bh.operators.SQRT_EPS, 1e-10, dv["w"].ptr, ct.byref(st), ct.byref(it), ct.byref(nh), ct.byref(al)), "minor")
        assert H.stats()["cg_kernels"] == expected_kernels(n, mA, nfix)
        w = dv["w"].download()
        n0 = H.stats()["n_hmul"]
        bh._lib.check(lib.bh_step_accumulate_dev(H.handle, dv["s"].ptr, dv["w"].ptr, dv["g"].ptr, dv["gm"].ptr), "step")
        assert H.stats()["n_hmul"] == n0
        gm1 = dv["gm"].download()
    finally:
        bh.set_option("step_from_cg", 0)
        bh.set_option("gram_cg_fused", 0)
    assert np.array_equal(w, w1)
    fresh = H * w
    bar = float(np.linalg.norm(np.abs(G) @ np.abs(w)))
    note_tol("Gram fused CG: accumulated H*w vs a fresh product (1e-12 of |G||w|)", np.linalg.norm(gm1 - (gm + fresh)), TOL1 * bar, "d=%d n=%d mA=%d" % (d, n, mA))
    assert np.linalg.norm(gm1 - (gm + fresh)) <= TOL1 * bar
    for v in dv.values():
        v.close()
    H.close()
    cons.close()


# --------------------------------------------------------------------------------------------------- ill-conditioned, long run
def test_ill_conditioned_long_run(fused):
    """The `ic` instance of test_pcg_ill_conditioned_synthetic_gram_form (8192 x 512, columns scaled 10^(-3j/n), more than 10 iterations)."""
    bh = fused
    syn = bh.synthetic
    d, n = 8192, 512
    J, x, x_l, x_u, fix = _ic_instance(bh, d, n, 1)
    g = J.T @ syn.residual_rows(0, d)
    w_l, w_u = syn.step_bounds(x, x_l, x_u, fix, syn.initial_tr(g))
    Ho = R.AlHessian(J, np.zeros((0, n)), 10.0)
    cons_o = R.make_mixed_constraints(np.zeros((0, n)), R.chol_lower(np.zeros((0, 0))), fix, l=x_l, u=x_u)
    w_ref, s_ref, it_ref = R.projected_cg(g, Ho, w_l, w_u, cons_o, 0.1)
    assert it_ref > 10
    H = _gram(bh, J, None, 10.0)
    cons = bh.MixedConstraints(np.zeros((0, n)), None, fix, l=x_l, u=x_u)
    w, status, info = bh.projected_cg(g, H, w_l, w_u, cons, 0.1, full_output=True)
    assert H.stats()["cg_kernels"] == 2
    assert int(status) == int(s_ref)
    assert_iters_in_oracle_band(info["iters"], gram_band(g, Ho, w_l, w_u, cons_o, 0.1), "Gram fused CG: iterations vs oracle band", "ic d=8192 n=512")
    w_g, s_g, it_g = R.projected_cg(g, Ho, w_l, w_u, cons_o, 0.1, hmul_fn=hmul_gram)
    assert_w_close(w, w_g, w_tolerance(g, Ho, w_l, w_u, cons_o, 0.1, w_g), "Gram fused CG: w vs the oracle's Gram form", "ic d=8192 n=512")
    H.close()
    cons.close()
