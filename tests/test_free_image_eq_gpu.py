"""The three-kernel equality CG loop on the compact image of the free columns (option free_image_eq), on the device.

The differential.  For every call of the runs of tests/free_image_eq_cases.py (active sets pushed to ONE Hessian handle under
free_image = 2 and free_image_eq = 1, with 1 .. 64 linear equalities whose matrix holds small integers) projected_cg runs on the
run's handle, and then on a FRESH pair of handles built from the explicitly compacted problem J[:, map], C[:, map], A[:, map], g[map],
bounds gathered likewise, nothing fixed, both options off.  The two loops run the same kernels with the same geometry and chunk
ownership (the chunk count of the live width picks the row-stream geometry, the update grid, the projection grid and the number of
r.v partials; max_iter = 2 (w - mA) on both sides); the Gram matrix of A_free is an exact integer matrix in any order, so factor,
explicit inverse and refinement operand are the same bits; only row strides and addresses differ.  So status,
iters, n_hmul, every trace row and w are demanded EQUAL AS uint64.  The reference of this comparison is the library's own full-image
equality loop, held to the oracle in tests/test_parity_gpu.py and tests/test_proj_exact_gpu.py and anchored here: the first and the
last call of every run are also held against the oracle under w_tolerance, and one whole iteration against exact dyadic numbers.

Every test sets the option through bh.set_option("free_image_eq", 1): without the feature that call is refused.
"""
import ctypes as ct

import numpy as np
import pytest

import benlsip_ref as R
import free_image_cases as F
import free_image_eq_cases as E
import proj_cases as pc
from _util import assert_w_close, relnorm, w_tolerance
from test_free_image_exact_gpu import TOL_LABEL, _assert_pair, _pcg_dev, _pcg_host
from test_free_image_gpu import _assert_image, _bits

pytestmark = pytest.mark.gpu

OPTION_DEFAULTS = {"blocks_per_cu": 0, "free_image": 1, "free_image_eq": 0, "cg_fused": 1, "proj_form": 1, "profile": 0, "profile_stride": 8}


@pytest.fixture(scope="module")
def n_cu(bh):
    n = ct.c_int32(0)
    bh._lib.check(bh._lib.lib().bh_device_info(None, 0, ct.byref(n), None, 0), "bh_device_info")
    bh.set_option("blocks_per_cu", 1)
    try:
        yield int(n.value)
    finally:
        for k, v in OPTION_DEFAULTS.items():
            bh.set_option(k, v)


@pytest.fixture
def compact_eq(bh, n_cu):
    """free_image = 2 and free_image_eq = 1 for one test; both back at their defaults afterwards."""
    bh.set_option("free_image", 2)
    bh.set_option("free_image_eq", 1)
    try:
        yield
    finally:
        for k, v in OPTION_DEFAULTS.items():
            if k != "blocks_per_cu":
                bh.set_option(k, v)


def _compact_run(bh, Jfull, A, m, g, w_l, w_u, kappa2=F.KAPPA2):
    """The ordinary full-image equality loop on the explicitly compacted problem (fresh handles, both options off)."""
    d = Jfull.shape[0] - F.Q
    Hc = bh.AlHessian(np.ascontiguousarray(Jfull[:d, m]), np.ascontiguousarray(Jfull[d:, m]), F.MU)
    cc = bh.MixedConstraints(np.ascontiguousarray(A[:, m]), None, None)
    try:
        bh.set_option("free_image", 0)
        bh.set_option("free_image_eq", 0)
        outs = [_pcg_host(bh, Hc, cc, g_[m], l_[m], u_[m], kappa2) for g_, l_, u_ in zip(g, w_l, w_u)]
        assert Hc.free_image_info(cc)["builds"] == 0 and Hc.stats()["cg_kernels"] == 3
        return outs
    finally:
        bh.set_option("free_image", 2)
        bh.set_option("free_image_eq", 1)
        Hc.close()
        cc.close()


@pytest.mark.parametrize("run", list(E.RUNS))
def test_equality_cg_on_the_compact_image_equals_the_compacted_problem_bit_for_bit(bh, n_cu, compact_eq, run):
    I = E.instance(run, n_cu)
    n, g = I["n"], I["g"]
    cs = E.calls(run)
    Jfull = np.vstack([I["J"], I["C"]])
    assert Jfull.shape[0] == F.rows_for(E.RUNS[run][0], n_cu)
    anchors = {0, len(cs) - 1}
    pcg = _pcg_dev if n % 16 == 0 else _pcg_host
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    cons = {}
    served = 0
    try:
        for i, c in enumerate(cs):
            what = "%s call %d (%s, width %d, stride %d, %s %d)" % (run, i, c.who, c.width, c.ldf, c.action, c.moved)
            A = E.lineq(run, c.who)
            if c.who not in cons:
                cons[c.who] = bh.MixedConstraints(A, None, c.fix.copy())
            elif i > 0 and cs[i - 1].who == c.who and np.array_equal(cs[i - 1].fix, c.fix):
                arr = cons[c.who].fixvars                         # the same array written again and pushed again
                arr[:] = c.fix
                cons[c.who].mark_dirty()
            elif not np.array_equal(cons[c.who].fixvars, c.fix):
                cons[c.who].fixvars = c.fix.copy()
            P = cons[c.who]
            cells = [E.cell(run, n_cu, i, s, band=i in anchors) for s in ("wide", "box")]
            got = []
            for cl in cells:
                got.append(pcg(bh, H, P, g, cl["w_l"], cl["w_u"]))
                served += 1
                assert H.stats()["cg_kernels"] == 3, what
                if cl is cells[0]:
                    info, mp = _assert_image(H, P, Jfull, c.fix, builds=c.builds, moves=c.moves)
                    assert np.array_equal(mp, c.map), (what, "the device map is not the mirror's")
                else:
                    info = H.free_image_info(P)
                    assert (info["state"], info["width"], info["builds"], info["moves"]) == ("valid", c.width, c.builds, c.moves), (what, info)
                assert info["calls_served"] == served, (what, info)
            m = c.map[:c.width].astype(np.int64)
            ref = _compact_run(bh, Jfull, A, m, [g, g], [cl["w_l"] for cl in cells], [cl["w_u"] for cl in cells])
            for cl, a, b, setting in zip(cells, got, ref, ("wide", "box")):
                _assert_pair(a, b, m, c.fix, what + " " + setting)
                assert a[1] == (int(R.CGStatus.solved) if setting == "wide" else int(R.CGStatus.bound_hit)), (what, setting, a[1:4])
                if i in anchors:
                    assert set(cl["band"].values()) == {(cl["status"], cl["iters"])}, (
                        "the ORACLE, on this machine's BLAS, does not decide its own iteration count (no device result is involved)", cl["band"])
                    assert a[1:4] == (cl["status"], cl["iters"], cl["n_hmul"]), (what, setting, a[1:4], (cl["status"], cl["iters"], cl["n_hmul"]))
                    tol = w_tolerance(g, I["Ho"], cl["w_l"], cl["w_u"], cl["cons_o"], F.KAPPA2, cl["w"])
                    print("[%s %s] ||w - w_oracle|| / ||w_oracle|| = %.3e (tolerance %.3e), %d products" % (what, setting, relnorm(a[0], cl["w"]), tol, a[3]))
                    assert_w_close(a[0], cl["w"], tol, TOL_LABEL, what + " " + setting)
    finally:
        H.close()
        for P in cons.values():
            P.close()


# ------------------------------------------------------------------------------------------ one exact iteration, dyadic ground truth
def test_one_exact_iteration_with_equalities_on_the_compact_image(bh, n_cu, compact_eq):
    """J'J = 16 I on any set of columns, A_free = T Q (proj_cases.py) on each of three nested free sets, integer g: v = P(g) is dyadic,
    p'Hp = 16 |v|^2, alpha = 1/16, the second projection vanishes: solved after one product with w = -P(g) / 16 in every bit and
    A w == 0 exactly.  After a build, after a move to a width = 0 mod 16, and at the smallest width the cap nfree > mA keeps."""
    cases = E.exact_cases()
    n = E.EXACT_N
    Jfull = pc.cg_jacobian(n)
    H = bh.AlHessian(Jfull, None, 1.0)
    inf = np.full(n, np.inf)
    moves = 0
    try:
        for k, c in enumerate(cases):
            gk = c.r                                              # integer, large on the fixed variables (they must not be seen)
            P = bh.MixedConstraints(c.A, None, c.fix.copy())
            try:
                if k:
                    moves += int(c.fix.sum() - cases[k - 1].fix.sum())
                cons_o = R.make_mixed_constraints(c.A, R.chol_lower(c.A @ c.A.T), c.fix)
                tr = R.CGTrace()
                _, st_o, it_o = R.projected_cg(gk, R.AlHessian(Jfull, np.zeros((0, n)), 1.0), -inf, inf, cons_o, 0.1, trace=tr)
                assert tr.n_hmul == 1 and int(st_o) == int(R.CGStatus.solved)
                w, status, iters, n_hmul, trace = _pcg_host(bh, H, P, gk, -inf, inf, 0.1)
                _assert_image(H, P, Jfull, c.fix, builds=1, moves=moves)
                assert H.free_image_info(P)["calls_served"] == k + 1 and H.stats()["cg_kernels"] == 3
                assert (status, iters, n_hmul) == (int(st_o), int(it_o), 1), (k, status, iters, n_hmul)
                vv = float(c.v @ c.v)
                want = np.array([pc.CG_C * vv, 1.0 / pc.CG_C, 0.0])
                assert np.array_equal(_bits(trace[0][[0, 1, 3]]), _bits(want)), (k, trace[0], want)
                assert trace[0][2] == tr.rows[0][2] or (np.isinf(trace[0][2]) and np.isinf(tr.rows[0][2]))
                w_exact = 0.0 - c.v / pc.CG_C
                bad = np.flatnonzero(_bits(w) != _bits(w_exact))
                assert bad.size == 0, (k, "w differs from -P(g)/16 at", bad[:8], w[bad[:8]], w_exact[bad[:8]])
                assert not (c.A @ w).any() and not _bits(w[c.fix]).any()
            finally:
                P.close()
    finally:
        H.close()


# ---------------------------------------------------------------------------------------------------------------------- structure
def test_reporting_and_the_option_at_zero_on_the_same_handle(bh, n_cu, compact_eq):
    """free_image_info and stats.bytes_per_hmul show the compact bytes, stats.cg_kernels == 3, bh_time_kernel kind 0 runs on the compact
    image; with the option back at 0 on the SAME handle the same call reports the full bytes and gives the bits of a handle pair that
    never saw the option."""
    run, i = "S1_m64", 0
    I, c = E.instance(run, n_cu), E.calls(run)[i]
    n, g, A = I["n"], I["g"], E.lineq(run, c.who)
    cl = E.cell(run, n_cu, i, "wide", band=False)
    rows = I["d"] + F.Q
    full_bytes = 8.0 * rows * n + 16.0 * n
    compact_bytes = 8.0 * rows * c.width + 16.0 * c.width
    bh.set_option("free_image_eq", 0)
    bh.set_option("free_image", 1)
    H0 = bh.AlHessian(I["J"], I["C"], F.MU)
    P0 = bh.MixedConstraints(A, None, c.fix.copy())
    try:
        never = _pcg_host(bh, H0, P0, g, cl["w_l"], cl["w_u"])
        assert H0.free_image_info(P0)["builds"] == 0
    finally:
        H0.close()
        P0.close()
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = bh.MixedConstraints(A, None, c.fix.copy())
    try:
        bh.set_option("profile", 1)
        bh.set_option("profile_stride", 1)
        bh.set_option("free_image", 2)
        bh.set_option("free_image_eq", 1)
        H.reset_stats()
        on = _pcg_host(bh, H, P, g, cl["w_l"], cl["w_u"])
        info = H.free_image_info(P)
        st = H.stats()
        assert (info["state"], info["width"], info["builds"], info["calls_served"]) == ("valid", c.width, 1, 1), info
        assert st["cg_kernels"] == 3 and st["hmul_timed"] >= 1 and st["bytes_per_hmul"] == compact_bytes, (st["bytes_per_hmul"], compact_bytes, full_bytes)
        assert H.time_kernel(0, reps=2) > 0.0
        # the option at 0 on the same handle (the image stays where it is: a box-constrained call could still use it)
        bh.set_option("free_image_eq", 0)
        H.reset_stats()
        off = _pcg_host(bh, H, P, g, cl["w_l"], cl["w_u"])
        st = H.stats()
        assert H.free_image_info(P)["calls_served"] == 1 and st["cg_kernels"] == 3
        assert st["hmul_timed"] >= 1 and st["bytes_per_hmul"] == full_bytes, (st["bytes_per_hmul"], compact_bytes, full_bytes)
        assert off[1:4] == never[1:4] and np.array_equal(_bits(off[0]), _bits(never[0])) and np.array_equal(_bits(off[4]), _bits(never[4]))
        # both loops solve the same problem
        assert on[1:4] == off[1:4] and relnorm(on[0], off[0]) <= 1e-9
    finally:
        H.close()
        P.close()


# ----------------------------------------------------------------------------------------------------------- hand-backs and refusals
def test_non_finite_g_on_a_fixed_variable_is_handed_back(bh, n_cu, compact_eq):
    """NaN, +Inf, -Inf in g on a fixed variable: status and w bit-equal to the option off, the call is not counted as served, and the
    next finite call is served again (the projection launches of the handed-back call wrote workspace only)."""
    run, i = "S1_m2_m1", 2
    I, c = E.instance(run, n_cu), E.calls(run)[i]
    n, A = I["n"], E.lineq(run, c.who)
    cl = E.cell(run, n_cu, i, "wide", band=False)
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = bh.MixedConstraints(A, None, c.fix.copy())
    try:
        first = _pcg_host(bh, H, P, I["g"], cl["w_l"], cl["w_u"])
        assert H.free_image_info(P)["calls_served"] == 1
        for bad in (np.nan, np.inf, -np.inf):
            g = I["g"].copy()
            g[np.flatnonzero(c.fix)[3]] = bad
            out = {}
            for opt in (0, 1):
                bh.set_option("free_image_eq", opt)
                out[opt] = _pcg_host(bh, H, P, g, cl["w_l"], cl["w_u"])
            assert out[0][1:4] == out[1][1:4] and np.array_equal(_bits(out[0][0]), _bits(out[1][0])), (bad, out[0][1:4], out[1][1:4])
            assert H.free_image_info(P)["calls_served"] == 1
        again = _pcg_host(bh, H, P, I["g"], cl["w_l"], cl["w_u"])
        assert H.free_image_info(P)["calls_served"] == 2
        assert again[1:4] == first[1:4] and np.array_equal(_bits(again[0]), _bits(first[0])) and np.array_equal(_bits(again[4]), _bits(first[4]))
    finally:
        H.close()
        P.close()


REFUSALS = ("cg_fused=2", "mA=65", "proj_form=0", "gram handle", "minor_iterate with H*w")


@pytest.mark.parametrize("what", REFUSALS)
def test_calls_that_stay_on_the_full_image(bh, n_cu, compact_eq, what):
    """The four-kernel shape, mA > 64, the augmented projection form, a Gram-form handle and bh_minor_iterate with an H*w buffer
    (ls_from_cg = 1) never touch the image, and give the bits they give with the option off."""
    run, i = "S1_m64", 0
    I, c = E.instance(run, n_cu), E.calls(run)[i]
    n, g = I["n"], I["g"]
    cl = E.cell(run, n_cu, i, "wide", band=False)
    A = E.lineq(run, c.who)
    if what == "mA=65":
        A = np.vstack([A, np.random.default_rng(65).integers(-3, 4, size=(1, n)).astype(np.float64)])
    L = None
    if what == "proj_form=0":
        L = R.make_mixed_constraints(A, R.chol_lower(A @ A.T), c.fix).chol_L
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = bh.MixedConstraints(A, L, c.fix.copy(), l=-F.XB * np.ones(n), u=F.XB * np.ones(n))
    try:
        if what == "cg_fused=2":
            bh.set_option("cg_fused", 2)
        if what == "proj_form=0":
            bh.set_option("proj_form", 0)
        if what == "gram handle":
            H.set_form("gram")
        out = {}
        for opt in (1, 0):
            bh.set_option("free_image_eq", opt)
            if what == "minor_iterate with H*w":
                x = np.where(c.fix, F.XB, 0.0)
                w, status, info = bh.minor_iterate(x, np.zeros(n), g, H, P, 0.5 * float(np.max(np.abs(cl["w"]))), F.KAPPA2, full_output=True)
                out[opt] = (w, int(status), info["iters"], info["n_hmul"], np.array([info["alpha"]]))
            else:
                out[opt] = _pcg_host(bh, H, P, g, cl["w_l"], cl["w_u"])
            fi = H.free_image_info(None)
            assert (fi["builds"], fi["calls_served"]) == (0, 0), (what, opt, fi)
        assert out[1][1:4] == out[0][1:4], (what, out[1][1:4], out[0][1:4])
        assert np.array_equal(_bits(out[1][0]), _bits(out[0][0])) and np.array_equal(_bits(out[1][4]), _bits(out[0][4])), what
    finally:
        H.close()
        P.close()
