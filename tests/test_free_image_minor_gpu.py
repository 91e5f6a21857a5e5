"""bh_minor_iterate* on the compact image of the free columns (option free_image_minor), bit for bit.

With free_image_minor = 1, ls_from_cg = 1 and step_from_cg = 0 a minor iterate is considered for the compact image like a bh_pcg*: its
CG loop accumulates the FREE part of H*w in slot order (cg_reduce_update_kernel on a compact hw), and free_image_linesearch_kernel
takes the line search and the scaling on the compact operands, delivering w through the slot -> column map.

The differential is the one of tests/test_free_image_exact_gpu.py: for every state of the sequences S1..S5 of free_image_cases.py the
minor iterate runs on the sequence's handle and then on a FRESH handle built from the explicitly compacted problem, nothing fixed, both
options off.  That comparison is legitimate for the reason given there (the two loops perform the same operations in the same order)
plus one more: minor_iterate gives +-Inf step bounds to every free variable (src/basic_tralcnlss.jl:660-665), so both runs see the same
bounds, and the new kernel sums g.w and w.Hw in the order linesearch_kernel uses on n = width (slot i on thread i mod 1024, the shared
linesearch_alpha).  So status, iters, n_hmul, alpha and w[map] are demanded equal as uint64; w is +0 on the fixed variables.

The full-image minor iterate is anchored on its own (test_parity_gpu.py, test_minor_steps_exact_gpu.py) and again here: the first
state and the last state of width >= 2 of every sequence against the oracle with the assertions of
test_minor_iterate_linesearch_gradient_parity, and one iterate against integer ground truth (J'J = 16 I).
"""
import ctypes as ct
import math

import numpy as np
import pytest

import benlsip_ref as R
import free_image_cases as F
from _util import assert_w_close, relnorm, w_tolerance
from test_free_image_exact_gpu import INNER
from test_free_image_gpu import _assert_image, _bits

pytestmark = pytest.mark.gpu

DELTA = 1.0                # only the fixed variables get finite step bounds from it, and the box loop never reads those
W_LABEL = "minor_iterate: scaled w vs oracle (10 x the CG tolerance: alpha inherits w's sensitivity)"


@pytest.fixture(scope="module")
def n_cu(bh):                                  # (as the fixture of test_free_image_gpu.py, plus the option of this module)
    n = ct.c_int32(0)
    bh._lib.check(bh._lib.lib().bh_device_info(None, 0, ct.byref(n), None, 0), "bh_device_info")
    bh.set_option("blocks_per_cu", 1)
    try:
        yield int(n.value)
    finally:
        bh.set_option("blocks_per_cu", 0)
        bh.set_option("free_image", 1)
        bh.set_option("free_image_minor", 0)
        bh.set_option("ls_from_cg", 1)
        bh.set_option("step_from_cg", 0)


def _same(a, b):
    """uint64 equality of two float64 values."""
    return _bits(a).tolist() == _bits(b).tolist()


def _box(n):
    return -F.XB * np.ones(n), F.XB * np.ones(n)


def _minor_host(bh, H, P, g, kappa2=F.KAPPA2):
    """bh_minor_iterate with x = s = 0: (w, status, iters, n_hmul, alpha)."""
    n = H.n
    w, status, info = bh.minor_iterate(np.zeros(n), np.zeros(n), g, H, P, DELTA, kappa2, full_output=True)
    return w, int(status), info["iters"], info["n_hmul"], info["alpha"]


def _minor_dev(bh, H, P, g, kappa2=F.KAPPA2, s=None, keep=False):
    """bh_minor_iterate_dev on device vectors (n == ld, 16-byte aligned: g and w are used in place); w arrives pre-filled with a
    non-zero pattern.  keep: also return the device vectors (x, s, g, xlow, xupp, w) instead of closing them."""
    n = H.n
    lo, up = _box(n)
    dv = [bh.DeviceVector(n, v) for v in (np.zeros(n), np.zeros(n) if s is None else s, g, lo, up, np.full(n, 7.25))]
    try:
        P._sync()
        status, iters, n_hmul, alpha = ct.c_int32(-1), ct.c_int32(0), ct.c_int32(0), ct.c_double(0.0)
        bh._lib.check(bh._lib.lib().bh_minor_iterate_dev(H.handle, P.handle, dv[0].ptr, dv[1].ptr, dv[2].ptr, dv[3].ptr, dv[4].ptr, DELTA,
                                                         float(kappa2), bh.operators.SQRT_EPS, 1e-10, dv[5].ptr, ct.byref(status),
                                                         ct.byref(iters), ct.byref(n_hmul), ct.byref(alpha)), "bh_minor_iterate_dev")
        out = (dv[5].download(), status.value, iters.value, n_hmul.value, alpha.value)
        return (out, dv) if keep else out
    finally:
        if not keep:
            for v in dv:
                v.close()


def _constraints(bh, I, fix):
    lo, up = _box(I["n"])
    return bh.MixedConstraints(I["A"], None, fix, l=lo, u=up)


def _compact_run(bh, Jfull, m, g, kappa2=F.KAPPA2):
    """The ordinary minor iterate on the explicitly compacted problem (fresh handles, nothing fixed, both options off)."""
    w = m.shape[0]
    d = Jfull.shape[0] - F.Q
    lo, up = _box(w)
    Hc = bh.AlHessian(np.ascontiguousarray(Jfull[:d, m]), np.ascontiguousarray(Jfull[d:, m]), F.MU)
    cc = bh.MixedConstraints(np.zeros((0, w)), None, None, l=lo, u=up)
    try:
        bh.set_option("free_image", 0)
        bh.set_option("free_image_minor", 0)
        out = _minor_host(bh, Hc, cc, g[m], kappa2)
        assert Hc.free_image_info(cc)["builds"] == 0
        return out
    finally:
        bh.set_option("free_image", 2)
        bh.set_option("free_image_minor", 1)
        Hc.close()
        cc.close()


def _assert_pair(got, ref, m, fix, what):
    """The compact-image call `got` (on n variables) against the compacted-problem call `ref` (on the width): everything as uint64."""
    w, status, iters, n_hmul, alpha = got
    wc, status_c, iters_c, n_hmul_c, alpha_c = ref
    assert (status, iters, n_hmul) == (status_c, iters_c, n_hmul_c), (what, (status, iters, n_hmul), (status_c, iters_c, n_hmul_c))
    assert _same(alpha, alpha_c), (what, "alpha", alpha, alpha_c)
    bad = np.flatnonzero(_bits(w[m]) != _bits(wc))
    assert bad.size == 0, (what, "w differs in slots", bad[:8], w[m][bad[:8]], wc[bad[:8]])
    assert not _bits(w[fix]).any(), (what, "w is not +0 on the fixed variables", np.flatnonzero(_bits(w[fix]))[:8])


_ORACLE = {}


def _oracle(name, n_cu, k):
    """The oracle's minor iterate of state k (x = s = 0), computed once: w, status, the CG run behind it, its line search, the tolerance."""
    if (name, n_cu, k) not in _ORACLE:
        I = F.instance(name, n_cu)
        st = F.states(name)[k]
        n, g, Ho = I["n"], I["g"], I["Ho"]
        cons_o = F.oracle_constraints(I, st.fix)
        w_ref, st_ref = R.minor_iterate(np.zeros(n), np.zeros(n), g, Ho, cons_o, DELTA, F.KAPPA2)
        wl, wu = R.build_step_bounds(np.zeros(n), cons_o, DELTA)
        w_cg, s_cg, it_cg = R.projected_cg(g, Ho, wl, wu, cons_o, F.KAPPA2)
        tol = w_tolerance(g, Ho, wl, wu, cons_o, F.KAPPA2, w_cg)
        a_cg = R.linesearch(g, Ho, w_cg, wl, wu, cons_o.fixvars)
        _ORACLE[(name, n_cu, k)] = dict(w=w_ref, status=int(st_ref), iters=int(it_cg), tol=tol, alpha=a_cg)
    return _ORACLE[(name, n_cu, k)]


# --------------------------------------------------------------------------------- 1. the compacted problem, 2. the anchors
@pytest.mark.parametrize("name", list(F.SEQS))
def test_minor_iterate_on_the_compact_image_equals_the_compacted_problem_bit_for_bit(bh, n_cu, name):
    I = F.instance(name, n_cu)
    g = I["g"]
    sts = F.states(name)
    Jfull = np.vstack([I["J"], I["C"]])
    assert Jfull.shape[0] == F.rows_for(name, n_cu)
    anchors = {0, max(k for k, s in enumerate(sts) if s.width >= 2)}
    run = _minor_dev if name == "S3" else _minor_host
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    cons = {}
    served = 0
    try:
        bh.set_option("free_image", 2)
        bh.set_option("free_image_minor", 1)              # (this call fails where the option does not exist)
        for k, st in enumerate(sts):
            what = "%s state %d (width %d, stride %d, %s %d)" % (name, k, st.width, st.ldf, st.action, st.k)
            if st.who not in cons:
                cons[st.who] = _constraints(bh, I, st.fix.copy())
            elif k > 0 and sts[k - 1].who == st.who and np.array_equal(sts[k - 1].fix, st.fix):
                arr = cons[st.who].fixvars                        # the same array written again and pushed again
                arr[:] = st.fix
                cons[st.who].mark_dirty()
            elif not np.array_equal(cons[st.who].fixvars, st.fix):
                cons[st.who].fixvars = st.fix.copy()             # (S4: a handle whose turn comes again still holds its set)
            P = cons[st.who]
            got = run(bh, H, P, g)
            served += 1
            info, mp = _assert_image(H, P, Jfull, st.fix, builds=st.builds, moves=st.moves)      # the action this call took
            assert np.array_equal(mp, st.map), (what, "the device map is not the mirror's")
            assert info["calls_served"] == served, (what, info)
            m = st.map[:st.width].astype(np.int64)
            ref = _compact_run(bh, Jfull, m, g)
            _assert_pair(got, ref, m, st.fix, what)
            assert got[1] == int(R.CGStatus.solved), (what, got[1:])
            if k in anchors:
                o = _oracle(name, n_cu, k)
                assert (got[1], got[2]) == (o["status"], o["iters"]), (what, got[1:4], o["status"], o["iters"])
                print("[%s] ||w - w_oracle|| / ||w_oracle|| = %.3e (tolerance %.3e), alpha %r (oracle %r), %d products" % (
                    what, relnorm(got[0], o["w"]), 10 * o["tol"], got[4], o["alpha"], got[3]))
                assert_w_close(got[0], o["w"], 10 * o["tol"], W_LABEL, what)
                assert got[4] == pytest.approx(o["alpha"], rel=max(1e-6, 1e3 * o["tol"])), (what, got[4], o["alpha"], o["tol"])
    finally:
        bh.set_option("free_image", 1)
        bh.set_option("free_image_minor", 0)
        H.close()
        for P in cons.values():
            P.close()


# ----------------------------------------------------------------------------------------------------- 3. integer ground truth
def test_one_exact_minor_iterate_on_the_compact_image(bh, n_cu):
    """J = four stacked 2 I (J'J = 16 I), C = 0, integer g: p_1 = -mask(g), p'Hp = 16 |g_f|^2, the CG step 1/16, r = 0 after one product;
    H*w = -mask(g), g.w = -|g_f|^2 / 16 = -w'Hw, so the line search gives alpha = 1 and w = -mask(g) / 16 — all exact in any order.
    After a build (width 1030, six slots past the line search's 1024 threads), after a move to a multiple of 16, and at width 1."""
    n = 1100
    rng = np.random.default_rng(F.EXACT_SEED)
    order = rng.permutation(n)
    g = rng.integers(1, 8, n).astype(np.float64) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    J = np.vstack([2.0 * np.eye(n)] * 4)
    H = bh.AlHessian(J, None, F.MU)
    P = None
    try:
        bh.set_option("free_image", 2)
        bh.set_option("free_image_minor", 1)
        moves = 0
        widths = (1030, 1024, 1)
        for k, width in enumerate(widths):
            fix = np.ones(n, dtype=bool)
            fix[order[:width]] = False
            if P is None:
                lo, up = _box(n)
                P = bh.MixedConstraints(np.zeros((0, n)), None, fix.copy(), l=lo, u=up)
            else:
                moves += widths[k - 1] - width
                P.fixvars = fix.copy()
            w, status, iters, n_hmul, alpha = _minor_host(bh, H, P, g)
            _assert_image(H, P, J, fix, builds=1, moves=moves)
            assert (status, iters, n_hmul) == (int(R.CGStatus.solved), 2, 1), (width, status, iters, n_hmul)
            assert _same(alpha, 1.0), (width, alpha)
            assert np.array_equal(_bits(w), _bits(np.where(fix, 0.0, -g / 16.0) + 0.0)), width
        assert H.free_image_info(P)["calls_served"] == len(widths)
    finally:
        bh.set_option("free_image", 1)
        bh.set_option("free_image_minor", 0)
        H.close()
        if P is not None:
            P.close()


# ------------------------------------------------------------------------------------------------- 4. reroute, 5. no curvature
def test_a_nonfinite_g_on_a_fixed_variable_is_handed_back_to_the_full_image(bh, n_cu):
    """The gather finds the NaN and hands the call back (kCgReroute): the loop, the line search and the scaling are today's, on the full
    vectors with the full H*w.  Status, alpha and every bit of w as with free_image_minor = 0; the call is not counted as served."""
    I = F.instance("S1", n_cu)
    st = F.states("S1")[3]
    g = I["g"].copy()
    g[np.flatnonzero(st.fix)[5]] = np.nan
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = _constraints(bh, I, st.fix.copy())
    try:
        bh.set_option("free_image", 2)
        bh.set_option("free_image_minor", 1)
        _minor_host(bh, H, P, I["g"])                                 # builds the image
        before = H.free_image_info(P)
        assert before["builds"] == 1 and before["calls_served"] == 1
        got = _minor_host(bh, H, P, g)
        assert H.free_image_info(P) == before
        bh.set_option("free_image_minor", 0)
        ref = _minor_host(bh, H, P, g)
        assert H.free_image_info(P) == before
        assert got[1:4] == ref[1:4], (got[1:], ref[1:])
        assert _same(got[4], ref[4]), (got[4], ref[4])
        assert np.array_equal(_bits(got[0]), _bits(ref[0]))
    finally:
        bh.set_option("free_image", 1)
        bh.set_option("free_image_minor", 0)
        H.close()
        P.close()


def test_no_curvature_along_the_first_direction(bh, n_cu):
    """J and C are zero in every free column on which g is non-zero: p_1'Hp_1 = 0, negative curvature, no line search (:669): alpha
    comes back NaN and w is the CG loop's, +0 everywhere, as on the compacted problem."""
    I = F.instance("S1", n_cu)
    st = F.states("S1")[3]
    n = I["n"]
    on = np.flatnonzero(~st.fix)[::3]
    Jfull = np.vstack([I["J"], I["C"]]).copy()
    Jfull[:, on] = 0.0
    g = np.zeros(n)
    g[on] = I["g"][on]
    g[st.fix] = I["g"][st.fix]                                   # (the fixed entries of g are the mask's business)
    d = Jfull.shape[0] - F.Q
    H = bh.AlHessian(np.ascontiguousarray(Jfull[:d]), np.ascontiguousarray(Jfull[d:]), F.MU)
    P = _constraints(bh, I, st.fix.copy())
    try:
        bh.set_option("free_image", 2)
        bh.set_option("free_image_minor", 1)
        got = _minor_host(bh, H, P, g)
        info, mp = _assert_image(H, P, Jfull, st.fix, builds=1, moves=0)
        assert info["calls_served"] == 1
        m = mp[:st.width].astype(np.int64)
        ref = _compact_run(bh, Jfull, m, g)
        assert got[1:4] == ref[1:4] == (int(R.CGStatus.negative_curvature), 1, 1), (got[1:4], ref[1:4])
        assert math.isnan(got[4]) and math.isnan(ref[4])
        assert np.array_equal(_bits(got[0][m]), _bits(ref[0])) and not _bits(got[0]).any()
    finally:
        bh.set_option("free_image", 1)
        bh.set_option("free_image_minor", 0)
        H.close()
        P.close()


# ------------------------------------------------------------------------------------------------------------ 6. step_from_cg
def test_step_from_cg_keeps_the_call_on_the_full_image(bh, n_cu):
    """With step_from_cg = 1 bh_step_accumulate_dev may add the accumulated H*w, fixed part included: the call is not considered."""
    I = F.instance("S1", n_cu)
    st = F.states("S1")[3]
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = _constraints(bh, I, st.fix.copy())
    try:
        bh.set_option("free_image", 2)
        bh.set_option("free_image_minor", 1)
        bh.set_option("step_from_cg", 1)
        full = _minor_host(bh, H, P, I["g"])
        assert H.free_image_info(None)["builds"] == 0 and H.free_image_info(None)["calls_served"] == 0
        bh.set_option("step_from_cg", 0)
        got = _minor_host(bh, H, P, I["g"])
        assert H.free_image_info(P)["calls_served"] == 1
        assert got[1:3] == full[1:3]
    finally:
        bh.set_option("step_from_cg", 0)
        bh.set_option("free_image", 1)
        bh.set_option("free_image_minor", 0)
        H.close()
        P.close()


def test_inner_step_is_untouched_by_the_option(bh, n_cu):
    """bh.inner_step switches step_from_cg on around its minor loop: s, the model reduction and the log of the minor iterates have the
    same bits with free_image_minor 0 and 1, and under 1 no minor iterate was served from the image."""
    d, n = INNER["d"], INNER["n"]
    J = R.synthetic_J(d, n, seed=INNER["seed"])
    inst = R.synthetic_box_vectors(d, n, fix_every=8)
    A = np.zeros((0, n))
    g = J.T @ inst.r0
    delta = R.initial_tr(g)
    out = {}
    try:
        bh.set_option("free_image", 2)
        for opt in (0, 1):
            bh.set_option("free_image_minor", opt)
            H = bh.AlHessian(J, None, 10.0)
            P = bh.MixedConstraints(A, None, None, l=inst.x_l, u=inst.x_u)
            try:
                s, pred, info = bh.inner_step(inst.x, g, H, P, delta, INNER["minor_steps"], INNER["kappa2"], INNER["kappa3"], full_output=True)
                out[opt] = (s, pred, [(int(a), int(b), int(c), float(e)) for a, b, c, e in info["minor"]], H.free_image_info(None))
            finally:
                H.close()
                P.close()
        assert len(out[0][2]) == INNER["minor_steps"]
        assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and _same(out[0][1], out[1][1])
        assert [m[:3] for m in out[0][2]] == [m[:3] for m in out[1][2]]
        assert _bits([m[3] for m in out[0][2]]).tolist() == _bits([m[3] for m in out[1][2]]).tolist()
        assert out[0][3] == out[1][3] and out[1][3]["calls_served"] == 0, (out[0][3], out[1][3])
    finally:
        bh.set_option("free_image", 1)
        bh.set_option("free_image_minor", 0)


def test_step_accumulate_recomputes_after_a_compact_minor_iterate(bh, n_cu):
    """bh_minor_iterate_dev on the compact image leaves only the free part of H*w behind.  step_from_cg switched on AFTER it must not make
    bh_step_accumulate_dev add that: it sweeps J (one product more on the handle's counter) and gives the bits of the step_from_cg = 0
    chain on the same operands.  (Behind a full-image minor iterate the same calls do take the H*w of the CG loop: no sweep.)"""
    I = F.instance("S3", n_cu)                                      # n == ld: the device vectors are used in place
    st = F.states("S3")[0]
    n, g = I["n"], I["g"]
    lib, chk = bh._lib.lib(), bh._lib.check
    s0 = np.where(st.fix, 0.0, 0.01 * np.random.default_rng(41).standard_normal(n))
    gm0 = R.hmul(I["Ho"], s0) + g
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = _constraints(bh, I, st.fix.copy())
    out = {}
    try:
        bh.set_option("free_image", 2)
        for key, minor, late in (("chain0", 1, 0), ("compact", 1, 1), ("full", 0, 1)):
            bh.set_option("free_image_minor", minor)
            served = H.free_image_info(None)["calls_served"]
            res, dv = _minor_dev(bh, H, P, gm0, s=s0, keep=True)      # dv: x, s, g_minor, xlow, xupp, w
            dg = bh.DeviceVector(n, g)
            try:
                assert H.free_image_info(None)["calls_served"] - served == minor
                bh.set_option("step_from_cg", late)
                products = H.stats()["n_hmul"]
                chk(lib.bh_step_accumulate_dev(H.handle, dv[1].ptr, dv[5].ptr, dg.ptr, dv[2].ptr), "bh_step_accumulate_dev")
                out[key] = (res, dv[1].download(), dv[2].download(), H.stats()["n_hmul"] - products)
            finally:
                bh.set_option("step_from_cg", 0)
                dg.close()
                for v in dv:
                    v.close()
        for a, b in zip(out["compact"][0], out["chain0"][0]):
            assert np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(out["compact"][1]), _bits(out["chain0"][1]))          # s + w
        assert np.array_equal(_bits(out["compact"][2]), _bits(out["chain0"][2]))          # H (s + w) + g
        assert (out["chain0"][3], out["compact"][3], out["full"][3]) == (1, 1, 0), [o[3] for o in out.values()]
        assert relnorm(out["full"][2], out["chain0"][2]) <= 1e-10
    finally:
        bh.set_option("step_from_cg", 0)
        bh.set_option("free_image", 1)
        bh.set_option("free_image_minor", 0)
        H.close()
        P.close()


# ---------------------------------------------------------------------------------------------------------- 7. option hygiene
def test_option_values_default_and_repeatability(bh, n_cu):
    lib = bh._lib.lib()
    I = F.instance("S1", n_cu)
    st = F.states("S1")[3]
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = _constraints(bh, I, st.fix.copy())
    try:
        for bad in (2, -1):
            assert lib.bh_set_option(b"free_image_minor", bad) == bh._lib.BH_ERR_INVALID_ARG
        bh.set_option("free_image", 2)
        # the default (the module's fixture has not touched it yet if this test runs alone; every test restores 0)
        before = H.free_image_info(None)
        _minor_host(bh, H, P, I["g"])
        assert H.free_image_info(None) == before and before["builds"] == 0
        # option 1: served, and a second identical call returns the same bits
        bh.set_option("free_image_minor", 1)
        a = _minor_host(bh, H, P, I["g"])
        b = _minor_host(bh, H, P, I["g"])
        assert H.free_image_info(P)["calls_served"] == 2
        assert a[1:4] == b[1:4] and _same(a[4], b[4]) and np.array_equal(_bits(a[0]), _bits(b[0]))
        # a rejected value leaves the option as it was
        assert lib.bh_set_option(b"free_image_minor", 2) == bh._lib.BH_ERR_INVALID_ARG
        _minor_host(bh, H, P, I["g"])
        assert H.free_image_info(P)["calls_served"] == 3
        # ls_from_cg = 0: no H*w is wanted, the call is eligible as before this option existed — the same under 0 and 1
        bh.set_option("ls_from_cg", 0)
        outs = []
        for opt in (0, 1):
            bh.set_option("free_image_minor", opt)
            served = H.free_image_info(P)["calls_served"]
            outs.append(_minor_host(bh, H, P, I["g"]))
            assert H.free_image_info(P)["calls_served"] == served + 1
        assert outs[0][1:4] == outs[1][1:4] and _same(outs[0][4], outs[1][4]) and np.array_equal(_bits(outs[0][0]), _bits(outs[1][0]))
    finally:
        bh.set_option("ls_from_cg", 1)
        bh.set_option("free_image", 1)
        bh.set_option("free_image_minor", 0)
        H.close()
        P.close()
