"""The box-constrained CG loop on the compact image of the free columns (option free_image), bit for bit.

The differential.  For every state of the sequences S1..S5 of tests/free_image_cases.py (active sets pushed to ONE Hessian handle under
free_image = 2: builds, moves of 1..323 columns, stride > width, widths on and around the multiples of 16 and the pick_config thresholds,
two constraint handles taking turns) projected_cg runs on the sequence's handle, and then on a FRESH handle built from the explicitly
compacted problem J' = J[:, map[:w]], C' = C[:, map[:w]], g' = g[map[:w]], bounds gathered likewise, nothing fixed, under
free_image = 0.  By pcg_run (csrc/bh_api.hip), the CG prologue of row_stream_kernel and cg_reduce_update_kernel the two loops perform the
same operations in the same order: the same pick_config for the same chunk count, the same grid (equal row counts, blocks_per_cu pinned),
the same column order inside a row and the same chunk ownership, max_iter = 2 w, a null mask, correctly rounded divisions, unfused
multiply-adds in the update, slab sums in a fixed order — only the row stride and the buffer addresses differ.  So status, iters, n_hmul,
every trace row and w are demanded EQUAL AS uint64, with real-valued operands, over all iterations.  The reference of this comparison is
the library's own full-image loop; that is legitimate because that loop is checked against the oracle and against integers on its own in
tests/test_row_stream_exact_gpu.py, and is anchored again here: the first state and the last state of width >= 2 of every sequence are
also held against the oracle with assert_w_close / w_tolerance, and one whole iteration is checked against integer ground truth that uses
neither the oracle's rounding nor the device's full path (J'J = 16 I on any set of columns).

Two bounds settings per state (free_image_cases.py): wide (kappa2 = 0.01, ends solved after up to 14 products) and a box whose radius makes
the oracle end on the boundary.

Trace column 3 holds r.v AFTER the update of its iteration (the oracle's CGTrace and the device agree on that: the next launch's
prologue writes it) where the loop went on or ended solved, and r.v before it where the loop ended on the boundary: the row of the exact
solved iteration is {16 |g_f|^2, 1/16, gamma, +0}, of the exact boundary iteration {16 |g_f|^2, 1/16, 2^-6, |g_f|^2}.
"""
import ctypes as ct

import numpy as np
import pytest

import benlsip_ref as R
import free_image_cases as F
from _util import assert_w_close, relnorm, w_tolerance
from test_free_image_gpu import _assert_image, _bits

pytestmark = pytest.mark.gpu

TRACE_CAP = 64
TOL_LABEL = "projected_cg: w vs oracle (tolerance max(1e-9, 20 x oracle sensitivity))"


@pytest.fixture(scope="module")
def n_cu(bh):                                  # (as the fixture of test_free_image_gpu.py: the two pin and restore the same options)
    n = ct.c_int32(0)
    bh._lib.check(bh._lib.lib().bh_device_info(None, 0, ct.byref(n), None, 0), "bh_device_info")
    bh.set_option("blocks_per_cu", 1)
    try:
        yield int(n.value)
    finally:
        bh.set_option("blocks_per_cu", 0)
        bh.set_option("free_image", 1)


def _pcg_host(bh, H, cons, g, w_l, w_u, kappa2=F.KAPPA2):
    w, status, info = bh.projected_cg(g, H, w_l, w_u, cons, kappa2, trace_cap=TRACE_CAP, full_output=True)
    return w, int(status), info["iters"], info["n_hmul"], info["trace"]


def _pcg_dev(bh, H, cons, g, w_l, w_u, kappa2=F.KAPPA2):
    """bh_pcg_dev on device vectors (n == ld, 16-byte aligned: used in place); w arrives pre-filled with a non-zero pattern."""
    n = H.n
    dv = [bh.DeviceVector(n, v) for v in (g, w_l, w_u, np.full(n, 7.25))]
    try:
        status, iters, n_hmul = ct.c_int32(-1), ct.c_int32(0), ct.c_int32(0)
        trace = np.full((TRACE_CAP, 4), np.nan)
        bh._lib.check(bh._lib.lib().bh_pcg_dev(H.handle, cons.handle, dv[0].ptr, dv[1].ptr, dv[2].ptr, float(kappa2), bh.operators.SQRT_EPS,
                                               1e-10, dv[3].ptr, ct.byref(status), ct.byref(iters), bh._lib.ptr(trace), TRACE_CAP,
                                               ct.byref(n_hmul)), "bh_pcg_dev")
        return dv[3].download(), status.value, iters.value, n_hmul.value, trace[:min(TRACE_CAP, n_hmul.value)]
    finally:
        for v in dv:
            v.close()


def _compact_run(bh, Jfull, m, g, w_l, w_u, kappa2=F.KAPPA2):
    """The ordinary full-image loop on the explicitly compacted problem (fresh handles, free_image = 0)."""
    w = m.shape[0]
    d = Jfull.shape[0] - F.Q
    Hc = bh.AlHessian(np.ascontiguousarray(Jfull[:d, m]), np.ascontiguousarray(Jfull[d:, m]), F.MU)
    cc = bh.MixedConstraints(np.zeros((0, w)), None, None)
    try:
        bh.set_option("free_image", 0)
        outs = [_pcg_host(bh, Hc, cc, g_[m], l_[m], u_[m], kappa2) for g_, l_, u_ in zip(g, w_l, w_u)]
        assert Hc.free_image_info(cc)["builds"] == 0
        return outs
    finally:
        bh.set_option("free_image", 2)
        Hc.close()
        cc.close()


def _assert_pair(got, ref, m, fix, what):
    """The compact-image call `got` (on n variables) against the compacted-problem call `ref` (on w): everything as uint64."""
    w, status, iters, n_hmul, trace = got
    wc, status_c, iters_c, n_hmul_c, trace_c = ref
    assert (status, iters, n_hmul) == (status_c, iters_c, n_hmul_c), (what, (status, iters, n_hmul), (status_c, iters_c, n_hmul_c))
    assert trace.shape == trace_c.shape == (min(TRACE_CAP, n_hmul), 4)
    diff = np.argwhere(_bits(trace) != _bits(trace_c))
    assert diff.size == 0, (what, "trace (row, column) differs first at", diff[0], trace[diff[0][0]], trace_c[diff[0][0]])
    bad = np.flatnonzero(_bits(w[m]) != _bits(wc))
    assert bad.size == 0, (what, "w differs in slots", bad[:8], w[m][bad[:8]], wc[bad[:8]])
    assert not _bits(w[fix]).any(), (what, "w is not +0 on the fixed variables", np.flatnonzero(_bits(w[fix]))[:8])


@pytest.mark.parametrize("name", list(F.SEQS))
def test_cg_on_the_compact_image_equals_the_compacted_problem_bit_for_bit(bh, n_cu, name):
    I = F.instance(name, n_cu)
    n, g = I["n"], I["g"]
    sts = F.states(name)
    Jfull = np.vstack([I["J"], I["C"]])
    assert Jfull.shape[0] == F.rows_for(name, n_cu)
    anchors = {0, max(k for k, s in enumerate(sts) if s.width >= 2)}
    run = _pcg_dev if name == "S3" else _pcg_host
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    cons = {}
    served = 0
    try:
        bh.set_option("free_image", 2)
        for k, st in enumerate(sts):
            what = "%s state %d (width %d, stride %d, %s %d)" % (name, k, st.width, st.ldf, st.action, st.k)
            if st.who not in cons:
                cons[st.who] = bh.MixedConstraints(I["A"], None, st.fix.copy())
            elif k > 0 and sts[k - 1].who == st.who and np.array_equal(sts[k - 1].fix, st.fix):
                arr = cons[st.who].fixvars                        # the same array written again and pushed again
                arr[:] = st.fix
                cons[st.who].mark_dirty()
            elif not np.array_equal(cons[st.who].fixvars, st.fix):
                cons[st.who].fixvars = st.fix.copy()             # (S4: a handle whose turn comes again still holds its set)
            P = cons[st.who]
            cells = [F.cell(name, n_cu, k, s, band=k in anchors) for s in ("wide", "box")]
            got = []
            for c in cells:
                got.append(run(bh, H, P, g, c["w_l"], c["w_u"]))
                served += 1
                if c is cells[0]:
                    # the action this call took: build / move of k / use
                    info, mp = _assert_image(H, P, Jfull, st.fix, builds=st.builds, moves=st.moves)
                    assert np.array_equal(mp, st.map), (what, "the device map is not the mirror's")
                else:
                    info = H.free_image_info(P)                   # the epoch fast path: nothing built, nothing moved
                    assert (info["state"], info["width"], info["builds"], info["moves"]) == ("valid", st.width, st.builds, st.moves), (what, info)
                assert info["calls_served"] == served, (what, info)
            m = st.map[:st.width].astype(np.int64)
            ref = _compact_run(bh, Jfull, m, [g, g], [c["w_l"] for c in cells], [c["w_u"] for c in cells])
            for c, a, b, setting in zip(cells, got, ref, ("wide", "box")):
                _assert_pair(a, b, m, st.fix, what + " " + setting)
                assert a[1] == (int(R.CGStatus.solved) if setting == "wide" else int(R.CGStatus.bound_hit)), (what, setting, a[1:4])
                if k in anchors:
                    assert set(c["band"].values()) == {(c["status"], c["iters"])}, (
                        "the ORACLE, on this machine's BLAS, does not decide its own iteration count (no device result is involved)", c["band"])
                    assert a[1:4] == (c["status"], c["iters"], c["n_hmul"]), (what, setting, a[1:4], (c["status"], c["iters"], c["n_hmul"]))
                    tol = w_tolerance(g, I["Ho"], c["w_l"], c["w_u"], c["cons_o"], F.KAPPA2, c["w"])
                    print("[%s %s] ||w - w_oracle|| / ||w_oracle|| = %.3e (tolerance %.3e), %d products" % (what, setting, relnorm(a[0], c["w"]), tol, a[3]))
                    assert_w_close(a[0], c["w"], tol, TOL_LABEL, what + " " + setting)
    finally:
        bh.set_option("free_image", 1)
        H.close()
        for P in cons.values():
            P.close()


def test_no_curvature_along_the_first_direction(bh, n_cu):
    """J and C are zero in every free column on which g is non-zero: p_1'Hp_1 = 0, no step is taken (add_w false).  Status and iters as on
    the compacted problem, and w all +0 bits."""
    I = F.instance("S1", n_cu)
    st = F.states("S1")[3]
    n = I["n"]
    free = np.flatnonzero(~st.fix)
    on = free[::3]
    Jfull = np.vstack([I["J"], I["C"]]).copy()
    Jfull[:, on] = 0.0
    g = np.zeros(n)
    g[on] = I["g"][on]
    g[st.fix] = I["g"][st.fix]                                   # (the fixed entries of g are the mask's business)
    c = F.cell("S1", n_cu, 3, "wide", band=False)
    d = Jfull.shape[0] - F.Q
    H = bh.AlHessian(np.ascontiguousarray(Jfull[:d]), np.ascontiguousarray(Jfull[d:]), F.MU)
    P = bh.MixedConstraints(I["A"], None, st.fix.copy())
    try:
        bh.set_option("free_image", 2)
        got = _pcg_host(bh, H, P, g, c["w_l"], c["w_u"])
        info, mp = _assert_image(H, P, Jfull, st.fix, builds=1, moves=0)
        assert info["calls_served"] == 1
        m = mp[:st.width].astype(np.int64)
        ref = _compact_run(bh, Jfull, m, [g], [c["w_l"]], [c["w_u"]])[0]
        _assert_pair(got, ref, m, st.fix, "no curvature")
        assert got[1:4] == (int(R.CGStatus.negative_curvature), 1, 1), got[1:4]
        assert _bits(got[4][0, 0]) == 0 and not _bits(got[0]).any()          # pHp = +0, w = +0 everywhere
    finally:
        bh.set_option("free_image", 1)
        H.close()
        P.close()


# ---------------------------------------------------------------------------------------- one exact iteration, integer ground truth
def test_one_exact_iteration_on_the_compact_image(bh, n_cu):
    """J'J = 16 I on any subset of columns, C = 0, integer g: p_1 = -mask(g), p'Hp = 16 |g_f|^2, alpha = 1/16, all exact in any order.
    Wide bounds (+-2^20): solved after one product, w = -mask(g) / 16.  Bounds +-2^-6 |g_i| on one free variable: gamma = 2^-6 < alpha, the
    loop ends outside the region at iteration 1 with w = -mask(g) / 64 and that variable exactly on its bound.  After a build, after a move
    that leaves width % 16 == 0, and at width 1."""
    sets, g = F.exact_sets()
    n = F.EXACT_N
    rows = 2 * n_cu * 8 + F.Q
    Jfull = np.vstack([F.exact_jacobian(n, rows - F.Q), np.zeros((F.Q, n))])
    H = bh.AlHessian(np.ascontiguousarray(Jfull[:rows - F.Q]), np.ascontiguousarray(Jfull[rows - F.Q:]), F.MU)
    P = bh.MixedConstraints(np.zeros((0, n)), None, sets[0].copy())
    pick = int(np.flatnonzero(~sets[-1])[0])                     # free in all three states
    try:
        bh.set_option("free_image", 2)
        moves = 0
        for k, fix in enumerate(sets):
            if k:
                moves += int(fix.sum() - sets[k - 1].sum())
                P.fixvars = fix.copy()
            gf2 = float(np.sum(g[~fix] ** 2))
            # wide
            big = F.EXACT_BIG * np.ones(n)
            w, status, iters, n_hmul, trace = _pcg_host(bh, H, P, g, -big, big)
            _assert_image(H, P, Jfull, fix, builds=1, moves=moves)
            assert (status, iters, n_hmul) == (int(R.CGStatus.solved), 2, 1), (k, status, iters, n_hmul)
            want = np.array([16.0 * gf2, 1.0 / 16.0, F.EXACT_BIG / float(np.max(np.abs(g[~fix]))), 0.0])
            assert np.array_equal(_bits(trace[0]), _bits(want)), (k, trace[0], want)
            assert np.array_equal(_bits(w), _bits(np.where(fix, 0.0, -g / 16.0) + 0.0)), k
            # one variable's bounds at 2^-6 |g_i|
            w_l, w_u = -big, big.copy()
            w_l[pick], w_u[pick] = -abs(g[pick]) / 64.0, abs(g[pick]) / 64.0
            w, status, iters, n_hmul, trace = _pcg_host(bh, H, P, g, w_l, w_u)
            assert (status, iters, n_hmul) == (int(R.CGStatus.bound_hit), 1, 1), (k, status, iters, n_hmul)
            want = np.array([16.0 * gf2, 1.0 / 16.0, 1.0 / 64.0, gf2])
            assert np.array_equal(_bits(trace[0]), _bits(want)), (k, trace[0], want)
            assert np.array_equal(_bits(w), _bits(np.where(fix, 0.0, -g / 64.0) + 0.0)), k
            assert w[pick] == (w_l[pick] if g[pick] > 0 else w_u[pick])
        assert H.free_image_info(P)["calls_served"] == 2 * len(sets)
    finally:
        bh.set_option("free_image", 1)
        H.close()
        P.close()


# ------------------------------------------------------------------------------------------------------- the callers of the loop
def test_minor_iterate_without_hw_runs_on_the_image_and_restages_its_vectors(bh, n_cu):
    """bh_minor_iterate with ls_from_cg = 0 hands pcg_run no H*w buffer, so its loop is eligible: the compact operands then overwrite
    the workspace vectors the call staged x, s and the bounds in.  Same status and iters as with the option off, the oracle's w and
    alpha (the assertions of test_minor_iterate_linesearch_gradient_parity), and a second identical call gives the same bits."""
    I = F.instance("S1", n_cu)
    st = F.states("S1")[3]
    assert st.width == 127
    n, fix = I["n"], st.fix
    rng = np.random.default_rng(31)
    xlow, xupp = -np.ones(n), np.ones(n)
    cons_o = R.make_mixed_constraints(I["A"], R.chol_lower(I["A"] @ I["A"].T), fix, l=xlow, u=xupp)
    x = np.clip(0.4 * rng.standard_normal(n), -0.9, 0.9)
    x[fix] = np.where(rng.random(int(fix.sum())) < 0.5, -1.0, 1.0)
    s = 0.01 * rng.standard_normal(n)
    s[fix] = 0.0
    Ho = I["Ho"]
    gm = R.hmul(Ho, s) + I["g"]
    delta = 0.1 * np.linalg.norm(I["g"])
    w_ref, st_ref = R.minor_iterate(x, s, gm, Ho, cons_o, delta, 0.1)
    wl2, wu2 = R.build_step_bounds(x + s, cons_o, delta)
    w_cg, s_cg, it_cg = R.projected_cg(gm, Ho, wl2, wu2, cons_o, 0.1)
    tol = w_tolerance(gm, Ho, wl2, wu2, cons_o, 0.1, w_cg)
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = bh.MixedConstraints(I["A"], None, fix.copy(), l=xlow, u=xupp)
    out = {}
    try:
        bh.set_option("ls_from_cg", 0)
        for opt in (2, 0):
            bh.set_option("free_image", opt)
            before = H.free_image_info(P)["calls_served"]
            w, status, info = bh.minor_iterate(x, s, gm, H, P, delta, 0.1, full_output=True)
            out[opt] = (w, int(status), info["iters"], info["alpha"])
            assert H.free_image_info(P)["calls_served"] - before == (1 if opt == 2 else 0)
            assert int(status) == int(st_ref) and info["iters"] == it_cg
            assert_w_close(w, w_ref, 10 * tol, "minor_iterate: scaled w vs oracle (10 x the CG tolerance: alpha inherits w's sensitivity)",
                           "free_image=%d ls_from_cg=0" % opt)
            if int(st_ref) != int(R.CGStatus.negative_curvature):
                a_cg = R.linesearch(gm, Ho, w_cg, wl2, wu2, cons_o.fixvars)
                assert info["alpha"] == pytest.approx(a_cg, rel=max(1e-6, 1e3 * tol)), (info["alpha"], a_cg, tol)
            assert not _bits(w[fix]).any()
            if opt == 2:
                w2, status2, info2 = bh.minor_iterate(x, s, gm, H, P, delta, 0.1, full_output=True)
                assert H.free_image_info(P)["calls_served"] - before == 2
                assert (int(status2), info2["iters"]) == (int(status), info["iters"]) and np.array_equal(_bits(w2), _bits(w))
                assert _bits(info2["alpha"]) == _bits(info["alpha"])
                _assert_image(H, P, np.vstack([I["J"], I["C"]]), fix, builds=1, moves=0)
        assert out[2][1:3] == out[0][1:3]
    finally:
        bh.set_option("ls_from_cg", 1)
        bh.set_option("free_image", 1)
        H.close()
        P.close()


INNER = dict(d=1027, n=301, seed=3, kappa2=0.5, kappa3=1e-3, minor_steps=6)      # chosen on the CPU against R.inner_step


def test_inner_step_grows_the_active_set_on_the_device_under_the_image(bh, n_cu):
    """bh.inner_step with ls_from_cg = 0: bh_proj_update_active_dev adds a few variables per minor iterate — the moves the image was built
    for.  The oracle's active set grows over four of the six minor iterates of this instance."""
    d, n = INNER["d"], INNER["n"]
    J = R.synthetic_J(d, n, seed=INNER["seed"])
    C0 = np.zeros((0, n))
    inst = R.synthetic_box_vectors(d, n, fix_every=8)
    A = np.zeros((0, n))
    L0 = R.chol_lower(A @ A.T)
    g = J.T @ inst.r0
    delta = R.initial_tr(g)
    cons_o = R.make_mixed_constraints(A, L0, l=inst.x_l, u=inst.x_u)
    log = []
    s_ref, pred_ref = R.inner_step(inst.x, g, R.AlHessian(J, C0, 10.0), L0, cons_o, delta, INNER["minor_steps"], INNER["kappa2"], INNER["kappa3"],
                                   log=log)
    sizes = [e[2] for e in log]
    assert len(log) == INNER["minor_steps"] and sum(b > a for a, b in zip(sizes, sizes[1:])) >= 3, sizes
    out = {}
    try:
        bh.set_option("ls_from_cg", 0)
        for opt in (2, 0):
            bh.set_option("free_image", opt)
            H = bh.AlHessian(J, None, 10.0)
            P = bh.MixedConstraints(A, None, None, l=inst.x_l, u=inst.x_u)
            try:
                s, pred, info = bh.inner_step(inst.x, g, H, P, delta, INNER["minor_steps"], INNER["kappa2"], INNER["kappa3"], full_output=True)
                minor = [(int(a), int(b), int(c)) for a, b, c, _ in info["minor"]]
                out[opt] = minor
                assert [m[0] for m in minor] == [e[1] for e in log]                  # same CG exit status in every minor iterate
                assert [m[2] for m in minor] == sizes                                # same active-set size after every minor iterate
                assert np.array_equal(P.fixvars, cons_o.fixvars)                     # same final active set
                assert relnorm(s, s_ref) <= 1e-6, relnorm(s, s_ref)
                assert pred == pytest.approx(pred_ref, rel=1e-8)
                fi = H.free_image_info(None)
                if opt == 2:
                    print("[inner_step free_image=2] %s; minor iterates (status, iters, fixed): %s" % (fi, minor))
                    # (builds == 1 because the oracle's active set only grows on this instance — asserted above through `sizes`; an
                    # instance that frees a variable would build again, and the image would follow the final set without the extra call)
                    assert sizes == sorted(sizes) and fi["moves"] > 0 and fi["builds"] == 1 and fi["calls_served"] >= 1, fi
                    # the image follows to the final active set with the next eligible call (a move, or nothing to do), and is then
                    # J[:, map] for the final lincons.fixvars
                    final = P.fixvars.copy()
                    P.fixvars = final
                    big = 1e6 * np.ones(n)
                    _pcg_host(bh, H, P, g, -big, big, 0.1)
                    after = _assert_image(H, P, J, final, builds=1)[0]
                    assert after["moves"] >= fi["moves"] and after["calls_served"] == fi["calls_served"] + 1
                else:
                    assert fi["builds"] == 0
            finally:
                H.close()
                P.close()
        assert out[2] == out[0], (out[2], out[0])
    finally:
        bh.set_option("ls_from_cg", 1)
        bh.set_option("free_image", 1)
