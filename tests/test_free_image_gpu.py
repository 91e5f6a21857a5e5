"""The compact image of the free columns (option free_image) on the device: the image itself, bit for bit, after a build and
after every kind of move; the box-constrained CG loop on it against the same loop on the full image and against the oracle;
the calls that must not touch it; and the memory it takes from and returns to the image pool.

Shapes: with blocks_per_cu = 1 the streaming grid is one workgroup per compute unit, and the image has 2 * n_cu * R + 3 rows
(R = rows per step of the geometry that streams the COMPACT width), the last three being the C block (q = 3, mu = 2): every
launch makes two full passes and a third over a partial group that lies behind the mu boundary."""
import ctypes as ct

import numpy as np
import pytest

import benlsip_ref as R
from _util import assert_w_close, oracle_iteration_band, w_tolerance

pytestmark = pytest.mark.gpu

MU = 2.0
Q = 3
# rows per step of the row-stream geometries, by the number of 16-byte chunks of the (padded) width (RsGeoms in bh_api.hip)
GEOM_R = ((64, 8), (256, 8), (512, 8), (1024, 4), (2048, 4), (4096, 2), (8192, 1))
BAND = ("reference", "C-order sums", "1024-row chunks", "rows reversed", "3 row blocks")


def _geometry(width):
    nch = (width + 15) // 16 * 16 // 2
    return next(i for i, (cap, _) in enumerate(GEOM_R) if nch <= cap)


def _rows_per_step(width):
    return GEOM_R[_geometry(width)][1]


@pytest.fixture(scope="module")
def n_cu(bh):
    n = ct.c_int32(0)
    bh._lib.check(bh._lib.lib().bh_device_info(None, 0, ct.byref(n), None, 0), "bh_device_info")
    bh.set_option("blocks_per_cu", 1)
    try:
        yield int(n.value)
    finally:
        bh.set_option("blocks_per_cu", 0)
        bh.set_option("free_image", 1)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fixed(n, nfix, seed):
    fix = np.zeros(n, dtype=bool)
    fix[np.random.default_rng(seed).choice(n, nfix, replace=False)] = True
    return fix


def _assert_image(H, cons, Jfull, fix, builds=None, moves=None):
    """Jf == J[:, map] as uint64 over the live width, +0.0 beyond; the map lists every free variable once; the counters."""
    n = fix.shape[0]
    info = H.free_image_info(cons)
    width = n - int(fix.sum())
    assert info["state"] == "valid" and info["width"] == width, (info, width)
    if builds is not None:
        assert info["builds"] == builds, info
    if moves is not None:
        assert info["moves"] == moves, info
    img, mp = H.free_image_read()
    assert img.shape[0] == Jfull.shape[0] and img.shape[1] % 16 == 0 and img.shape[1] >= width
    assert np.array_equal(np.sort(mp[:width]), np.flatnonzero(~fix)) and np.all(mp[width:] == -1)
    assert np.array_equal(_bits(img[:, :width]), _bits(Jfull[:, mp[:width]]))
    assert not _bits(img[:, width:]).any()
    return info, mp


def _cg_once(bh, H, cons, n, seed=0):
    """One eligible projected_cg (wide bounds: its result is not the point here)."""
    rng = np.random.default_rng(seed)
    return bh.projected_cg(rng.standard_normal(n), H, -np.ones(n), np.ones(n), cons, 0.1, full_output=True)


# ------------------------------------------------------------------------------------------------------------- the image
def test_image_bitwise_after_build_and_every_kind_of_move(bh, n_cu):
    n, nfix = 301, 200
    rows = 2 * n_cu * _rows_per_step(n - nfix) + 3
    d = rows - Q
    rng = np.random.default_rng(5)
    Jfull = rng.standard_normal((rows, n))
    # NaN (two payloads), +-Inf, -0 and denormals, in free and in fixed columns, J rows and C rows
    specials = np.array([0x7ff8000000000000, 0xfff8000000000123, 0x7ff0000000000000, 0xfff0000000000000, 0x8000000000000000, 0x0000000000000001,
                         0x800fffffffffffff], dtype=np.uint64).view(np.float64)
    for k, (i, j) in enumerate(zip(rng.integers(0, rows, 400), rng.integers(0, n, 400))):
        Jfull[i, j] = specials[k % len(specials)]
    Jfull[rows - 1, :] = np.tile(specials, n // len(specials) + 1)[:n]
    fix = _fixed(n, nfix, 6)
    A = np.zeros((0, n))
    H = bh.AlHessian(np.asfortranarray(Jfull[:d]), np.asfortranarray(Jfull[d:]), MU)
    cons = bh.MixedConstraints(A, None, fix)
    try:
        bh.set_option("free_image", 2)
        assert H.free_image_info(cons)["state"] == "none"
        _cg_once(bh, H, cons, n)
        info, mp = _assert_image(H, cons, Jfull, fix, builds=1, moves=0)
        assert np.array_equal(mp[:n - nfix], np.flatnonzero(~fix)) and info["calls_served"] == 1          # built in index order
        # one variable fixed (from the middle of the image)
        fix = fix.copy()
        fix[mp[17]] = True
        cons.fixvars = fix
        assert H.free_image_info(cons)["state"] == "stale"
        _cg_once(bh, H, cons, n)
        info, mp = _assert_image(H, cons, Jfull, fix, builds=1, moves=1)
        # many fixed, among them the variables that sit in the last slots (the tail the moves read from) and the very first slot
        w = n - int(fix.sum())
        fix = fix.copy()
        fix[mp[[0, 3, 40, w - 1, w - 2, w - 5, w - 9]]] = True
        cons.fixvars = fix
        _cg_once(bh, H, cons, n)
        info, mp = _assert_image(H, cons, Jfull, fix, builds=1, moves=8)
        # the same active set pushed again: nothing to do
        cons.mark_dirty()
        _cg_once(bh, H, cons, n)
        info, mp = _assert_image(H, cons, Jfull, fix, builds=1, moves=8)
        # all but one fixed
        keep = int(mp[11])
        fix = np.ones(n, dtype=bool)
        fix[keep] = False
        cons.fixvars = fix
        _cg_once(bh, H, cons, n)
        info, mp = _assert_image(H, cons, Jfull, fix, builds=1, moves=w)
        assert info["width"] == 1 and mp[0] == keep
        served = info["calls_served"]
        # one freed: the image cannot grow.  Under the policy it is stale and the call runs on the full image ...
        fix = fix.copy()
        fix[(keep + 1) % n] = False
        cons.fixvars = fix
        bh.set_option("free_image", 1)
        _cg_once(bh, H, cons, n)
        info = H.free_image_info(cons)
        assert info["state"] == "stale" and info["width"] == 1 and info["builds"] == 1 and info["calls_served"] == served, info
        # ... and option 2 builds it again
        bh.set_option("free_image", 2)
        _cg_once(bh, H, cons, n)
        info, mp = _assert_image(H, cons, Jfull, fix, builds=2, moves=w)
        assert info["width"] == 2 and info["calls_served"] == served + 1
    finally:
        bh.set_option("free_image", 1)
        H.close()
        cons.close()


# ------------------------------------------------------------------------------------------------- projected_cg on the image
SHAPES = {                                   # name: (n, nfix, kappa2, seed, geometry of the full width, geometry of the compact width)
    "n3001_fix380_same_geometry": (3001, 380, 0.1, 1, 4, 4),
    "n3001_fix1500_narrower_geometry": (3001, 1500, 0.3, 2, 4, 3),
    "n301_fix200": (301, 200, 0.01, 3, 1, 0),
    "n6001_fix2000": (6001, 2000, 0.1, 4, 5, 4),
}
_ORACLE = {}


def _instance(name, n_cu):
    if (name, n_cu) not in _ORACLE:
        n, nfix, kappa2, seed = SHAPES[name][:4]
        rows = 2 * n_cu * _rows_per_step(n - nfix) + 3
        d = rows - Q
        rng = np.random.default_rng(seed)
        J = rng.standard_normal((d, n)) / np.sqrt(d)
        C = rng.standard_normal((Q, n))
        fix = _fixed(n, nfix, seed + 100)
        A = np.zeros((0, n))
        cons_o = R.make_mixed_constraints(A, R.chol_lower(A @ A.T), fix, l=-np.ones(n), u=np.ones(n))
        g = J.T @ rng.standard_normal(d) + 1e-3 * rng.standard_normal(n)
        w_l, w_u = R.build_step_bounds(np.where(fix, 1.0, 0.0), cons_o, 0.5 * np.linalg.norm(g))
        Ho = R.AlHessian(J, C, MU)
        tr = R.CGTrace()
        w_ref, s_ref, it_ref = R.projected_cg(g, Ho, w_l, w_u, cons_o, kappa2, trace=tr)
        band = oracle_iteration_band(g, Ho, w_l, w_u, cons_o, kappa2, variants=BAND)
        tol = w_tolerance(g, Ho, w_l, w_u, cons_o, kappa2, w_ref)
        _ORACLE[(name, n_cu)] = dict(n=n, nfix=nfix, kappa2=kappa2, d=d, J=J, C=C, fix=fix, A=A, g=g, w_l=w_l, w_u=w_u, Ho=Ho, cons_o=cons_o,
                                     w_ref=w_ref, s_ref=int(s_ref), it_ref=it_ref, n_hmul=tr.n_hmul, band=band, tol=tol)
    return _ORACLE[(name, n_cu)]


@pytest.mark.parametrize("name", list(SHAPES))
def test_pcg_on_the_compact_image_against_the_full_image_and_the_oracle(bh, n_cu, name):
    I = _instance(name, n_cu)
    n = I["n"]
    # the instance decides its iteration count by itself: every re-association of the oracle's own H*p gives the same one
    assert len(set(I["band"].values())) == 1 and I["band"]["reference"] == (I["s_ref"], I["it_ref"]), I["band"]
    assert (_geometry(n), _geometry(n - I["nfix"])) == SHAPES[name][4:] and (n - I["nfix"]) % 16 != 0
    Jfull = np.vstack([I["J"], I["C"]])
    H = bh.AlHessian(I["J"], I["C"], MU)
    cons = bh.MixedConstraints(I["A"], None, I["fix"])
    try:
        out = {}
        for opt in (0, 2):
            bh.set_option("free_image", opt)
            w, status, info = bh.projected_cg(I["g"], H, I["w_l"], I["w_u"], cons, I["kappa2"], trace_cap=32, full_output=True)
            out[opt] = (w, int(status), info)
            assert (int(status), info["iters"], info["n_hmul"]) == (I["s_ref"], I["it_ref"], I["n_hmul"]), (opt, status, info["iters"], info["n_hmul"])
            print("[%s] free_image=%d: ||w - w_oracle|| / ||w_oracle|| = %.3e (tolerance %.3e)" % (
                name, opt, np.linalg.norm(w - I["w_ref"]) / np.linalg.norm(I["w_ref"]), I["tol"]))
            assert_w_close(w, I["w_ref"], I["tol"], "projected_cg: w vs oracle (tolerance max(1e-9, 20 x oracle sensitivity))", "%s free_image=%d" % (name, opt))
            assert not _bits(w[I["fix"]]).any(), "w is exactly +0 on the fixed variables"
            fi = H.free_image_info(cons)
            assert (fi["builds"], fi["calls_served"]) == ((0, 0) if opt == 0 else (1, 1)), fi
        _assert_image(H, cons, Jfull, I["fix"], builds=1, moves=0)
        # a second call, one variable more on its bound: served from moved columns, no build
        fix2 = I["fix"].copy()
        fix2[np.flatnonzero(~I["fix"])[7]] = True
        cons.fixvars = fix2
        cons_o2 = R.make_mixed_constraints(I["A"], R.chol_lower(I["A"] @ I["A"].T), fix2, l=-np.ones(n), u=np.ones(n))
        w_l2, w_u2 = np.where(fix2, 0.0, I["w_l"]), np.where(fix2, 0.0, I["w_u"])
        tr2 = R.CGTrace()
        w_ref2, s_ref2, it_ref2 = R.projected_cg(I["g"], I["Ho"], w_l2, w_u2, cons_o2, I["kappa2"], trace=tr2)
        band2 = oracle_iteration_band(I["g"], I["Ho"], w_l2, w_u2, cons_o2, I["kappa2"], variants=BAND)
        assert set(band2.values()) == {(int(s_ref2), it_ref2)}, band2
        w2, status2, info2 = bh.projected_cg(I["g"], H, w_l2, w_u2, cons, I["kappa2"], full_output=True)
        fi = _assert_image(H, cons, Jfull, fix2, builds=1, moves=1)[0]
        assert fi["calls_served"] == 2
        assert (int(status2), info2["iters"], info2["n_hmul"]) == (int(s_ref2), it_ref2, tr2.n_hmul)
        assert_w_close(w2, w_ref2, w_tolerance(I["g"], I["Ho"], w_l2, w_u2, cons_o2, I["kappa2"], w_ref2),
                       "projected_cg: w vs oracle (tolerance max(1e-9, 20 x oracle sensitivity))", name + " after a move")
        assert not _bits(w2[fix2]).any()
    finally:
        bh.set_option("free_image", 1)
        H.close()
        cons.close()


@pytest.mark.parametrize("nfix", [3, 6, 0])
def test_tiny_shape_and_nothing_fixed(bh, n_cu, nfix):
    """d = 5, n = 7 with 3 and with 6 of the variables fixed (one free column left); nothing fixed: never built."""
    d, n = 5, 7
    rng = np.random.default_rng(70 + nfix)
    J, C = rng.standard_normal((d, n)), rng.standard_normal((Q, n))
    fix = _fixed(n, nfix, 71)
    A = np.zeros((0, n))
    cons_o = R.make_mixed_constraints(A, R.chol_lower(A @ A.T), fix if nfix else None, l=-np.ones(n), u=np.ones(n))
    g = rng.standard_normal(n)
    w_l, w_u = R.build_step_bounds(np.where(fix, 1.0, 0.0), cons_o, 0.5)
    Ho = R.AlHessian(J, C, MU)
    tr = R.CGTrace()
    w_ref, s_ref, it_ref = R.projected_cg(g, Ho, w_l, w_u, cons_o, 0.01, trace=tr)
    H = bh.AlHessian(J, C, MU)
    cons = bh.MixedConstraints(A, None, fix)
    try:
        bh.set_option("free_image", 2)
        w, status, info = bh.projected_cg(g, H, w_l, w_u, cons, 0.01, full_output=True)
        assert (int(status), info["iters"], info["n_hmul"]) == (int(s_ref), it_ref, tr.n_hmul)
        assert_w_close(w, w_ref, w_tolerance(g, Ho, w_l, w_u, cons_o, 0.01, w_ref),
                       "projected_cg: w vs oracle (tolerance max(1e-9, 20 x oracle sensitivity))", "d=5 n=7 nfix=%d" % nfix)
        if nfix:
            _assert_image(H, cons, np.vstack([J, C]), fix, builds=1, moves=0)
            assert not _bits(w[fix]).any()
        else:
            assert H.free_image_info(cons) == {"state": "none", "width": 0, "builds": 0, "moves": 0, "calls_served": 0}
    finally:
        bh.set_option("free_image", 1)
        H.close()
        cons.close()


def test_first_curvature_is_exact_on_integer_operands(bh, n_cu):
    """Integer J, C, g and mu = 2: p_1 = -mask(g) and every product and sum of p_1'Hp_1 = sum_i w_i (J p_1)_i^2 is exact in fp64
    whatever the order, so the first row of the trace equals the int64 value bit for bit — on the compact image as on the full."""
    n, nfix = 3001, 380
    rows = 2 * n_cu * _rows_per_step(n - nfix) + 3
    d = rows - Q
    rng = np.random.default_rng(9)
    Ji = rng.integers(-3, 4, size=(n, d), dtype=np.int8).T
    Ci = rng.integers(-3, 4, size=(n, Q), dtype=np.int8).T
    gi = rng.integers(-3, 4, size=n).astype(np.int64)
    fix = _fixed(n, nfix, 10)
    p = np.where(fix, 0, -gi)
    t, c = Ji.astype(np.int64) @ p, Ci.astype(np.int64) @ p
    php = int(t @ t) + 2 * int(c @ c)
    assert 3 * 3 * n < 2 ** 26 and php < 2 ** 52                      # every partial sum is an integer below 2^53
    H = bh.AlHessian(Ji.astype(np.float64), Ci.astype(np.float64), MU)
    cons = bh.MixedConstraints(np.zeros((0, n)), None, fix)
    try:
        for opt in (0, 2):
            bh.set_option("free_image", opt)
            w, status, info = bh.projected_cg(gi.astype(np.float64), H, -1e6 * np.ones(n), 1e6 * np.ones(n), cons, 0.1, trace_cap=4, full_output=True)
            assert _bits(info["trace"][0, 0]) == _bits(np.float64(php)), (opt, info["trace"][0, 0], php)
        assert H.free_image_info(cons)["calls_served"] == 1
    finally:
        bh.set_option("free_image", 1)
        H.close()
        cons.close()


# --------------------------------------------------------------------------------------------------------------- the edges
def test_non_finite_g_on_a_fixed_variable_runs_on_the_full_image(bh, n_cu):
    """r = g carries the entry into r.v on the full image (NaN * 0): such a call is handed back to it — same status and the same
    bits of w as with the option off — and is not counted as served."""
    I = _instance("n301_fix200", n_cu)
    n = I["n"]
    H = bh.AlHessian(I["J"], I["C"], MU)
    cons = bh.MixedConstraints(I["A"], None, I["fix"])
    try:
        bh.set_option("free_image", 2)
        bh.projected_cg(I["g"], H, I["w_l"], I["w_u"], cons, I["kappa2"])
        assert H.free_image_info(cons)["calls_served"] == 1
        for bad in (np.nan, np.inf, -np.inf):
            g = I["g"].copy()
            g[np.flatnonzero(I["fix"])[3]] = bad
            out = {}
            for opt in (0, 2):
                bh.set_option("free_image", opt)
                w, status, info = bh.projected_cg(g, H, I["w_l"], I["w_u"], cons, I["kappa2"], full_output=True)
                out[opt] = (w, int(status), info["iters"], info["n_hmul"])
            assert out[0][1:] == out[2][1:] and np.array_equal(_bits(out[0][0]), _bits(out[2][0])), (bad, out[0][1:], out[2][1:])
            assert H.free_image_info(cons)["calls_served"] == 1
        # a non-finite g on a FREE variable is the loop's own business on either image
        bh.set_option("free_image", 2)
        g = I["g"].copy()
        g[np.flatnonzero(~I["fix"])[3]] = np.nan
        w, status, info = bh.projected_cg(g, H, I["w_l"], I["w_u"], cons, I["kappa2"], full_output=True)
        assert H.free_image_info(cons)["calls_served"] == 2
    finally:
        bh.set_option("free_image", 1)
        H.close()
        cons.close()


def test_ineligible_calls_leave_the_counters_unchanged(bh, n_cu):
    """H*w wanted (minor_iterate), linear equalities, atol_f2b = 0 and the Gram form never touch the image."""
    I = _instance("n301_fix200", n_cu)
    n = I["n"]
    H = bh.AlHessian(I["J"], I["C"], MU)
    cons = bh.MixedConstraints(I["A"], None, I["fix"], l=-np.ones(n), u=np.ones(n))
    rng = np.random.default_rng(12)
    Aeq = rng.standard_normal((2, n))
    cons_eq = bh.MixedConstraints(Aeq, None, I["fix"])
    try:
        bh.set_option("free_image", 2)
        before = H.free_image_info(None)
        assert before["builds"] == 0
        x = np.where(I["fix"], 1.0, 0.0)
        bh.minor_iterate(x, np.zeros(n), I["g"], H, cons, 0.5, I["kappa2"])
        bh.projected_cg(I["g"], H, I["w_l"], I["w_u"], cons_eq, I["kappa2"])
        bh.projected_cg(I["g"], H, I["w_l"], I["w_u"], cons, I["kappa2"], atol_f2b=0.0)
        H.set_form("gram")
        bh.projected_cg(I["g"], H, I["w_l"], I["w_u"], cons, I["kappa2"])
        H.set_form("implicit")
        assert H.free_image_info(None) == before
        bh.projected_cg(I["g"], H, I["w_l"], I["w_u"], cons, I["kappa2"])           # the eligible one
        after = H.free_image_info(cons)
        assert after["builds"] == 1 and after["calls_served"] == 1 and after["state"] == "valid"
        bh.minor_iterate(x, np.zeros(n), I["g"], H, cons, 0.5, I["kappa2"])
        bh.projected_cg(I["g"], H, I["w_l"], I["w_u"], cons, I["kappa2"], atol_f2b=0.0)
        assert H.free_image_info(cons) == after
    finally:
        bh.set_option("free_image", 1)
        H.close()
        cons.close()
        cons_eq.close()


def test_destroying_handles_returns_the_memory(bh, n_cu):
    """Create / build / destroy cycles: free device memory settles (give or take what the image pool parks), as tools/leak_check.py
    demands of every other buffer of a handle."""
    hip = ct.CDLL("libamdhip64.so")

    def free_mib():
        f, t = ct.c_size_t(), ct.c_size_t()
        assert hip.hipMemGetInfo(ct.byref(f), ct.byref(t)) == 0
        return f.value / 2 ** 20

    rng = np.random.default_rng(13)
    d, n = 700, 1024                                   # image 5.6 MiB, compact image 4.9 MiB: both above the pool's 1 MiB floor
    J = rng.standard_normal((d, n))
    fix = _fixed(n, 128, 14)
    seen = []
    try:
        bh.set_option("free_image", 2)
        for cycle in range(12):
            H = bh.AlHessian(J, None, MU)
            cons = bh.MixedConstraints(np.zeros((0, n)), None, fix)
            _cg_once(bh, H, cons, n)
            assert H.free_image_info(cons)["builds"] == 1
            H.close()
            cons.close()
            bh._lib.check(bh._lib.lib().bh_synchronize(), "bh_synchronize")
            seen.append(free_mib())
        # the pool holds at most two images: after the first cycles nothing more may be taken from the device
        # (4 MiB: less than one image, so an image lost per cycle shows at once; more than the allocator's own granularity)
        assert max(seen[4:]) - min(seen[4:]) <= 4.0, seen
    finally:
        bh.set_option("free_image", 1)
