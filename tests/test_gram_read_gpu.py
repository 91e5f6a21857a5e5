"""GPU tests of the Gram form read through its lower triangle (bh_hess_set_gram_read / AlHessian.set_gram_read):

    gram_symv_kernel<T, CPT, R, 0, VL> + reduce_partials_kernel    mode "lower": every product through launch_gram_hmul
    gram_symv_kernel<T, CPT, R, 1> + reduce_scalar_kernel          mode "lower+quad": vthv, the line search, the swept model reduction

On the integer instances of tests/gram_read_cases.py (proved exact by tests/test_gram_read_cases_cpu.py) every assertion is equality
of bits: the int64 answer, the handle's own full-read result, any grid.  On badly scaled data the rounding is held against a derived
bound (test_rounding_on_badly_scaled_columns).  Every option touched is back at its default afterwards."""
import ctypes as ct
import functools
import math

import numpy as np
import pytest

import benlsip_ref as R
import gram_cases as gc
import gram_read_cases as grc
import refresh_cases as rc
import rs_cases as rs
from _util import note_tol

pytestmark = pytest.mark.gpu

DEFAULTS = {"gram_cg_fused": 0, "blocks_per_cu": 0, "cauchy_gram": 0, "ls_from_cg": 1}
MODES = ("full", "lower", "lower+quad")


@pytest.fixture
def options(bh):
    def set_options(**kw):
        for k, v in kw.items():
            assert k in DEFAULTS
            bh.set_option(k, v)
    try:
        yield set_options
    finally:
        for k, v in DEFAULTS.items():
            bh.set_option(k, v)


@pytest.fixture(scope="module")
def n_cu(bh):
    n = ct.c_int32(0)
    bh._lib.check(bh._lib.lib().bh_device_info(None, 0, ct.byref(n), None, 0), "bh_device_info")
    return int(n.value)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def gram_handle(bh, inst):
    H = bh.AlHessian(inst.J, inst.C, inst.mu)
    H.set_form("gram")
    return H


def counters(H):
    st = H.stats()
    return dict(n_hmul=st["n_hmul"], n_jv=st["n_jv"], lower=H.products_lower, quads=H.quads_from_g)


def delta(H, before):
    after = counters(H)
    return {k: after[k] - before[k] for k in after}


def full_bytes(n):
    return 8.0 * n * rs.ld_of(n) + 16.0 * n


# ---------------------------------------------------------------------------------------------------------------- the interface
def test_set_and_get_round_trip(bh):
    """Fails without the feature: the two entry points exist, round-trip, refuse bad modes and a NULL handle, and the mode is
    remembered across bh_hess_set_form in both directions without rebuilding G."""
    lib, L = bh._lib.lib(), bh._lib
    inst = grc.instance(129)
    H = bh.AlHessian(inst.J, inst.C, inst.mu)
    try:
        mode, srv, pl, qg = ct.c_int32(-1), ct.c_int32(-1), ct.c_int64(-1), ct.c_int64(-1)
        assert lib.bh_hess_get_gram_read(H.handle, ct.byref(mode), ct.byref(srv), ct.byref(pl), ct.byref(qg)) == L.BH_OK
        assert (mode.value, srv.value, pl.value, qg.value) == (L.BH_GRAM_READ_FULL, 1, 0, 0)
        assert lib.bh_hess_get_gram_read(H.handle, None, None, None, None) == L.BH_OK
        for m in (L.BH_GRAM_READ_LOWER, L.BH_GRAM_READ_LOWER_QUAD, L.BH_GRAM_READ_FULL, L.BH_GRAM_READ_LOWER_QUAD):
            assert lib.bh_hess_set_gram_read(H.handle, m) == L.BH_OK
            assert lib.bh_hess_get_gram_read(H.handle, ct.byref(mode), None, None, None) == L.BH_OK and mode.value == m
        for bad in (-1, 3, 7):
            assert lib.bh_hess_set_gram_read(H.handle, bad) == L.BH_ERR_INVALID_ARG
            assert H.gram_read == "lower+quad"                                           # the handle keeps its mode
        assert lib.bh_hess_set_gram_read(None, 1) == L.BH_ERR_INVALID_ARG
        assert lib.bh_hess_get_gram_read(None, ct.byref(mode), None, None, None) == L.BH_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            H.set_gram_read("upper")
        # set in the implicit form: no effect there (the product sweeps J, nothing is counted), remembered into the Gram form
        before = counters(H)
        assert same_bits(H * inst.v, inst.y) and same_bits(bh.vthv(H, inst.v), inst.q)
        assert delta(H, before) == dict(n_hmul=1, n_jv=1, lower=0, quads=0)
        assert lib.bh_hess_set_form(H.handle, 2) == L.BH_ERR_INVALID_ARG
        H.set_form("gram")
        assert H.gram_read == "lower+quad" and H.gram_builds == 0
        before = counters(H)
        assert same_bits(H * inst.v, inst.y) and same_bits(bh.vthv(H, inst.v), inst.q)
        assert delta(H, before) == dict(n_hmul=1, n_jv=0, lower=1, quads=1) and H.gram_builds == 1
        H.set_gram_read("full")
        assert H.gram_builds == 1                                                        # never rebuilds G
        H.set_form("implicit")
        H.set_gram_read("lower")
        H.set_form("gram")
        assert H.gram_read == "lower" and H.gram_read_served
        ms = ct.c_double(0.0)
        assert lib.bh_time_kernel(H.handle, 11, 2, ct.byref(ms)) == L.BH_OK and ms.value > 0.0
        assert lib.bh_time_kernel(H.handle, 10, 2, ct.byref(ms)) == L.BH_OK and ms.value > 0.0
        assert (H.products_lower, H.quads_from_g) == (1, 1)                              # timing launches are not counted
        assert lib.bh_time_kernel(H.handle, 12, 2, ct.byref(ms)) == L.BH_ERR_INVALID_ARG
        H.set_form("implicit")
        assert lib.bh_time_kernel(H.handle, 11, 2, ct.byref(ms)) == L.BH_ERR_PRECONDITION
    finally:
        H.close()


# -------------------------------------------------------------------------------------------------------- products, bit for bit
def _products(bh, H, inst, g):
    """H v through bh_hmul, bh_hmul_dev and H v + g through bh_hmul_add_dev."""
    lib, chk = bh._lib.lib(), bh._lib.check
    n = inst.n
    dv, dg, dt = bh.DeviceVector(n, inst.v), bh.DeviceVector(n, g), bh.DeviceVector(n)
    y_host = H * inst.v
    chk(lib.bh_hmul_dev(H.handle, dv.ptr, dt.ptr), "hmul_dev")
    y_dev = dt.download()
    chk(lib.bh_hmul_add_dev(H.handle, dv.ptr, dg.ptr, dt.ptr), "hmul_add_dev")
    y_add = dt.download()
    for d in (dv, dg, dt):
        d.close()
    return y_host, y_dev, y_add


@pytest.mark.parametrize("n", grc.SERVED_WIDTHS)
def test_products_from_the_lower_triangle_bit_for_bit(bh, options, n):
    """bh_hmul, bh_hmul_dev and bh_hmul_add_dev under mode "lower", two grids: the int64 answer and the handle's own full-read
    result as uint64; products_lower grows by one per product, n_hmul and n_jv move as under "full"; bytes_per_hmul is the triangle
    formula."""
    inst = grc.instance(n)
    g = np.arange(1, n + 1, dtype=np.float64) % 13 - 6.0
    H = gram_handle(bh, inst)
    try:
        assert H.gram_read_served
        for bpc in (0, 2):
            options(blocks_per_cu=bpc)
            H.set_gram_read("full")
            assert H.stats()["bytes_per_hmul"] == full_bytes(n)
            before = counters(H)
            full = _products(bh, H, inst, g)
            d_full = delta(H, before)
            assert d_full["lower"] == 0 and d_full["quads"] == 0
            H.set_gram_read("lower")
            assert H.stats()["bytes_per_hmul"] == grc.lower_bytes(n) + 16.0 * n
            before = counters(H)
            low = _products(bh, H, inst, g)
            d_low = delta(H, before)
            assert d_low == dict(d_full, lower=3), (d_low, d_full)
            for got, ref, what in zip(low, (inst.y, inst.y, inst.y + g), ("bh_hmul", "bh_hmul_dev", "bh_hmul_add_dev")):
                assert same_bits(got, ref), (n, bpc, what, np.flatnonzero(bits(got) != bits(ref))[:8])
            for got, ref in zip(low, full):
                assert same_bits(got, ref), (n, bpc)
        assert H.gram_builds == 1
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------- quadratic forms, bit for bit
def _quads(bh, H, Ho, inst, cons, g, w_l, w_u):
    """vthv, the line search (host and device operands) and the swept model reduction on the instance's integer vector."""
    lib, chk = bh._lib.lib(), bh._lib.check
    n = inst.n
    q = bh.vthv(H, inst.v)
    a_host = bh.linesearch(g, H, inst.v, w_l, w_u, cons)
    dv = [bh.DeviceVector(n, x) for x in (g, inst.v, w_l, w_u)]
    out = ct.c_double(math.nan)
    chk(lib.bh_linesearch_dev(H.handle, cons.handle, dv[0].ptr, dv[1].ptr, dv[2].ptr, dv[3].ptr, ct.byref(out)), "linesearch_dev")
    a_dev = out.value
    chk(lib.bh_model_reduction_dev(H.handle, dv[0].ptr, dv[1].ptr, ct.byref(out)), "model_reduction_dev")
    for d in dv:
        d.close()
    return q, a_host, a_dev, out.value


@pytest.mark.parametrize("n", grc.SERVED_WIDTHS)
def test_quadratic_forms_from_g_bit_for_bit(bh, options, n):
    """bh_vthv, bh_linesearch(_dev) and bh_model_reduction_dev under "lower+quad": the exact values (int64; the oracle's line search
    on the exact w'Hw) and the handle's own "full" results; n_jv does not move, quads_from_g grows by one per call.  Under "lower"
    the same calls still sweep J."""
    inst = grc.instance(n)
    g = -(np.arange(1, n + 1, dtype=np.float64) % 5 + 1.0) * np.sign(inst.v)             # g.w < 0: the line search has a minimiser
    w_l, w_u = np.full(n, -np.inf), np.full(n, np.inf)
    fix = np.zeros(n, dtype=bool)
    Ho = R.AlHessian(inst.J, inst.C, inst.mu)
    alpha = R.linesearch(g, Ho, inst.v, w_l, w_u, fix, vthv_fn=lambda H_, w_: inst.q)
    model = float(int(g @ inst.v) * 2 + int(inst.q)) / 2.0                               # g.s + s'Hs / 2, exact
    want = (inst.q, alpha, alpha, model)
    H = gram_handle(bh, inst)
    cons = bh.MixedConstraints(np.zeros((0, n)), None, fix)
    try:
        for bpc in (0, 2):
            options(blocks_per_cu=bpc)
            res = {}
            for mode in MODES:
                H.set_gram_read(mode)
                before = counters(H)
                res[mode] = _quads(bh, H, Ho, inst, cons, g, w_l, w_u)
                d = delta(H, before)
                assert d == (dict(n_hmul=0, n_jv=0, lower=0, quads=4) if mode == "lower+quad" else dict(n_hmul=0, n_jv=4, lower=0, quads=0)), (mode, d)
                for got, ref, what in zip(res[mode], want, ("bh_vthv", "bh_linesearch", "bh_linesearch_dev", "bh_model_reduction_dev")):
                    assert same_bits(got, ref), (n, bpc, mode, what, got, ref)
    finally:
        cons.close()
        H.close()


def test_minor_iterate_with_its_own_vthv(bh, options):
    """bh_minor_iterate with ls_from_cg = 0 on the exact family C2 (dense G, dyadic iterates): w, the status and alpha under every
    mode are the oracle's bits; under "lower+quad" the line search's w'Hw comes from G (n_jv unchanged, quads_from_g + 1) and the
    loop's products from the lower triangle; under "lower" the line search sweeps J."""
    n = 1000
    inst = gc.cg_instance("C2", n)
    case = gc.cg_case("C2", n, 0, "tie", "upper")
    g = case.g
    x, s = np.zeros(n), np.zeros(n)
    big = 2.0 ** 20
    Ho = R.AlHessian(inst.J, inst.C, inst.mu)
    cons_o = R.make_mixed_constraints(np.zeros((0, n)), R.chol_lower(np.zeros((0, 0))), inst.fix, l=np.full(n, -big), u=np.full(n, big))
    w_ref, st_ref = R.minor_iterate(x, s, g, Ho, cons_o, 2.0 ** 10, case.kappa2)
    H = bh.AlHessian(inst.J, inst.C, inst.mu)
    H.set_form("gram")
    cons = bh.MixedConstraints(np.zeros((0, n)), None, inst.fix, l=np.full(n, -big), u=np.full(n, big))
    options(ls_from_cg=0)
    try:
        for mode in MODES:
            H.set_gram_read(mode)
            before = counters(H)
            w, st, info = bh.minor_iterate(x, s, g, H, cons, 2.0 ** 10, case.kappa2, full_output=True)
            d = delta(H, before)
            assert int(st) == int(st_ref) and same_bits(w, w_ref), (mode, st, st_ref, np.flatnonzero(bits(w) != bits(w_ref))[:8])
            assert d["n_hmul"] == info["n_hmul"] >= 2
            assert (d["n_jv"], d["quads"]) == ((0, 1) if mode == "lower+quad" else (1, 0)), (mode, d)
            # (launches: the scheduler may enqueue products past the loop's end; those are skipped on the device but counted)
            assert d["lower"] == 0 if mode == "full" else d["lower"] >= info["n_hmul"], (mode, d)
    finally:
        cons.close()
        H.close()


# ------------------------------------------------------------------------------------------------------------ through the loops
@functools.lru_cache(maxsize=None)
def _cg_ref(family, n, index, kind, side):
    ref = gc.cg_oracle(gc.cg_case(family, n, index, kind, side))
    ref[0].setflags(write=False)
    ref[3].setflags(write=False)
    return ref


@pytest.mark.parametrize("family,n", [(f, n) for f in ("C2", "C3") for n in (500, 2050, 4099)])
def test_separate_kernel_cg_loop_under_lower_is_the_oracle(bh, options, n_cu, family, n):
    """The separate-kernel Gram CG loop (gram_cg_fused = 0) with every H*p from the lower triangle: status, iters, n_hmul, every trace
    row and w bit for bit against the oracle; products_lower grows by the loop's products.  With gram_cg_fused = 1 the loop reads
    whole rows: the same bits, products_lower does not move."""
    inst = gc.cg_instance(family, n)
    H = bh.AlHessian(inst.J, inst.C if inst.C.shape[0] else None, inst.mu)
    H.set_form("gram")
    H.set_gram_read("lower")
    cons = bh.MixedConstraints(np.zeros((0, n)), None, inst.fix)
    try:
        for c in gc.cg_cases(family, n, n_cu, 0)[:6]:
            ref = _cg_ref(family, n, c.index, c.kind, c.side)
            for fused in (0, 1):
                options(gram_cg_fused=fused)
                before = counters(H)
                w, st, info = bh.projected_cg(c.g, H, c.w_l, c.w_u, cons, c.kappa2, trace_cap=8, full_output=True)
                d = delta(H, before)
                what = "%s n=%d i=%d %s from %s, gram_cg_fused=%d" % (family, n, c.index, c.kind, c.side, fused)
                assert (int(st), info["iters"], info["n_hmul"]) == (ref[1], ref[2], ref[3].shape[0]), what
                assert same_bits(info["trace"], ref[3]) and same_bits(w, ref[0]), what
                # (launches: products enqueued past the loop's end are skipped on the device but counted)
                assert (d["lower"] == 0 if fused else d["lower"] >= info["n_hmul"]) and d["n_hmul"] == info["n_hmul"], (what, d)
                assert H.stats()["cg_kernels"] == (2 if fused else 0)
    finally:
        cons.close()
        H.close()


def test_cauchy_gram_search_under_lower_is_the_oracle(bh, options):
    """One family-K search with cauchy_gram = 1: its one product G d comes from the lower triangle, the search itself reads whole
    rows; step, active set and passes are the oracle's."""
    c = gc.k_cases(1030)[0]
    J, C, mu, A, x, g, xlow, xupp, dlt = c.inst
    s_ref, fix_ref, passes = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, dlt)
    H = bh.AlHessian(J, C if C.shape[0] else None, mu)
    H.set_form("gram")
    H.set_gram_read("lower")
    options(cauchy_gram=1)
    cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
    try:
        before = counters(H)
        s, info = bh.cauchy_step(x, g, H, cons, dlt, full_output=True)
        d = delta(H, before)
        assert info["form"] == 3 and info["n_hmul"] == passes
        assert np.array_equal(np.asarray(cons.fixvars, dtype=bool), fix_ref) and same_bits(s, s_ref)
        assert (d["n_hmul"], d["n_jv"], d["lower"]) == (1, 0, 1), d
    finally:
        cons.close()
        H.close()


# ------------------------------------------------------------------------------------------------- rounding on badly scaled data
def _two_prod(a, b):
    """a * b = p + e exactly (Veltkamp / Dekker; no fma in NumPy).  a, b: float64 arrays far from over- and underflow."""
    p = a * b
    split = 134217729.0                                                                  # 2^27 + 1
    ca, cb = split * a, split * b
    ah, bh_ = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh_
    return p, ((ah * bh_ - p) + ah * bl + al * bh_) + al * bl


@pytest.mark.parametrize("n", [1000, 4097])
def test_rounding_on_badly_scaled_columns(bh, n_cu, n):
    """Column scaling 10^(-3 j / n).  G is the handle's own: column j is the full-read product with e_j, which is exact (one non-zero
    term per row).  y^ and q^ are the exact sums of the exact products G_ij v_j (two-product + math.fsum).

    Bound (derived, not fitted).  Every term G_ij v_j of y_i goes through one rounding where it is formed (an fma into the dot or into
    the slab accumulator) and then through at most (a) the rest of a thread's fma chain, 2 CPT - 1 <= 31, the six butterfly steps and
    the NW <= 8 cross-wave adds of the row's dot, or the fmas of the other rows of its workgroup, at most ceil(n / grid) + R; (b) the
    add of t_i into the slab; (c) the slab reduction, grid - 1 adds in any tree.  That is fewer than k = n + grid + 2 roundings for
    the widths here, so |y - y^|_i <= gamma_k (|G||v|)_i with gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability,
    §3.1, any summation order).  v'G v: the terms v_i G_ij v_j pass one product more and the scalar reduction instead of the slab
    reduction: the same k with |v|'|G||v|."""
    rng = np.random.default_rng(n)
    scale = 10.0 ** (-3.0 * np.arange(n) / n)
    J = rng.standard_normal((grc.ROWS, n)) * scale
    C = rng.standard_normal((1, n)) * scale
    v = rng.standard_normal(n)
    H = bh.AlHessian(J, C, 0.5)
    H.set_form("gram")
    try:
        G = np.empty((n, n))
        e = np.zeros(n)
        for j in range(n):
            e[j] = 1.0
            G[:, j] = H * e
            e[j] = 0.0
        assert np.array_equal(G, G.T)                                                    # bitwise symmetric, as the header says
        H.set_gram_read("lower+quad")
        y = H * v
        q = bh.vthv(H, v)
        assert (H.products_lower, H.quads_from_g) == (1, 1)
    finally:
        H.close()
    grid = rs.grid_for(rs.path_of(n), n, n_cu, 0)
    k = n + grid + 2
    u = 2.0 ** -53
    gamma = k * u / (1.0 - k * u)
    P, E = _two_prod(G, v[None, :])
    absGv = np.abs(G) @ np.abs(v)
    worst = 0.0
    for i in range(n):
        err = abs(math.fsum(np.concatenate([P[i], E[i], [-y[i]]])))                      # |y^_i - y_i|, the exact sum rounded once
        worst = max(worst, err / (gamma * absGv[i]))
        note_tol("gram read: |G v - exact| vs gamma_(n+grid+2) |G||v|, per element", err, gamma * absGv[i], "n=%d row %d" % (n, i))
        assert err <= gamma * absGv[i], (n, i, err, gamma * absGv[i])
    # v'G v: the exact sum of v_i (G_ij v_j), each term the four exact pieces of (P + E)_ij * v_i; G is bitwise symmetric, so the
    # strict lower triangle counts twice (an exact doubling) and the upper one is left out
    terms = [np.array([-q])]
    low = np.tril_indices(n, -1)
    for part in (P, E):
        p2, e2 = _two_prod(part, v[:, None])
        terms += [2.0 * p2[low], 2.0 * e2[low], np.diagonal(p2), np.diagonal(e2)]
    err_q = abs(math.fsum(np.concatenate(terms)))
    bound_q = gamma * float(np.abs(v) @ absGv)
    note_tol("gram read: |v'G v - exact| vs gamma_(n+grid+2) |v|'|G||v|", err_q, bound_q, "n=%d" % n)
    print("n=%d grid=%d: worst share of the bound, G v %.3e, v'G v %.3e" % (n, grid, worst, err_q / bound_q))
    assert err_q <= bound_q, (n, err_q, bound_q)


# ----------------------------------------------------------------------------------------------------------------- not served
def test_a_width_without_a_lower_kernel_keeps_the_full_read(bh):
    """n = 8200 (8192 < n <= 16384): served = 0; under every mode the product and vthv are the full-read bits, both counters stay 0,
    bytes_per_hmul stays 8 n ld + 16 n and bh_time_kernel kind 11 refuses."""
    n = grc.UNSERVED_WIDTH
    assert not grc.served(n)
    inst = grc.instance(n)
    v = np.random.default_rng(5).standard_normal(n)
    H = gram_handle(bh, inst)
    try:
        assert not H.gram_read_served
        res = {}
        for mode in MODES:
            H.set_gram_read(mode)
            before = counters(H)
            res[mode] = (H * v, bh.vthv(H, v), H * inst.v, bh.vthv(H, inst.v))
            assert delta(H, before) == dict(n_hmul=2, n_jv=2, lower=0, quads=0)
            assert H.stats()["bytes_per_hmul"] == full_bytes(n)
            assert same_bits(res[mode][2], inst.y) and same_bits(res[mode][3], inst.q)
            for a, b in zip(res[mode], res["full"]):
                assert same_bits(a, b), mode
        ms = ct.c_double(0.0)
        assert bh._lib.lib().bh_time_kernel(H.handle, 11, 1, ct.byref(ms)) == bh._lib.BH_ERR_PRECONDITION
        assert bh._lib.lib().bh_time_kernel(H.handle, 10, 1, ct.byref(ms)) == bh._lib.BH_OK
    finally:
        H.close()


# -------------------------------------------------------------------------------------------------------------- mode 0 is today
@pytest.mark.parametrize("n", [513, 4097])
def test_mode_full_set_explicitly_is_the_untouched_handle(bh, n):
    """On real-valued data: a handle whose mode was never touched, and one that went through "lower+quad" and back to "full", give
    the same bits and move the same counters in every call of the modules above."""
    rng = np.random.default_rng(40 + n)
    J, C = rng.standard_normal((grc.ROWS, n)), rng.standard_normal((1, n))
    v, g = rng.standard_normal(n), rng.standard_normal(n)
    w_l, w_u = np.full(n, -np.inf), np.full(n, np.inf)
    out = []
    for touch in (False, True):
        H = bh.AlHessian(J, C, 0.5)
        H.set_form("gram")
        if touch:
            H.set_gram_read("lower+quad")
            H.set_gram_read("full")
        cons = bh.MixedConstraints(np.zeros((0, n)), None, np.zeros(n, dtype=bool))
        try:
            before = counters(H)
            inst = grc.Instance(n, J, C, 0.5, None, v, None, None)
            res = _products(bh, H, inst, g) + _quads(bh, H, None, inst, cons, g, w_l, w_u)
            out.append((res, delta(H, before), H.stats()["bytes_per_hmul"], H.gram_builds))
        finally:
            cons.close()
            H.close()
    (r0, d0, b0, g0), (r1, d1, b1, g1) = out
    assert (d0, b0, g0) == (d1, b1, g1) and d0 == dict(n_hmul=3, n_jv=4, lower=0, quads=0) and b0 == full_bytes(n)
    for a, b in zip(r0, r1):
        assert same_bits(a, b)
