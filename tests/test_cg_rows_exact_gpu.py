"""The box-constrained CG loop on an implicit handle, its decisions bit for bit at kernel-sized n, on the exact instances of
tests/cg_rows_cases.py (proved exact, equal to the oracle and placed on the edges they name by tests/test_cg_rows_cases_cpu.py):

    shape                                options                         kernels it pins
    fused, full image                    cg_fused = 1, free_image = 0    row_stream_kernel<CGP = 1> prologue, cg_reduce_update_kernel
    the identical call again             same                            the predicted-stop symbol CGP = 2
    the short case, then the case again  same                            CGP = 2 predicted wrongly: it must carry on
    separate kernels                     cg_fused = 0, fold_init 1 | 0   cg_step_reg_kernel (n <= 8192), cg_step_kernel (8200), cg_init*
    compact image                        cg_fused = 1, free_image = 2    the gather and cg_reduce_update_compact_kernel (one answer, no
                                                                         edge placement claimed: tests/test_free_image_exact_gpu.py)
    device pointers                      bh_pcg_dev, final_sync 0 | 1    the caller's buffers unpadded at n == ld (4096), staging at odd n

Every assertion is equality of bits (float64 viewed as uint64) or of integers: the instances have one right answer whatever the
grid, the pass, the slab or the lane order, so a tie resolved the other way, a gamma partial lost at a run or workgroup edge, a
stale w in the boundary term or a wrong prediction symbol that does not carry on is a different bit.  Every option touched is
back at its default afterwards."""
import ctypes as ct

import numpy as np
import pytest

import cg_rows_cases as cr
import gram_cases as gc

pytestmark = pytest.mark.gpu

DEFAULTS = {"cg_fused": 1, "free_image": 1, "fold_init": 1, "final_sync": 0, "blocks_per_cu": 0}
TRACE_CAP = 8
DEV_SIZES = (2047, 4096, 4099)           # bh_pcg_dev: n == ld (in place) and two odd n (staged)


@pytest.fixture
def options(bh):
    """options(key=value, ...) sets library options; every option this module touches is back at its default afterwards."""
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
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------ the case table
def test_case_table(n_cu, capsys):
    """Prints, once per session and past the capture, what every case makes the kernels do on this device (geometry, grid, passes
    per workgroup, the edge each case places) and FAILS on a device whose grids the instances were not designed for."""
    lines = ["", "Row-form exact cases for %d compute units (tests/cg_rows_cases.py):" % n_cu]
    for family in cr.PLACED:
        for n in cr.SIZES:
            for bpc in gc.cg_grids(n):
                lines += ["  " + line for line in cr.describe_rows(family, n, n_cu, bpc)]
    lines.append("  each placement: C2, C3 as a tie and a half step from w_l and w_u; C2n (the grid of C2) from both sides")
    for n in cr.SIZES:
        t, nn = cr.t_cases(n), cr.n_cases(n)
        lines.append("  T  n=%-5d k=%-4d kappa2 = %.17g | its upper neighbour    N  atol = %.17g | its lower neighbour | %.17g"
                     % (n, cr.t_square(n) ** 2, t[0].kappa2, nn[0].atol, nn[2].atol))
    with capsys.disabled():
        print("\n".join(lines))
    for family in ("C2", "C3", "C2n"):
        for n in cr.SIZES:
            for bpc in gc.cg_grids(n):
                placed = {i for i, _ in cr.rows_placements(family, n, n_cu, bpc)}
                assert placed <= set(cr.rows_reserved(n)), (family, n, bpc, sorted(placed - set(cr.rows_reserved(n))))


# ------------------------------------------------------------------------------------------------------------------ plumbing
_REFS = {}


def ref_of(c):
    """The oracle's (w, status, iters, trace rows) of a case, computed once per session and read-only."""
    key = (c.group, c.n, c.index, c.kind, c.side)
    if key not in _REFS:
        ref = cr.rows_oracle(c)
        ref[0].setflags(write=False)
        ref[3].setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


@pytest.fixture(scope="module")
def cg_handle(bh):
    """cg_handle(family, n): ONE implicit handle and one constraint handle per (family, n), shared by every placement, both grids
    and every shape (the parametrisation keeps them adjacent; the previous pair is closed when the key changes)."""
    slot = {}

    def close():
        if slot:
            slot["H"].close()
            slot["cons"].close()
            slot.clear()

    def get(family, n):
        if slot.get("key") != (family, n):
            close()
            inst = cr.rows_instance(family, n)
            H = bh.AlHessian(inst.J, inst.C if inst.C.shape[0] else None, inst.mu)
            assert H.form == "implicit"
            slot.update(key=(family, n), H=H, cons=bh.MixedConstraints(np.zeros((0, n)), None, inst.fix))
        return slot["H"], slot["cons"]
    try:
        yield get
    finally:
        close()


def _pcg(bh, H, cons, c):
    w, st, info = bh.projected_cg(c.g, H, c.w_l, c.w_u, cons, c.kappa2, atol=c.atol, trace_cap=TRACE_CAP, full_output=True)
    return w, int(st), info["iters"], info["n_hmul"], info["trace"]


def _pcg_dev(bh, H, cons, c):
    """bh_pcg_dev on device vectors of exactly n elements; w arrives pre-filled with a non-zero pattern."""
    n = c.n
    dv = [bh.DeviceVector(n, v) for v in (c.g, c.w_l, c.w_u, np.full(n, 7.25))]
    try:
        status, iters, n_hmul = ct.c_int32(-1), ct.c_int32(0), ct.c_int32(0)
        trace = np.full((TRACE_CAP, 4), np.nan)
        bh._lib.check(bh._lib.lib().bh_pcg_dev(H.handle, cons.handle, dv[0].ptr, dv[1].ptr, dv[2].ptr, float(c.kappa2), float(c.atol), 1e-10,
                                               dv[3].ptr, ct.byref(status), ct.byref(iters), bh._lib.ptr(trace), TRACE_CAP, ct.byref(n_hmul)),
                      "bh_pcg_dev")
        return dv[3].download(), status.value, iters.value, n_hmul.value, trace[:min(TRACE_CAP, n_hmul.value)]
    finally:
        for v in dv:
            v.close()


def _check(out, ref, fix, what):
    w, st, iters, n_hmul, trace = out
    w_ref, st_ref, it_ref, tr_ref = ref
    assert (st, iters, n_hmul) == (st_ref, it_ref, tr_ref.shape[0]), (what, st, iters, n_hmul, st_ref, it_ref, tr_ref.shape[0])
    assert same_bits(trace, tr_ref), (what, trace, tr_ref)
    assert same_bits(w, w_ref), (what, np.flatnonzero(bits(w) != bits(w_ref))[:8])
    assert not np.any(bits(w[fix])), what                                        # fixed components: +0.0


def _fused(bh, options, H, cons, c, fix, what):
    options(cg_fused=1, free_image=0)
    _check(_pcg(bh, H, cons, c), ref_of(c), fix, what + ": fused")
    assert H.stats()["cg_kernels"] == 2, what


def _separate_and_compact(bh, options, H, cons, c, fix, what):
    for fold in (1, 0):
        options(cg_fused=0, free_image=0, fold_init=fold)
        _check(_pcg(bh, H, cons, c), ref_of(c), fix, what + ": cg_fused = 0, fold_init = %d" % fold)
        assert H.stats()["cg_kernels"] == 0, what
    options(cg_fused=1, free_image=2, fold_init=1)
    served = H.free_image_info(cons)["calls_served"]
    _check(_pcg(bh, H, cons, c), ref_of(c), fix, what + ": compact image")
    info = H.free_image_info(cons)
    assert H.stats()["cg_kernels"] == 2 and (info["state"], info["width"], info["calls_served"]) == ("valid", c.n - int(fix.sum()), served + 1), (what, info)
    options(free_image=0)


def _device_pointers(bh, options, H, cons, c, fix, what):
    if c.n not in DEV_SIZES:
        return
    options(cg_fused=1, free_image=0)
    for sync in (0, 1):
        options(final_sync=sync)
        _check(_pcg_dev(bh, H, cons, c), ref_of(c), fix, what + ": bh_pcg_dev, final_sync = %d" % sync)
        assert H.stats()["cg_kernels"] == 2, what
    options(final_sync=0)


# ---------------------------------------------------------------------------------------------------------- families C2 and C3
@pytest.mark.parametrize("family,n,bpc", [(f, n, b) for f in cr.PLACED for n in cr.SIZES for b in gc.cg_grids(n)])
def test_cg_rows_is_the_oracle_bit_for_bit(bh, options, n_cu, cg_handle, family, n, bpc):
    """Every placement of (family, n) at one grid, all on one handle, each as a tie and as a half step, through every shape of
    the table above."""
    inst = cr.rows_instance(family, n)
    H, cons = cg_handle(family, n)
    options(blocks_per_cu=bpc)
    assert {i for i, _ in cr.rows_placements(family, n, n_cu, bpc)} <= set(inst.deciding)
    short = cr.short_case(family, n)
    assert ref_of(short)[1:3] == (1, 1)
    for c in cr.placed_cases(family, n, n_cu, bpc):
        what = "%s n=%d bpc=%d i=%d %s from %s (%s)" % (family, n, bpc, c.index, c.kind, c.side, c.edge)
        assert ref_of(c)[2] >= 2
        _fused(bh, options, H, cons, c, inst.fix, what)
        _check(_pcg(bh, H, cons, c), ref_of(c), inst.fix, what + ": fused, the identical call again")
        _check(_pcg(bh, H, cons, short), ref_of(short), inst.fix, what + ": the one-iteration call")
        _check(_pcg(bh, H, cons, c), ref_of(c), inst.fix, what + ": fused, after a shorter call")
        assert H.stats()["cg_kernels"] == 2
        _separate_and_compact(bh, options, H, cons, c, inst.fix, what)
        _device_pointers(bh, options, H, cons, c, inst.fix, what)


# ------------------------------------------------------------------------------------------------------------ families T and N
@pytest.mark.parametrize("n", cr.SIZES)
def test_tolerance_tie_goes_on_and_its_neighbour_stops(bh, options, cg_handle, n):
    """Family T: |r.v| == tol_cg after iteration 2 is not < (iters 4, three products, w the exact minimiser); one ulp of kappa2
    more and the loop ends there (iters 3)."""
    inst = cr.rows_instance("C3", n)
    H, cons = cg_handle("C3", n)
    tie, above = cr.t_cases(n)
    assert ref_of(tie)[1:3] == (0, 4) and ref_of(tie)[3].shape[0] == 3 and ref_of(above)[1:3] == (0, 3) and ref_of(above)[3].shape[0] == 2
    for bpc in gc.cg_grids(n):
        options(blocks_per_cu=bpc)
        for c in (tie, above, tie):
            what = "T n=%d bpc=%d %s" % (n, bpc, c.kind)
            _fused(bh, options, H, cons, c, inst.fix, what)
            _separate_and_compact(bh, options, H, cons, c, inst.fix, what)


@pytest.mark.parametrize("n", cr.SIZES)
def test_curvature_threshold(bh, options, cg_handle, n):
    """Family N: atol == pHp_2 ends iteration 2 with negative_curvature, w_1 untouched and gamma NaN in the trace; one ulp below
    the loop runs as usual; atol == pHp_1 ends iteration 1 with w = 0 (the from_g path of the update)."""
    inst = cr.rows_instance("C2", n)
    H, cons = cg_handle("C2", n)
    at2, below2, at1 = cr.n_cases(n)
    assert [ref_of(c)[1:3] for c in (at2, below2, at1)] == [(2, 2), (0, 3), (2, 1)]
    assert np.isnan(ref_of(at2)[3][1, 2]) and not bits(ref_of(at1)[0]).any()
    for bpc in gc.cg_grids(n):
        options(blocks_per_cu=bpc)
        for c in (at2, below2, at1, at2):
            what = "N n=%d bpc=%d %s" % (n, bpc, c.kind)
            _fused(bh, options, H, cons, c, inst.fix, what)
            _separate_and_compact(bh, options, H, cons, c, inst.fix, what)


# ------------------------------------------------------------------------------------------------------------------ family C2n
@pytest.mark.parametrize("n,bpc", [(n, b) for n in cr.SIZES for b in gc.cg_grids(n)])
def test_negative_curvature_step_to_the_boundary(bh, options, n_cu, cg_handle, n, bpc):
    """Family C2n: pHp_2 = -72 lam m < 0, the loop ends iteration 2 with negative_curvature and w = w_1 + gamma p_2, gamma = 2^-4
    from the one bound — at every placement, from w_l and from w_u."""
    inst = cr.rows_instance("C2n", n)
    H, cons = cg_handle("C2n", n)
    options(blocks_per_cu=bpc)
    assert {i for i, _ in cr.rows_placements("C2n", n, n_cu, bpc)} <= set(inst.deciding)
    for c in cr.c2n_cases(n, n_cu, bpc):
        what = "C2n n=%d bpc=%d i=%d from %s (%s)" % (n, bpc, c.index, c.side, c.edge)
        ref = ref_of(c)
        assert ref[1:3] == (2, 2) and ref[3][1, 0] < 0 and ref[3][1, 2] == 2.0 ** -4
        _fused(bh, options, H, cons, c, inst.fix, what)
        _separate_and_compact(bh, options, H, cons, c, inst.fix, what)
