"""The device steps between two projected_cg calls of the resident minor loop, on the exactly computed cases of minor_cases.py
(proved to be what they claim by test_minor_cases_cpu.py): active_update_kernel, canon_mask_kernel, flags_from_chunks_kernel,
gram_downdate_list_kernel, linesearch_kernel, vec_norm(_masked)_kernel, vec_dot_kernel, vec_add_kernel and the products behind
bh_hmul_add(_dev), bh_step_accumulate_dev (sweep path, "step_from_cg" off), bh_model_reduction_dev, bh_grad(_dev) and
bh_resid_sqnorm.  Every comparison is bit for bit, except

* the projection after an active-set update: the rule of test_device_side_active_set_update_matches_oracle, 1e-10 ||r||;
* bh_reduced_gradient_norm_dev: within 1 ulp of sqrt(S) for the exact sum of squares S (nothing promises a correctly rounded
  device sqrt), exact where S is a perfect square.

Not checked here: step_bounds_kernel writes w_l, w_u only for fixed variables, which never move, so its output cannot be
observed through the ABI; the from-CG path of bh_step_accumulate_dev is not exact by construction and is covered elsewhere.

The projection after an update is also bit-identical to that of a fresh MixedConstraints created on the final fixvars, for every
mA: with integer A the Gram matrix A_free A_free' has the same bits whether it is downdated over the newly fixed columns
(gram_downdate_list_kernel) or summed from the mask (gram_free_kernel, or the matrix-core kernel above mA = 96), and both
routes then run the same launch_chol on it and the same projection kernels on the canonical mask."""
import ctypes as ct
import math

import numpy as np
import pytest

import benlsip_ref as R
import minor_cases as mc
from _util import note_tol

pytestmark = pytest.mark.gpu

ACTIVE = mc.active_cases()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """Bit equality of two float64 values or arrays, any NaN counting as equal to any NaN."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def unpack(chunks, n):
    return np.unpackbits(chunks.view(np.uint8), bitorder="little")[:n].astype(bool)


def update_active(bh, cons, dx, ds, dxl, dxu, delta, n):
    chunks = np.zeros((n + 63) // 64, dtype=np.uint64)
    n_at, n_fix, br = ct.c_int32(-1), ct.c_int32(-1), ct.c_int32(-1)
    bh._lib.check(bh._lib.lib().bh_proj_update_active_dev(cons._h, dx.ptr, ds.ptr, dxl.ptr, dxu.ptr, float(delta), R.SQRT_EPS, ct.byref(n_at),
                                                          ct.byref(n_fix), ct.byref(br), bh._lib.ptr(chunks)), "update_active")
    return n_at.value, n_fix.value, br.value, chunks


def oracle_update(cons_o, L0, x, s, delta):
    """src/basic_tralcnlss.jl:439-453 on the oracle: (n_at_bound, branch)."""
    idx = R.active_bounds(cons_o, x, s, delta)
    if cons_o.lineq.shape[0] + idx.shape[0] <= x.shape[0]:
        R.add_active(cons_o, L0, idx)
        return idx.shape[0], 0
    R.active_bounds_inplace(cons_o, x + s, L0)
    return idx.shape[0], 1


# ------------------------------------------------------------------------------------------------------- active-set update
@pytest.mark.parametrize("case", ACTIVE, ids=repr)
def test_active_set_update_gives_the_oracles_flags(bh, case):
    """bh_proj_update_active_dev twice on one handle (the second update runs on the device-side state): n_at_bound, branch,
    n_fixed and the chunks equal the oracle's (R.active_bounds, then add_active or active_bounds_inplace) and the exactly
    computed ones; where the remaining set is feasible the projection of two integer vectors agrees with the oracle's under
    1e-10 ||r|| and is bit-identical to that of a fresh handle on the final fixvars; where the oracle cannot factor the remaining A_free the call reports the library's rank-deficiency error."""
    n, mA = case.n, case.mA
    L0 = R.chol_lower(case.A @ case.A.T)
    cons_o = R.make_mixed_constraints(case.A, L0, case.fix0 if case.fix0.any() else None, l=case.xlow, u=case.xupp)
    cons = bh.MixedConstraints(case.A, None, case.fix0, l=case.xlow, u=case.xupp)
    dx, dxl, dxu = bh.DeviceVector(n, case.x), bh.DeviceVector(n, case.xlow), bh.DeviceVector(n, case.xupp)
    ds = bh.DeviceVector(n)
    cons._sync()
    rng = np.random.default_rng(n + mA)
    for k, st in enumerate(case.steps):
        ds.upload(st.s)
        if st.error:
            with pytest.raises(np.linalg.LinAlgError):
                oracle_update(cons_o, L0, case.x, st.s, st.delta)
            with pytest.raises(bh._lib.BenlsipHipError, match="positive definite"):
                update_active(bh, cons, dx, ds, dxl, dxu, st.delta, n)
            break
        n_at_o, br_o = oracle_update(cons_o, L0, case.x, st.s, st.delta)
        n_at, n_fix, br, chunks = update_active(bh, cons, dx, ds, dxl, dxu, st.delta, n)
        fix_dev = unpack(chunks, n)
        print("%s step %d: n_at %d (oracle %d, exact %d) branch %d (%d, %d) n_fixed %d (%d)" % (case, k, n_at, n_at_o, st.n_at, br, br_o, st.branch,
                                                                                         n_fix, int(st.fix.sum())))
        assert (n_at, br) == (n_at_o, br_o) == (st.n_at, st.branch)
        assert np.array_equal(fix_dev, cons_o.fixvars) and np.array_equal(fix_dev, st.fix)
        assert np.array_equal(chunks, bh.pack_bitvector(st.fix)[:chunks.shape[0]]) and n_fix == int(st.fix.sum())
        cons._fixvars, cons._dirty = fix_dev, False
        if mA + n_fix <= n and (mA == 0 or n_fix < n - mA):
            fresh = bh.MixedConstraints(case.A, None, st.fix, l=case.xlow, u=case.xupp)
            for _ in range(2):
                r = rng.integers(-9, 10, size=n).astype(np.float64)
                v = bh.projection(cons, r)
                assert same_bits(v, bh.projection(fresh, r)), "projection differs from a fresh handle on the final fixvars"
                err = np.linalg.norm(v - R.projection(cons_o, r))
                note_tol("minor steps: projection after update_active vs oracle (1e-10 ||r||)", err, 1e-10 * np.linalg.norm(r), repr(case))
                assert err <= 1e-10 * np.linalg.norm(r)
            fresh.close()
    cons.close()


MASKS = [(n, 0, name) for n in mc.N_EDGE for name in mc.mask_patterns(n)] + \
        [(n, mA, name) for n, mA in mc.MASK_MA.items() for name in mc.mask_patterns(n) if name != "all_fixed"]


@pytest.mark.parametrize("n,mA,name", MASKS, ids=["n%d-mA%d-%s" % m for m in MASKS])
def test_mask_round_trip(bh, n, mA, name):
    """bh_proj_set_active, then bh_proj_update_active_dev with s = 0, x strictly interior and bounds +-1: the chunks come back bit
    for bit, n_fixed is the popcount, n_at_bound what the oracle's active_bounds reports."""
    pat = mc.mask_patterns(n)[name]
    A = mc.int_matrix(mA, n, 31 * n + mA)
    L0 = R.chol_lower(A @ A.T)
    xl, xu = -np.ones(n), np.ones(n)
    x, s = np.full(n, 0.25), np.zeros(n)
    cons_o = R.make_mixed_constraints(A, L0, None, l=xl, u=xu)          # active_bounds reads only the bounds: no n x n factor
    cons = bh.MixedConstraints(A, None, pat, l=xl, u=xu)
    cons._sync()
    dx, ds, dxl, dxu = (bh.DeviceVector(n, v) for v in (x, s, xl, xu))
    n_at_o = R.active_bounds(cons_o, x, s, 0.5).shape[0]
    n_at, n_fix, br, chunks = update_active(bh, cons, dx, ds, dxl, dxu, 0.5, n)
    want = bh.pack_bitvector(pat)[:chunks.shape[0]]
    assert np.array_equal(chunks, want), np.flatnonzero(chunks != want)[:4]
    assert (n_at, n_fix, br) == (n_at_o, int(pat.sum()), 0)
    cons.close()


# ------------------------------------------------------------------------------------------------------- line search
@pytest.mark.parametrize("n", mc.N_EDGE)
def test_linesearch_is_bit_equal_to_the_literal_oracle(bh, n):
    """bh_linesearch and bh_linesearch_dev on every line-search case that a vector of length n can hold: alpha has the bits of
    src/basic_tralcnlss.jl:776-790 evaluated literally (and of the oracle's R.linesearch); NaN compares as NaN."""
    lib = bh._lib.lib()
    handles = {}
    A = np.zeros((0, n))
    bad = []
    for c in mc.linesearch_cases(n):
        key = id(c.J)
        if key not in handles:
            handles[key] = (bh.AlHessian(c.J, None, 0.0), R.AlHessian(c.J, np.zeros((0, n)), 0.0))
        H, Ho = handles[key]
        with np.errstate(all="ignore"):
            a_o = R.linesearch(c.g, Ho, c.w, c.w_l, c.w_u, c.fix)
        assert same_bits(a_o, c.alpha), (c, a_o, c.alpha)
        cons = bh.MixedConstraints(A, None, c.fix)
        a_host = bh.linesearch(c.g, H, c.w, c.w_l, c.w_u, cons)
        dv = [bh.DeviceVector(n, v) for v in (c.g, c.w, c.w_l, c.w_u)]
        out = ct.c_double(-1.0)
        bh._lib.check(lib.bh_linesearch_dev(H.handle, cons.handle, dv[0].ptr, dv[1].ptr, dv[2].ptr, dv[3].ptr, ct.byref(out)), "linesearch_dev")
        print("%s: expected %r host %r dev %r" % (c, c.alpha, a_host, out.value))
        if not (same_bits(a_host, c.alpha) and same_bits(out.value, c.alpha)):
            bad.append((c.name, c.alpha, a_host, out.value))
        cons.close()
    for H, _ in handles.values():
        H.close()
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- integer vectors
VEC = [(c, form) for c in mc.vector_cases() for form in ("implicit", "gram") if form == "implicit" or c.n <= mc.GRAM_N_MAX]


@pytest.mark.parametrize("c,form", VEC, ids=["%s-%s" % (c, f) for c, f in VEC])
def test_integer_vector_steps_are_bit_exact(bh, c, form):
    """H*s + g (bh_hmul_add, bh_hmul_add_dev), s .+= w; H*s + g (bh_step_accumulate_dev, sweep path), g.s + s'Hs / 2
    (bh_model_reduction_dev) and J'r + C'ybar (bh_grad, bh_grad_dev) on integer operands: the bits of the integer results, on the
    implicit and on the Gram form of the handle."""
    lib, chk = bh._lib.lib(), bh._lib.check
    n = c.n
    H = bh.AlHessian(c.J, c.C if c.q else None, c.mu)
    H.set_form(form)
    assert same_bits(bh.hmul_add(H, c.s, c.g), c.hs_g)
    ds, dw, dg, dt = bh.DeviceVector(n, c.s), bh.DeviceVector(n, c.w), bh.DeviceVector(n, c.g), bh.DeviceVector(n)
    chk(lib.bh_hmul_add_dev(H.handle, ds.ptr, dg.ptr, dt.ptr), "hmul_add_dev")
    assert same_bits(dt.download(), c.hs_g)
    out = ct.c_double(math.nan)
    chk(lib.bh_model_reduction_dev(H.handle, dg.ptr, ds.ptr, ct.byref(out)), "model_reduction_dev")
    assert same_bits(out.value, c.model), (out.value, c.model)
    chk(lib.bh_step_accumulate_dev(H.handle, ds.ptr, dw.ptr, dg.ptr, dt.ptr), "step_accumulate_dev")
    assert same_bits(ds.download(), c.s + c.w) and same_bits(dt.download(), c.hsw_g)
    assert same_bits(bh.gradient(H, c.r, c.ybar), c.grad)
    dr = bh.DeviceVector(c.d, c.r)
    yb = np.ascontiguousarray(c.ybar)
    chk(lib.bh_grad_dev(H.handle, dr.ptr, bh._lib.ptr(yb) if c.q else None, dg.ptr), "grad_dev")
    assert same_bits(dg.download(), c.grad)
    H.close()


@pytest.mark.parametrize("d", [1, 63, 1025, 4100, 16384])
def test_resid_sqnorm_is_exact(bh, d):
    r, S = mc.resid_case(d)
    assert same_bits(bh.resid_sqnorm(r), float(S))


@pytest.mark.parametrize("n", mc.VEC_N)
def test_reduced_gradient_norm_with_box_constraints(bh, n):
    """bh_reduced_gradient_norm_dev with box constraints: the free components are integers with the exact sum of squares S, the
    fixed ones hold 2^40 * odd or one NaN and must not reach the result: within 1 ulp of sqrt(S), exact for a perfect square."""
    lib = bh._lib.lib()
    for c in mc.norm_cases(n):
        cons = bh.MixedConstraints(np.zeros((0, n)), None, c.fix)
        dg = bh.DeviceVector(n, c.g)
        out = ct.c_double(-1.0)
        bh._lib.check(lib.bh_reduced_gradient_norm_dev(cons.handle, dg.ptr, ct.byref(out)), "reduced_gradient_norm_dev")
        want = math.sqrt(c.S)
        print("%s: S %d sqrt %r device %r" % (c, c.S, want, out.value))
        if c.exact:
            assert same_bits(out.value, float(math.isqrt(c.S))), (c, out.value)
        else:
            note_tol("minor steps: reduced gradient norm vs sqrt(S) (1 ulp)", abs(out.value - want), np.spacing(want), repr(c))
            assert abs(out.value - want) <= np.spacing(want), (c, out.value, want)
        cons.close()
