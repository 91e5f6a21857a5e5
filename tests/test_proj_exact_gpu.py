"""The null-space projection kernels of csrc/bh_proj.hip.h on the exactly computed cases of proj_cases.py (proved to be what they
claim by test_proj_cases_cpu.py): proj_left_mul_kernel, proj_left_mul_tr_kernel<*, 4 | 16>, gram_free_kernel, gram_free_mfma_kernel,
chol_small_kernel, copy_lower_kernel, chol_trsm_kernel, chol_syrk_kernel, trsv_small_kernel, trsv_pair_kernel (split 4 and 1),
tri_inv_small_kernel and proj_apply_linv_kernel<INIT | !INIT>.

* bh_left_mul, bh_left_mul_tr: bit-equal to the integer results, on every case and under both projection forms (a reduced-form case
  hands over an identity of the right order under proj_form = 0: the two entry points never read the factor).
* Augmented form: bh_project, bh_project_dev bit-equal to v = r - B'(L L')^-1 B r evaluated exactly for the factor handed over (an
  exact check of gather, blocked substitution and scatter — L L' is not B B', so this is not a projector), NaN in the unread upper
  triangle, factor orders 3 .. 3265 (the last order with the split trailing update and the first with the single slice).
* Reduced form: REDUCED_BIT_EQUAL says what the assertion is.  The expected vector is exact, so no condition number enters: either
  bit equality, or max |v - v_exact| <= tol of the case (64 x what a last-bit error of every reciprocal pivot does to a float64
  restatement; below granularity / 1024 for every case).  Fixed components are exactly 0.0, host and device entry points and a
  second, fresh handle give the same bits.
* One exact CG iteration through every iteration shape (J'J = 16 I: alpha = 1/16, w = -P(g)/16, the second projection vanishes),
  and the active-set sequence F1 -> F2 -> F1 on one handle: the only test that can see a stale explicit inverse W.

Blind spots.  On exact instances the refinement residual rho = t - M y of proj_apply_linv_kernel is exactly zero, so these tests
cannot tell a wrong refinement step from a right one: the ill-conditioned parity tests of test_parity_gpu.py remain its guard.  No
several-rank path is exercised."""
import numpy as np
import pytest

import benlsip_ref as R
import proj_cases as pc
from _util import note_tol

pytestmark = pytest.mark.gpu

# True: every reduced-form cell was bit-equal on the MI355X (v_rsq_f64 of a power of four comes out exact, so chol_small_body's
# reciprocal pivots are exact), and the reduced-form assertions are bit equality.  False: they are `tol` of the case.
REDUCED_BIT_EQUAL = True

DEFAULTS = {"proj_form": 1, "gram_mfma": 1, "cg_fused": 1, "linv_refine": 1, "gram_cg_fused": 0, "chol_downdate": 0}
REDUCED = pc.reduced_cases()
AUGMENTED = pc.augmented_cases()
EVERY = REDUCED + [pc.identity_case()] + pc.sequence_cases()[:2] + AUGMENTED


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def handle(bh, c, form=None):
    """A fresh MixedConstraints on the case (form: the proj_form it will be used under; the case's own by default)."""
    form = c.form if form is None else form
    L = None
    if form == 0:
        L = c.factor_with_nan() if c.form == 0 else np.eye(c.mpp)
    return bh.MixedConstraints(c.A, L, c.fix)


def project_dev(bh, cons, r):
    dr, dv = bh.DeviceVector(cons.n, r), bh.DeviceVector(cons.n)
    bh._lib.check(bh._lib.lib().bh_project_dev(cons.handle, dr.ptr, dv.ptr), "bh_project_dev")
    return dv.download()


def check_reduced(c, v, what):
    """The reduced-form assertion on one projection; returns whether it was bit-equal."""
    dev = float(np.max(np.abs(v - c.v)))
    equal = same_bits(v, c.v)
    share = note_tol("exact projection cases: max |v - v_exact| vs tol of the case", dev, c.tol, "%s %s" % (c, what)) if c.tol > 0 else float(dev > 0)
    print("%s %s: %d of %d entries bit-equal, max deviation %.3e = %.3g of tol %.3e (granularity %g)"
          % (c, what, int(np.sum(bits(v) == bits(c.v))), c.n, dev, share, c.tol, c.granularity))
    assert not np.any(bits(v[c.fix])), "a fixed component is not +0.0"
    if REDUCED_BIT_EQUAL:
        assert equal, (c, what, dev)
    else:
        assert dev <= c.tol, (c, what, dev, c.tol)
    return equal


# ------------------------------------------------------------------------------------------------------- the reciprocal square root
def test_reciprocal_square_root_of_powers_of_four(bh, options):
    """M = diag(4^k) (T = I, mA = 64): chol_small_body's v_rsq_f64 seed plus two Newton steps on exact powers of four.  If the seed is
    exact the factor, its reciprocal diagonal and the projection are exact."""
    c = pc.identity_case()
    options(proj_form=1, gram_mfma=0)
    cons = handle(bh, c)
    v = bh.projection(cons, c.r)
    exact = check_reduced(c, v, "identity")
    print("reciprocal square root of 4^k on this device: %s" % ("EXACT (projection bit-equal)" if exact else "NOT exact (projection within tol)"))
    cons.close()


# ------------------------------------------------------------------------------------------------------- left_mul, left_mul_tr
@pytest.mark.parametrize("form", [1, 0], ids=["reduced_form", "augmented_form"])
@pytest.mark.parametrize("c", EVERY, ids=repr)
def test_left_mul_and_left_mul_tr_are_bit_exact(bh, options, c, form):
    """[A x; x_fix] and A'y_A + scatter(y_fix) on integers, gather blocks and scatter included."""
    options(proj_form=form)
    cons = handle(bh, c, form)
    lm, lmt = bh.left_mul(cons, c.x_lm), bh.left_mul_tr(cons, c.y_lmt)
    cons.close()
    assert same_bits(lm, c.lm), np.flatnonzero(bits(lm) != bits(c.lm))[:8]
    assert same_bits(lmt, c.lmt), np.flatnonzero(bits(lmt) != bits(c.lmt))[:8]


# ------------------------------------------------------------------------------------------------------- augmented form
@pytest.mark.parametrize("c", AUGMENTED, ids=repr)
def test_augmented_form_is_bit_exact(bh, options, c):
    """bh_project and bh_project_dev equal r - B'(L L')^-1 B r, evaluated exactly for the factor handed over, bit for bit; a fresh
    handle repeats the bits.  Not a projector: an exact check of proj_left_mul_kernel's gather, trsv_pair_kernel and the scatter of
    proj_left_mul_tr_kernel."""
    options(proj_form=0)
    first = None
    for k in range(2):
        cons = handle(bh, c)
        v, vd = bh.projection(cons, c.r), project_dev(bh, cons, c.r)
        cons.close()
        bad = np.flatnonzero(bits(v) != bits(c.v))
        assert bad.size == 0, (c, k, bad[:8], v[bad[:8]], c.v[bad[:8]])
        assert same_bits(vd, c.v)
        first = v if first is None else first
    assert same_bits(first, v)


# ------------------------------------------------------------------------------------------------------- reduced form
RED_CELLS = [(c, g) for c in REDUCED for g in c.gram]


@pytest.mark.parametrize("c,gram", RED_CELLS, ids=["%s-mfma%d" % cg for cg in RED_CELLS])
def test_reduced_form_projection(bh, options, c, gram):
    """Gram matrix (VALU kernel or matrix cores), factorisation (one panel or blocked), substitutions and left_mul_tr against the exact
    vector; host and device entry points and a fresh handle give the same bits."""
    options(proj_form=1, gram_mfma=gram)
    cons = handle(bh, c)
    v, vd = bh.projection(cons, c.r), project_dev(bh, cons, c.r)
    cons.close()
    check_reduced(c, v, "mfma%d" % gram)
    assert same_bits(v, vd), "bh_project and bh_project_dev differ"
    cons = handle(bh, c)
    v2 = bh.projection(cons, c.r)
    cons.close()
    assert same_bits(v, v2), "a fresh handle gives other bits"


def test_rank_deficiency_is_reported_under_the_matrix_core_gram_kernel(bh, options):
    """mA = 40, A_free = T Q with row 32 of Q supported on fixed columns only: the pivot of column 33 is an exact zero whichever kernel
    sums the Gram matrix."""
    c = pc.rank_deficient_case()
    assert c.D[32] == 0 and np.all(c.D[:32] > 0)                 # T D T' has the exact pivots a^2 D: column 33 is the first zero
    for gram in (2, 0):
        options(proj_form=1, gram_mfma=gram)
        cons = bh.MixedConstraints(c.A, None, c.fix)
        with pytest.raises(bh.BenlsipHipError) as e:
            bh.projection(cons, c.r)
        assert e.value.code == -5 and "positive definite" in str(e.value)
        cons.close()


# ------------------------------------------------------------------------------------------------------- one exact CG iteration
_ORACLE = {}


def cg_oracle(c):
    """(status, iters, gamma of trace row 0) of the oracle's projected_cg on the case."""
    if c.name not in _ORACLE:
        n = c.n
        cons = R.make_mixed_constraints(c.A, R.chol_lower(c.A @ c.A.T), c.fix)
        tr = R.CGTrace()
        inf = np.full(n, np.inf)
        _, st, it = R.projected_cg(c.r, R.AlHessian(pc.cg_jacobian(n), np.zeros((0, n)), 1.0), -inf, inf, cons, 0.1, trace=tr)
        assert tr.n_hmul == 1
        _ORACLE[c.name] = (int(st), int(it), tr.rows[0][2])
    return _ORACLE[c.name]


def check_cg(bh, c, H, cons, what):
    """One projected_cg on the case: one product, the oracle's status and iters, trace row 0 = {16 ||v||^2, 1/16, gamma, 0}, w = -v/16."""
    n = c.n
    inf = np.full(n, np.inf)
    w, st, info = bh.projected_cg(c.r, H, -inf, inf, cons, 0.1, trace_cap=4, full_output=True)
    st_o, it_o, gamma_o = cg_oracle(c)
    vv = float(c.v @ c.v)
    row = info["trace"][0]
    w_exact = 0.0 - c.v / pc.CG_C                                # w = 0 + alpha p: +0.0 where v is zero
    dev = float(np.max(np.abs(w - w_exact)))
    print("%s %s: status %d iters %d n_hmul %d trace %r, max |w + v/16| = %.3e (tol/16 = %.3e), %d of %d entries bit-equal"
          % (c, what, int(st), info["iters"], info["n_hmul"], row.tolist(), dev, c.tol / pc.CG_C, int(np.sum(bits(w) == bits(w_exact))), n))
    assert info["n_hmul"] == 1 and (int(st), info["iters"]) == (st_o, it_o)
    assert row[2] == gamma_o or (np.isinf(row[2]) and np.isinf(gamma_o))
    if c.tol > 0:
        note_tol("exact CG iteration: max |w + v/16| vs tol/16 of the case", dev, c.tol / pc.CG_C, "%s %s" % (c, what))
    if REDUCED_BIT_EQUAL:
        assert same_bits(w, w_exact) and same_bits(row[[0, 1, 3]], [pc.CG_C * vv, 1.0 / pc.CG_C, 0.0]), (c, what, row)
    else:
        s1 = float(np.sum(np.abs(c.v)) + np.sum(np.abs(c.r)))
        assert dev <= c.tol / pc.CG_C
        assert abs(row[0] - pc.CG_C * vv) <= pc.CG_C * 4.0 * c.tol * s1 and abs(row[1] - 1.0 / pc.CG_C) <= 4.0 * c.tol * s1 / vv
        assert abs(row[3]) <= 4.0 * c.tol * s1


CG_CELLS = [(mA, n, f, rf) for mA in (1, 16, 17, 33, 64) for n in pc.CG_N for f in (0, 1, 2) for rf in (0, 1)] + \
           [(65, n, f, 1) for n in pc.CG_N for f in (0, 1)]


@pytest.mark.parametrize("mA,n,fused,refine", CG_CELLS, ids=["mA%d-n%d-fused%d-refine%d" % x for x in CG_CELLS])
def test_one_exact_cg_iteration(bh, options, mA, n, fused, refine):
    """Seven-, four- and three-kernel iteration (cg_fused 0 / 2 / 1), with and without the refinement step of the explicit inverse, at
    n = 203 (g copied into the padded workspace) and n = 208 (g read in place); mA = 65 takes the separate-kernel shape and the
    blocked factor whatever cg_fused says."""
    c = pc.cg_case(mA, n)
    options(proj_form=1, cg_fused=fused, linv_refine=refine)
    H = bh.AlHessian(pc.cg_jacobian(n), None, 1.0)
    cons = handle(bh, c)
    try:
        check_cg(bh, c, H, cons, "cg_fused=%d linv_refine=%d" % (fused, refine))
    finally:
        cons.close()
        H.close()


@pytest.mark.parametrize("mA,n", [(mA, n) for mA in (17, 64) for n in pc.CG_N])
def test_one_exact_cg_iteration_on_a_gram_form_handle(bh, options, mA, n):
    c = pc.cg_case(mA, n)
    options(proj_form=1, gram_cg_fused=1)
    H = bh.AlHessian(pc.cg_jacobian(n), None, 1.0)
    H.set_form("gram")
    cons = handle(bh, c)
    try:
        check_cg(bh, c, H, cons, "gram_cg_fused=1")
    finally:
        cons.close()
        H.close()


def test_active_set_sequence_on_one_handle(bh, options):
    """F1 -> F2 -> F1 by set_active on ONE handle, with the three-kernel iteration (cg_fused = 1: the explicit inverse W is cached
    under linv_valid): every projection and every CG run gives that set's own answer.  Every row of A_free changes its norm 64 -> 16
    between the sets, so a stale factor or a stale W gives the other set's vector."""
    seq = pc.sequence_cases()
    options(proj_form=1, cg_fused=1)
    n = seq[0].n
    H = bh.AlHessian(pc.cg_jacobian(n), None, 1.0)
    cons = bh.MixedConstraints(seq[0].A, None, seq[0].fix)
    try:
        for k, c in enumerate(seq):
            cons.set_active(c.fix, None)
            check_cg(bh, c, H, cons, "sequence step %d" % k)
            check_reduced(c, bh.projection(cons, c.r), "sequence step %d" % k)
            other = seq[1 - (k % 2)]
            assert np.max(np.abs(c.v - other.v)) >= c.granularity
    finally:
        cons.close()
        H.close()
