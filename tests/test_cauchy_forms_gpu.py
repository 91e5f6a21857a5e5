"""GPU tests of the host driver of bh_cauchy_step: every launcher behind its dispatcher (bh_cauchy_info forms 0-4, each with the
options that change which kernels a pass launches) on the exact instances of tests/refresh_cases.py, whose step is the same to the
last bit in every form — a launch that moved, a grid, a buffer or a ping-pong index that changed shows as a different bit, a
different active set or a different counter.  Every instance: 6 passes, 5 variables fixed, seed 0; the oracle's step is the same
bits with H*d accumulated in long double (checked where the reference is computed)."""
import functools

import numpy as np
import pytest

import refresh_cases as rc
from _util import relnorm

pytestmark = pytest.mark.gpu

FORM_HD, FORM_ROWSPACE, FORM_ROWSPACE_EQ, FORM_GRAM, FORM_GRAM_EQ = 0, 1, 2, 3, 4
PASSES = 6
GRAM_EQ_INTERVAL = 128          # a and B of form 4 are formed again every 128th pass (include/benlsip_hip.h, "cauchy_gram_eq")
DEFAULTS = {"cauchy_image": 1, "cauchy_image_max_ma": 64, "cauchy_fused": 1, "cauchy_gemm": 1, "cauchy_image_refresh": 0,
            "cauchy_gram": 0, "cauchy_gram_eq": 0, "chol_downdate": 0}


@functools.lru_cache(maxsize=None)
def _instance(rows, n, mA, npass=PASSES):
    """(J, C, mu, A, x, g, xlow, xupp, delta) and the oracle's (step, active set, passes), computed once and read-only."""
    inst = rc.exact_equality_instance(rows, n, 8, npass, mA) if mA else rc.exact_instance(rows, n, 8, npass)
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    ref = rc.oracle_step(J, C, mu, A, x, g, xlow, xupp, delta)
    ref_ld = rc.oracle_step(J, C, mu, A, x, g, xlow, xupp, delta, longdouble=True)
    assert ref[2] == npass and int(ref[1].sum()) == npass - 1
    assert np.array_equal(ref[0], ref_ld[0]) and np.array_equal(ref[1], ref_ld[1]) and ref_ld[2] == npass
    for arr in inst[:2] + inst[3:8] + ref[:2]:
        arr.setflags(write=False)
    return inst, ref


def _hessian(bh, inst, gram=False):
    H = bh.AlHessian(inst[0], inst[1], inst[2])
    if gram:
        H.set_form("gram")
    return H


def _search(bh, H, inst, opts, cons=None):
    """One search under `opts` (every option back at its default afterwards): step, active set, info and the growth of the handle's
    n_hmul and n_jv."""
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    own = cons is None
    try:
        for k, v in opts.items():
            bh.set_option(k, v)
        if own:
            cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
        st0 = H.stats()
        s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
        st1 = H.stats()
        assert bh.cauchy_info(cons) == (info["form"], info["n_launches"])
        fix = np.asarray(cons.fixvars, dtype=bool).copy()
        if own:
            cons.close()
    finally:
        for k in opts:
            bh.set_option(k, DEFAULTS[k])
    return s, fix, info, st1["n_hmul"] - st0["n_hmul"], st1["n_jv"] - st0["n_jv"]


def _check(out, ref, form, d_hmul, d_jv, passes=PASSES, exact=True):
    s, fix, info, hmul, jv = out
    s_ref, fix_ref, _ = ref
    print("form %d, %d passes, %d launches; n_hmul + %d, n_jv + %d; |s - s_ref| / |s_ref| = %.3e"
          % (info["form"], info["n_hmul"], info["n_launches"], hmul, jv, relnorm(s, s_ref)))
    assert info["form"] == form, info
    assert info["n_hmul"] == passes, info
    assert np.array_equal(fix, fix_ref), (np.flatnonzero(fix), np.flatnonzero(fix_ref))
    if exact:
        assert np.array_equal(s, s_ref), relnorm(s, s_ref)
    else:
        assert relnorm(s, s_ref) <= 1e-9, relnorm(s, s_ref)
    assert (hmul, jv) == (d_hmul, d_jv), (hmul, jv, d_hmul, d_jv)


def _reformations(R, passes=PASSES):
    """m of the header: re-formations that ran — pass indices R, 2R, ... below the number of passes."""
    return (passes - 1) // R if R > 0 else 0


# ------------------------------------------------------------------------------------------------------------ form 0
@pytest.mark.parametrize("mA", [0, 3])
def test_form_0_one_sweep_per_breakpoint(bh, mA):
    """cauchy_image = 0: one H*d per pass (n_hmul of the handle grows by the passes), no stand-alone J v."""
    inst, ref = _instance(96, 48 if mA else 40, mA)
    H = _hessian(bh, inst)
    out = _search(bh, H, inst, {"cauchy_image": 0})
    H.close()
    _check(out, ref, FORM_HD, PASSES, 0)


@pytest.mark.parametrize("chol_downdate", [0, 1])
def test_form_0_beyond_the_row_space_limit(bh, chol_downdate):
    """mA = 65: past the 64 rows of the row-space form whatever the options say; the factor follows the active set by a downdate of
    the Gram matrix + the blocked factorisation (0) or by rank-one downdates of the factor (1)."""
    inst, ref = _instance(200, 300, 65)
    H = _hessian(bh, inst)
    out = _search(bh, H, inst, {"chol_downdate": chol_downdate})
    H.close()
    _check(out, ref, FORM_HD, PASSES, 0)


# ------------------------------------------------------------------------------------------------------------ form 1
@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("fused", [1, 0])
def test_form_1_row_space_box(bh, fused, R):
    """One kernel per breakpoint (launch 0, normal launches, launches with a re-formation) and the two-kernel form (with two gated
    J v sweeps per re-formation): n_jv grows by 1 + m, 1 + 2 m; n_hmul by nothing."""
    inst, ref = _instance(96, 40, 0)
    H = _hessian(bh, inst)
    out = _search(bh, H, inst, {"cauchy_fused": fused, "cauchy_image_refresh": R})
    H.close()
    _check(out, ref, FORM_ROWSPACE, 0, 1 + (1 if fused else 2) * _reformations(R))


def test_form_1_several_sweeps_per_workgroup(bh):
    """1100 rows: the row kernels loop, and cauchy_reform_kernel runs more than one workgroup."""
    inst, ref = _instance(1100, 40, 0)
    H = _hessian(bh, inst)
    out = _search(bh, H, inst, {"cauchy_fused": 1, "cauchy_image_refresh": 2})
    H.close()
    _check(out, ref, FORM_ROWSPACE, 0, 1 + _reformations(2))


# ------------------------------------------------------------------------------------------------------------ form 2
@pytest.mark.parametrize("R", [0, 2])
@pytest.mark.parametrize("gemm", [1, 0])
@pytest.mark.parametrize("n,mA", [(48, 3), (120, 20)], ids=["per_thread_rows", "tiled_rows"])
def test_form_2_row_space_with_equalities(bh, n, mA, gemm, R):
    """B by the GEMM or by mA sweeps, the per-thread (mA <= 16) and the tiled row body, with and without re-formations: n_jv grows by
    1 + 2 m or by 1 + mA + (2 + mA) m."""
    inst, ref = _instance(96, n, mA)
    H = _hessian(bh, inst)
    out = _search(bh, H, inst, {"cauchy_gemm": gemm, "cauchy_image_refresh": R})
    H.close()
    m = _reformations(R)
    _check(out, ref, FORM_ROWSPACE_EQ, 0, 1 + 2 * m if gemm else 1 + mA + (2 + mA) * m)


def test_form_2_chosen_from_history(bh):
    """cauchy_image_max_ma = 0, two searches on the same constraint handle (as test_cauchy_step_row_space_form_chosen_from_history):
    the first sweeps, the second — the first having taken more than 4 (1 + mA) passes — runs in the row space.  The rule needs more
    than 16 passes at mA = 3, so this instance alone has 18 instead of 6 (same shape and data otherwise; exact in the same way)."""
    mA, passes = 3, 18
    assert passes > 4 * (1 + mA)
    inst, ref = _instance(96, 48, mA, passes)
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    H = _hessian(bh, inst)
    cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
    first = _search(bh, H, inst, {"cauchy_image_max_ma": 0}, cons=cons)
    second = _search(bh, H, inst, {"cauchy_image_max_ma": 0}, cons=cons)
    cons.close()
    H.close()
    _check(first, ref, FORM_HD, passes, 0, passes)
    _check(second, ref, FORM_ROWSPACE_EQ, 0, 1 + 2 * _reformations(0, passes), passes)


# ------------------------------------------------------------------------------------------------------------ forms 3, 4
def test_form_3_gram_one_launch(bh):
    """Gram handle, cauchy_gram = 1, box: one G d, then the whole search in one launch — the launch count is that of a search of any
    length (below 16, as test_launch_count_does_not_depend_on_the_search_length has it) once G is built."""
    inst, ref = _instance(96, 40, 0)
    H = _hessian(bh, inst, gram=True)
    out = _search(bh, H, inst, {"cauchy_gram": 1})
    again = _search(bh, H, inst, {"cauchy_gram": 1})
    H.close()
    _check(out, ref, FORM_GRAM, 1, 0)
    _check(again, ref, FORM_GRAM, 1, 0)
    assert again[2]["n_launches"] < 16 and again[2]["n_launches"] <= out[2]["n_launches"], (out[2], again[2])


def test_form_4_gram_with_equalities(bh):
    """Gram handle, cauchy_gram_eq = 1, mA = 3: n_hmul grows by the G v launches (pass 0 and every 128th pass), n_jv by nothing."""
    inst, ref = _instance(96, 48, 3)
    H = _hessian(bh, inst, gram=True)
    out = _search(bh, H, inst, {"cauchy_gram_eq": 1})
    H.close()
    _check(out, ref, FORM_GRAM_EQ, 1 + (PASSES - 1) // GRAM_EQ_INTERVAL, 0)
