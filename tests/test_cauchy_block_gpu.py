"""GPU tests of option cauchy_block = K: the one-kernel row-space Cauchy search (bh_cauchy_info form 1) takes K breakpoints per launch
(cauchy_block_kernel<K>, csrc/bh_cauchyblock.hip.h).  Every row performs the operations of the one-breakpoint-per-launch form in its
order and every partial sum is reduced over the same grid in the same order, so everything here is compared bit for bit with option
0 on the same handle — no tolerance anywhere.  Instances and the CPU model of the launch structure: tests/block_cases.py."""
import functools

import numpy as np
import pytest

import block_cases as bc
import refresh_cases as rc
from _util import closed_form_cauchy_cases
from hip_ops import HipOpsResident
import benlsip_ref as R

pytestmark = pytest.mark.gpu

FORM_ROWSPACE, FORM_GRAM = 1, 3
FIRST, BATCH = 4, 4                       # the blocked search's launch-ahead schedule (cauchy_make_plan)
ERR_INVALID_ARG = -1


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _search(bh, H, inst, K, cons=None, options=()):
    """One search with cauchy_block = K (and `options` set for its duration); everything is back at its default afterwards.
    inst = (J, C, mu, x, g, xlow, xupp, delta).  Returns the step, the active set and bh_cauchy_step's info with the growth of the
    handle's n_jv and n_hmul."""
    J, C, mu, x, g, xlow, xupp, delta = inst
    defaults = {"cauchy_fused": 1, "cauchy_image_refresh": 0, "cauchy_gram": 0}
    bh.set_option("cauchy_block", K)
    for key, value in options:
        bh.set_option(key, value)
    own = cons is None
    try:
        if own:
            cons = bh.MixedConstraints(np.zeros((0, J.shape[1])), None, None, l=xlow, u=xupp)
        st0 = H.stats()
        s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
        st1 = H.stats()
        info["n_jv"] = st1["n_jv"] - st0["n_jv"]
        info["H_n_hmul"] = st1["n_hmul"] - st0["n_hmul"]
        fix = np.asarray(cons.fixvars, dtype=bool).copy()
    finally:
        if own and cons is not None:
            cons.close()
        bh.set_option("cauchy_block", 0)
        for key, _ in options:
            bh.set_option(key, defaults[key])
    return s, fix, info


def _same(a, b, launches=False):
    """Step (as uint64), active set, breakpoints, passes, the handle's counters and the form of two searches."""
    (s1, f1, i1), (s0, f0, i0) = a, b
    assert np.array_equal(_bits(s1), _bits(s0)), float(np.max(np.abs(s1 - s0)))
    assert np.array_equal(f1, f0)
    keys = ["n_breakpoints", "n_hmul", "n_jv", "H_n_hmul", "form"] + (["n_launches"] if launches else [])
    assert [i1[k] for k in keys] == [i0[k] for k in keys], (i1, i0)


@functools.lru_cache(maxsize=None)
def _exact(rows, n, q, npass):
    """An exact instance and the oracle's step on it, computed once and shared (read-only)."""
    inst = bc.exact(rows, n, q, npass)
    J, C, mu, x, g, xlow, xupp, delta = inst
    ref = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
    for arr in (J, C, x, g, xlow, xupp) + ref[:2]:
        arr.setflags(write=False)
    return inst, ref


def _hessian(bh, inst):
    J, C, mu = inst[:3]
    return bh.AlHessian(J, C if (C is not None and C.shape[0]) else None, mu)


# ------------------------------------------------------------------------------------------------------------ 1. the option
def test_option_is_accepted_checked_and_keeps_its_value(bh):
    """Fails without the feature (unknown option).  0, 1, 2, 4, 8, 16 are accepted; 3, 32 and -1 are BH_ERR_INVALID_ARG and leave the
    option as it was: the library has no getter, so the value is read back by its effect — after the three refusals a 40-pass search
    still runs with the launch count of K = 4, which is below that of K = 0."""
    lib = bh._lib.lib()
    inst, (s_ref, fix_ref, passes) = _exact(40, 48, 3, 40)
    H = _hessian(bh, inst)
    try:
        for v in (0, 1, 2, 4, 8, 16):
            assert lib.bh_set_option(b"cauchy_block", v) == 0
        r4 = _search(bh, H, inst, 4)
        r0 = _search(bh, H, inst, 0)
        assert lib.bh_set_option(b"cauchy_block", 4) == 0
        for v in (3, 32, -1):
            assert lib.bh_set_option(b"cauchy_block", v) == ERR_INVALID_ARG
        J, C, mu, x, g, xlow, xupp, delta = inst
        cons = bh.MixedConstraints(np.zeros((0, 48)), None, None, l=xlow, u=xupp)
        s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
        cons.close()
    finally:
        assert lib.bh_set_option(b"cauchy_block", 0) == 0
        H.close()
    assert np.array_equal(_bits(s), _bits(r4[0])) and info["n_hmul"] == passes
    assert info["n_launches"] < r0[2]["n_launches"] - 10
    assert abs(info["n_launches"] - r4[2]["n_launches"]) <= FIRST + BATCH     # (the units past the end depend on when the host looks)


# ------------------------------------------------------------------------------------------------------------ 2. bit for bit
@pytest.mark.parametrize("K", bc.KS)
def test_exact_instances_every_ending_offset(bh, K):
    """refresh_cases.exact_instance (40 rows of which 3 weighted, n = 48) for every search length of block_cases.NPASS: step, active
    set, breakpoints, passes, n_jv (+ 1) and the handle's n_hmul (+ 0) equal option 0's, form 1; the step is the oracle's to the
    last bit; 1 is the same path as 0, launches included up to the units past the end."""
    for npass in bc.NPASS:
        inst, (s_ref, fix_ref, passes) = _exact(40, 48, 3, npass)
        assert passes == npass
        H = _hessian(bh, inst)
        r0 = _search(bh, H, inst, 0)
        rk = _search(bh, H, inst, K)
        r1 = _search(bh, H, inst, 1)
        H.close()
        _same(rk, r0)
        _same(r1, r0)
        assert rk[2]["form"] == FORM_ROWSPACE and rk[2]["n_jv"] == 1 and rk[2]["H_n_hmul"] == 0
        assert rk[2]["n_hmul"] == npass and rk[2]["n_breakpoints"] == npass - 1
        assert np.array_equal(rk[0], s_ref) and np.array_equal(rk[1], fix_ref), (K, npass)


@pytest.mark.parametrize("K", bc.KS)
@pytest.mark.parametrize("name,inst", list(bc.named_cases()), ids=[n for n, _ in bc.named_cases()])
def test_edges_of_the_search(bh, name, inst, K):
    """Non-dyadic data with 120 breakpoints ending inside a segment, every variable fixed (nfix == nmm), phi' >= 0 at pass 0, two equal
    thetas inside one block: the bits of option 0."""
    H = _hessian(bh, inst)
    r0 = _search(bh, H, inst, 0)
    rk = _search(bh, H, inst, K)
    H.close()
    _same(rk, r0)
    n = inst[0].shape[1]
    if name.startswith("all_fixed"):
        assert rk[2]["n_hmul"] == n + 1 and rk[1].all()
    if name == "stationary_at_pass_0":
        assert rk[2]["n_hmul"] == 1 and not rk[1].any() and not rk[0].any()
    if name == "bad_instance_d300":
        assert rk[2]["n_hmul"] == 121
    if name == "tie_in_block":
        s_ref, fix_ref, passes = rc.oracle_step(inst[0], inst[1], inst[2], None, *inst[3:])
        assert np.array_equal(rk[0], s_ref) and np.array_equal(rk[1], fix_ref) and rk[2]["n_hmul"] == passes == 9


@pytest.mark.parametrize("K", bc.KS)
def test_no_breakpoint_left_is_the_same_error(bh, K):
    """J = 0, infinite bounds and trust region: pass 0 finds no breakpoint — the same error code as option 0, and the call returns."""
    inst = bc.no_breakpoint()
    H = _hessian(bh, inst)
    codes = []
    for k in (0, K):
        try:
            _search(bh, H, inst, k)
            codes.append(0)
        except bh.BenlsipHipError as e:
            codes.append(e.code)
    H.close()
    assert codes[0] == codes[1] != 0, codes


@pytest.mark.parametrize("K", bc.KS)
def test_closed_form_cases_to_the_last_bit(bh, K):
    """_util.closed_form_cauchy_cases (H = I in two variables, dyadic data, incl. the exact tie dt == theta): the hand-derived step,
    active set and number of passes."""
    for case in closed_form_cauchy_cases():
        inst = (np.eye(2), None, 0.0, np.zeros(2), case["g"], -np.ones(2), np.ones(2), case["delta"])
        H = _hessian(bh, inst)
        s, fix, info = _search(bh, H, inst, K)
        H.close()
        assert info["form"] == FORM_ROWSPACE, (case["name"], info)
        assert np.array_equal(_bits(s), _bits(case["s"])), (case["name"], s)
        assert np.array_equal(fix, case["fix"]) and info["n_hmul"] == case["n_hmul"], (case["name"], fix, info)


# ------------------------------------------------------------------------------------------------------------ 3. shapes
def _shape_case(bh, rows, n, q, npass):
    inst, (s_ref, fix_ref, passes) = _exact(rows, n, q, npass)
    H = _hessian(bh, inst)
    r0 = _search(bh, H, inst, 0)
    assert r0[2]["n_hmul"] == passes
    for K in bc.KS:
        rk = _search(bh, H, inst, K)
        _same(rk, r0)
        assert np.array_equal(rk[0], s_ref) and np.array_equal(rk[1], fix_ref), (rows, n, q, K)
    H.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 4095, 4096])
def test_prologue_widths(bh, n):
    """96 rows; n around the wave, the workgroup and the 8 x 512 register-resident limit (clamped loads, idle lanes, owners of the
    64-element groups of s_c); searches of min(n, 10) + 1 passes: they end inside a block for every K."""
    _shape_case(bh, 96, n, 0, min(n, 10) + 1)


@pytest.mark.parametrize("rows", [1, 511, 512, 513, 1100])
def test_row_count_edges(bh, rows):
    """n = 24, the last 8 rows weighted by mu (a single row: none), so the weighted rows straddle a thread range; one workgroup with a
    tail, exactly one, two, three with a tail."""
    _shape_case(bh, rows, 24, min(8, rows - 1), 11)


def test_grid_stride_row_loop(bh):
    """131072 + 700 rows: more than 256 workgroups x 512 rows, so the row loop takes a second trip for the first 700 rows."""
    _shape_case(bh, 131072 + 700, 24, 8, 11)


# ------------------------------------------------------------------------------------------------------------ 4. launches
def test_launch_count(bh):
    """The 40-pass instance: bh_cauchy_info's n_launches <= the launches outside the passes + ceil((passes - 1) / K) + first + batch,
    and strictly below option 0's for K >= 4.  The launches outside the passes (init, J v, launch 0's row kernel, the renumbering
    behind the search) are measured on a search of the same shape whose unit count is fixed by max_units: all 48 variables end on
    their bounds, n + 1 passes, n + 2 units with option 0 whenever the host looks."""
    allf = bc.all_fixed(48, 40)
    H = _hessian(bh, allf)
    ra = _search(bh, H, allf, 0)
    H.close()
    assert ra[2]["n_hmul"] == 49
    outside = ra[2]["n_launches"] - 49
    inst, (s_ref, fix_ref, passes) = _exact(40, 48, 3, 40)
    H = _hessian(bh, inst)
    n0 = _search(bh, H, inst, 0)[2]["n_launches"]
    assert n0 >= outside + passes
    for K in bc.KS:
        nk = _search(bh, H, inst, K)[2]["n_launches"]
        print("K=%d: %d launches (option 0: %d, outside the passes: %d)" % (K, nk, n0, outside))
        assert outside + 1 + -(-(passes - 1) // K) <= nk <= outside + -(-(passes - 1) // K) + FIRST + BATCH, (K, nk, outside)
        if K >= 4:
            assert nk < n0
    H.close()


# ------------------------------------------------------------------------------------------------------------ 5. fall-backs
def test_fall_backs_take_the_path_of_option_0(bh):
    """n = 4097, three linear equalities, cauchy_fused = 0, cauchy_image_refresh = 2 and a Gram-form handle with cauchy_gram = 1: the
    same form, the same n_launches and the same bits as cauchy_block = 0.  (These paths run their launch-ahead schedule in lock
    step: the launch count does not depend on when the host looks.)"""
    K = 8
    # n = 4097: the register-resident prologue does not hold it
    inst, _ = _exact(11, 4097, 0, 3)
    H = _hessian(bh, inst)
    _same(_search(bh, H, inst, K), _search(bh, H, inst, 0), launches=True)
    H.close()
    allf = bc.all_fixed(6)
    J, C, mu, x, g, xlow, xupp, delta = allf
    H = _hessian(bh, allf)
    for options in ((("cauchy_fused", 0),), (("cauchy_image_refresh", 2),)):
        rk, r0 = _search(bh, H, allf, K, options=options), _search(bh, H, allf, 0, options=options)
        _same(rk, r0, launches=True)
        assert rk[2]["form"] == FORM_ROWSPACE
    H.close()
    # mA = 3 (refresh_cases.exact_instance with a dense A in {-1, 0, 1})
    J, C, mu, A, x, g, xlow, xupp, delta = rc.exact_instance(40, 48, 3, 9, mA=3)
    H = bh.AlHessian(J, C, mu)
    out = []
    for k in (K, 0):
        bh.set_option("cauchy_block", k)
        try:
            cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
            s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
            out.append((s, np.asarray(cons.fixvars, dtype=bool).copy(), info))
            cons.close()
        finally:
            bh.set_option("cauchy_block", 0)
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2]["form"] == out[1][2]["form"] == 2 and out[0][2]["n_hmul"] == out[1][2]["n_hmul"]
    assert out[0][2]["n_launches"] == out[1][2]["n_launches"]
    H.close()
    # a Gram-form handle with cauchy_gram = 1: one launch whatever the option
    H = _hessian(bh, allf)
    H.set_form("gram")
    _search(bh, H, allf, 0, options=(("cauchy_gram", 1),))               # (the first search on the handle also builds G)
    rk, r0 = _search(bh, H, allf, K, options=(("cauchy_gram", 1),)), _search(bh, H, allf, 0, options=(("cauchy_gram", 1),))
    H.close()
    assert rk[2]["form"] == r0[2]["form"] == FORM_GRAM and rk[2]["n_launches"] == r0[2]["n_launches"]
    assert np.array_equal(_bits(rk[0]), _bits(r0[0])) and np.array_equal(rk[1], r0[1]) and rk[2]["n_hmul"] == r0[2]["n_hmul"]


# ------------------------------------------------------------------------------------------------------------ 6. state hygiene
def test_back_to_back_and_repeated_searches(bh):
    """K = 16 then K = 2 on one handle pair, each equal to option 0; a repeated search is bit-identical."""
    inst, (s_ref, fix_ref, passes) = _exact(40, 48, 3, 18)
    H = _hessian(bh, inst)
    r0 = _search(bh, H, inst, 0)
    cons = bh.MixedConstraints(np.zeros((0, 48)), None, None, l=inst[5], u=inst[6])
    for K in (16, 2, 2, 16):
        cons.fixvars = np.zeros(48, dtype=bool)
        _same(_search(bh, H, inst, K, cons=cons), r0)
    cons.close()
    H.close()


@pytest.mark.parametrize("K", [4, 16])
def test_no_speculative_mark_reaches_the_active_set(bh, K):
    """A search of 18 passes ends inside a block (offset 1): the advances run ahead of it were thrown away.  The active set
    bh_cauchy_step reports and a following bh_pcg_dev on that bh_proj (device-side mask as the search left it) equal those after an
    option-0 search bit for bit."""
    inst, (s_ref, fix_ref, passes) = _exact(40, 48, 3, 18)
    J, C, mu, x, g, xlow, xupp, delta = inst
    H = _hessian(bh, inst)
    res = []
    for k in (0, K):
        cons = bh.MixedConstraints(np.zeros((0, 48)), None, None, l=xlow, u=xupp)
        s, fix, info = _search(bh, H, inst, k, cons=cons)
        gd, wl, wu, w = (bh.DeviceVector(48, g), bh.DeviceVector(48, np.where(fix, 0.0, -1.0)), bh.DeviceVector(48, np.where(fix, 0.0, 1.0)),
                         bh.DeviceVector(48))
        st = bh.projected_cg_dev(gd, H, wl, wu, cons, 0.1, w)
        res.append((fix, int(fix.sum()), w.download(), st))
        for v in (gd, wl, wu, w):
            v.close()
        cons.close()
    H.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][0], fix_ref) and res[0][1] == 17
    assert np.array_equal(_bits(res[0][2]), _bits(res[1][2])) and res[0][3] == res[1][3], (res[0][3], res[1][3])
    assert not np.any(res[1][2][fix_ref])


def test_inner_step_with_the_device_search(bh):
    """bh.inner_step (the device-resident chain: bh_cauchy_step_dev, minor iterates) with the option on and off: the same s to the
    last bit, the same decisions."""
    d, n = 4096, 512
    J = R.synthetic_J(d, n, seed=1)
    inst = R.synthetic_box_vectors(d, n, fix_every=8)
    A = np.zeros((0, n))
    L0 = R.chol_lower(A @ A.T)
    x = np.clip(inst.x, inst.x_l, inst.x_u)
    g = J.T @ inst.r0
    delta = R.initial_tr(g)

    def run(K):
        ops = HipOpsResident(bh)
        cons = R.make_mixed_constraints(A, L0, l=inst.x_l, u=inst.x_u)
        H = ops.new_hessian(J, np.zeros((0, n)), 10.0)
        log = []
        bh.set_option("cauchy_block", K)
        try:
            s, pred = ops.inner_step(x, g, H, L0, cons, delta, 50, 0.1, 0.1, log)
            form = bh.cauchy_info(cons._dev)[0]
        finally:
            bh.set_option("cauchy_block", 0)
        H.close()
        return s, pred, log, cons.fixvars.copy(), form

    s0, pred0, log0, fix0, form0 = run(0)
    for K in (4, 16):
        s, pred, log, fix, form = run(K)
        assert form == form0 == FORM_ROWSPACE
        assert np.array_equal(_bits(s), _bits(s0)) and pred == pred0 and np.array_equal(fix, fix0)
        assert log == log0
