"""GPU tests of option cauchy_image_refresh = R: the row-space Cauchy search (bh_cauchy_info forms 1 and 2) forms its carried images
again from J at every pass index that is a positive multiple of R — one kernel per breakpoint: a decision-only launch of
cauchy_fused_kernel + cauchy_reform_kernel (J d and J s_c in one sweep); two-kernel form: two gated J v sweeps; with equalities: a, B
and J s_c.  Instances and the CPU restatement: tests/refresh_cases.py; the conditions the bounds rest on: test_cauchy_refresh_cpu.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import refresh_cases as rc
from _util import note_tol, relnorm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_ROWSPACE, FORM_ROWSPACE_EQ = 1, 2


def _search(bh, H, A, xlow, xupp, x, g, delta, R, fused=1, gemm=1, cons=None):
    """One search with cauchy_image_refresh = R; the options are back at their defaults afterwards.  Returns the step, the active
    set, bh_cauchy_step's info and the growth of the handle's n_jv."""
    bh.set_option("cauchy_image_refresh", R)
    bh.set_option("cauchy_fused", fused)
    bh.set_option("cauchy_gemm", gemm)
    own = cons is None
    try:
        if own:
            cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
        jv0 = H.stats()["n_jv"]
        s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
        info["n_jv"] = H.stats()["n_jv"] - jv0
        fix = np.asarray(cons.fixvars, dtype=bool).copy()
        if own:
            cons.close()
    finally:
        bh.set_option("cauchy_image_refresh", 0)
        bh.set_option("cauchy_fused", 1)
        bh.set_option("cauchy_gemm", 1)
    return s, fix, info


def _n_jv(passes, R, fused, mA=0, gemm=1):
    """The header's formula: sweeps over J of one search."""
    m = (passes - 1) // R if R > 0 else 0
    if mA == 0:
        return 1 + (m if fused else 2 * m)
    return 1 + 2 * m if gemm else 1 + mA + (2 + mA) * m


# ------------------------------------------------------------------------------------------------------------ 1. the option exists
def test_option_is_accepted_checked_and_takes_effect(bh):
    """Fails without the feature: 16 is accepted, -1 is BH_ERR_INVALID_ARG; the library has no getter, so the value is read back by
    its effect — a 5-pass search with R = 2 counts 1 + 2 sweeps over J, with R = 0 one."""
    lib = bh._lib.lib()
    try:
        assert lib.bh_set_option(b"cauchy_image_refresh", 16) == 0
        assert lib.bh_set_option(b"cauchy_image_refresh", -1) == -1
    finally:
        assert lib.bh_set_option(b"cauchy_image_refresh", 0) == 0
    J, C, mu, A, x, g, xlow, xupp, delta = rc.exact_instance(5, 7, 0, 5)
    H = bh.AlHessian(J, None, mu)
    assert _search(bh, H, A, xlow, xupp, x, g, delta, 2)[2]["n_jv"] == 3
    assert _search(bh, H, A, xlow, xupp, x, g, delta, 0)[2]["n_jv"] == 1
    H.close()


# ------------------------------------------------------------------------------------------------------------ 2. exact logic
@functools.lru_cache(maxsize=None)
def _exact(rows, n, q, npass, mA=0):
    inst = rc.exact_instance(rows, n, q, npass, mA=mA)
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    ref = rc.oracle_step(J, C, mu, A, x, g, xlow, xupp, delta)
    for arr in inst[:2] + inst[3:8] + ref[:2]:
        arr.setflags(write=False)
    return inst, ref


# rows = d + q, n, q, passes: n = 7 / 192 / 4100 (the prologue's loop beyond 4096 elements, another J v geometry), 5 rows / 1100 rows
# (more than one workgroup, a row tail), q = 0 / 3 with mu = 1/2; 33 = 2 * 16 + 1 passes, 32 and 16: searches that end at a multiple of R
EXACT_BOX = [(5, 7, 0, 5), (5, 7, 3, 3), (1100, 192, 3, 33), (5, 192, 0, 33), (1100, 4100, 3, 33), (5, 4100, 0, 32), (1100, 192, 0, 17),
             (1100, 192, 3, 16)]
# ... and a cheap case in each geometry of cauchy_reform_kernel the list above does not reach (it runs <64,1,8>, <256,1,8> and
# <512,8,2>): n = 1000 <256,2,8>, 2000 <256,4,4>, 4096 <256,8,4> (the config-3 geometry), 8200 <512,16,1> with d parked in LDS;
# 11 rows: three row groups at R = 4, a row tail at R = 8, 4 and 2
EXACT_GEOMETRIES = [(11, 1000, 0, 6), (11, 2000, 3, 6), (11, 4096, 0, 6), (11, 8200, 3, 6)]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("rows,n,q,npass", EXACT_BOX + EXACT_GEOMETRIES)
def test_exact_box_search_is_bit_identical_for_every_interval(bh, rows, n, q, npass, fused):
    """Dyadic data, every product and sum exact: for R in {1, 2, 5, 16} the step is bit for bit the step of R = 0 and of the oracle,
    passes, breakpoints and active set too; n_jv follows the header's formula; a repeat on the same constraint handle (launch
    batches then over-launch re-formations past the end: gated) is bit-identical; bh_cauchy_info's form stays 1."""
    (J, C, mu, A, x, g, xlow, xupp, delta), (s_ref, fix_ref, passes) = _exact(rows, n, q, npass)
    assert passes == npass
    H = bh.AlHessian(J, C if q else None, mu)
    s0, fix0, info0 = _search(bh, H, A, xlow, xupp, x, g, delta, 0, fused)
    assert np.array_equal(s0, s_ref) and np.array_equal(fix0, fix_ref) and info0["n_hmul"] == passes and info0["n_jv"] == 1
    for R in (1, 2, 5, 16):
        cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
        for rep in range(2):
            s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, R, fused, cons=cons)
            assert np.array_equal(s, s_ref), (R, rep, relnorm(s, s_ref))
            assert np.array_equal(fix, fix_ref), (R, rep)
            assert info["n_hmul"] == passes and info["n_breakpoints"] == info0["n_breakpoints"] == passes - 1, (R, rep, info)
            assert info["form"] == FORM_ROWSPACE == info0["form"]
            assert info["n_jv"] == _n_jv(passes, R, fused), (R, rep, info, passes)
        cons.close()
    H.close()


@pytest.mark.parametrize("R,passes", [(4, 4), (4, 5), (4, 9), (16, 16), (16, 17), (16, 33)])
@pytest.mark.parametrize("fused", [1, 0])
def test_counter_at_the_edges_of_the_interval(bh, R, passes, fused):
    """passes in {R, R + 1, 2R + 1}: a search of R passes ran no re-formation (the one enqueued at index R is gated), R + 1 one,
    2R + 1 two."""
    (J, C, mu, A, x, g, xlow, xupp, delta), (s_ref, fix_ref, p) = _exact(1100, 192, 3, passes)
    assert p == passes
    H = bh.AlHessian(J, C, mu)
    s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, R, fused)
    H.close()
    assert np.array_equal(s, s_ref) and np.array_equal(fix, fix_ref) and info["n_hmul"] == passes
    assert info["n_jv"] == 1 + ((passes - 1) // R) * (1 if fused else 2), info


@functools.lru_cache(maxsize=None)
def _exact_eq(rows, mA, per_row):
    inst = rc.exact_equality_instance(rows, 192, 3, 40, mA, per_row)
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    ref = rc.oracle_step(J, C, mu, A, x, g, xlow, xupp, delta)
    for arr in inst[:2] + inst[3:8] + ref[:2]:
        arr.setflags(write=False)
    return inst, ref


# rows, mA, entries per row of A, B by the GEMM: per-thread row body (mA = 1, 3) and tiled body (mA = 17), 5 / 1100 rows, both forms of B
@pytest.mark.parametrize("rows,mA,per_row,gemm", [(1100, 1, 16, 1), (5, 3, 4, 1), (1100, 3, 16, 0), (1100, 17, 4, 1), (5, 17, 4, 0)])
def test_exact_equality_search_is_bit_identical_for_every_interval(bh, rows, mA, per_row, gemm):
    """Linear equalities whose projector stays dyadic (refresh_cases.exact_equality_instance: A_free A_free' = 4^k I throughout): y,
    d, a, B, t_d = -a - B y, t_s and both sums are exact, so for R in {1, 2, 5, 16} the step is bit for bit the step of R = 0 and of
    the oracle — a `fresh` row body, a re-formed a, B or t_s that is off in any bit fails; passes, breakpoints, active set identical;
    n_jv by the header's formula; the repeat on the same handle (re-formations over-launched past the end: gated) bit-identical."""
    (J, C, mu, A, x, g, xlow, xupp, delta), (s_ref, fix_ref, passes) = _exact_eq(rows, mA, per_row)
    assert passes == 40
    H = bh.AlHessian(J, C, mu)
    s0, fix0, info0 = _search(bh, H, A, xlow, xupp, x, g, delta, 0, 1, gemm)
    assert info0["form"] == FORM_ROWSPACE_EQ and info0["n_hmul"] == passes and np.array_equal(fix0, fix_ref)
    assert np.array_equal(s0, s_ref), relnorm(s0, s_ref)
    assert info0["n_jv"] == _n_jv(passes, 0, 1, mA, gemm)
    for R in (1, 2, 5, 16):
        cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
        for rep in range(2):
            s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, R, 1, gemm, cons=cons)
            assert np.array_equal(s, s_ref), (R, rep, relnorm(s, s_ref))
            assert np.array_equal(fix, fix_ref) and info["n_hmul"] == passes and info["n_breakpoints"] == info0["n_breakpoints"] == passes - 1, (R, info)
            assert info["form"] == FORM_ROWSPACE_EQ
            assert info["n_jv"] == _n_jv(passes, R, 1, mA, gemm), (R, info, passes)
        cons.close()
    H.close()


@pytest.mark.parametrize("rows,mA,gemm", [(1100, 3, 0), (1100, 17, 1)])
def test_equality_form_with_a_dense_a_takes_the_same_decisions(bh, rows, mA, gemm):
    """Beside the exact case: a dense A with entries in {-1, 0, 1}, whose projection is not dyadic — passes, breakpoints and active set
    identical to R = 0 and the oracle, steps at the bound of test_cauchy_step_parity (1e-9), feasible at 1e-10 ||A|| ||s||."""
    (J, C, mu, A, x, g, xlow, xupp, delta), (s_ref, fix_ref, passes) = _exact(rows, 192, 3, 40, mA)
    H = bh.AlHessian(J, C, mu)
    s0, fix0, info0 = _search(bh, H, A, xlow, xupp, x, g, delta, 0, 1, gemm)
    assert info0["form"] == FORM_ROWSPACE_EQ and info0["n_hmul"] == passes and np.array_equal(fix0, fix_ref)
    for R in (1, 16):
        s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, R, 1, gemm)
        assert np.array_equal(fix, fix_ref) and info["n_hmul"] == passes and info["n_breakpoints"] == info0["n_breakpoints"], (R, info)
        assert info["n_jv"] == _n_jv(passes, R, 1, mA, gemm), (R, info, passes)
        rel = relnorm(s, s_ref)
        note_tol("cauchy_image_refresh, dense A: step vs oracle, 1e-9", rel, 1e-9, "rows=%d mA=%d R=%d" % (rows, mA, R))
        assert rel <= 1e-9 and relnorm(s, s0) <= 1e-9, (R, rel)
        assert np.linalg.norm(A @ s) <= 1e-10 * np.linalg.norm(A) * max(np.linalg.norm(s), 1e-300)
    H.close()


# ------------------------------------------------------------------------------------------------------------ 4. the point
@functools.lru_cache(maxsize=None)
def _bad(d, mA=0):
    J, x, g, xlow, xupp, delta = rc.bad_instance(d)
    n = J.shape[1]
    A = rc.bad_equalities(mA, n) if mA else np.zeros((0, n))
    s, fix, passes = rc.oracle_step(J, None, 0.0, A, x, g, xlow, xupp, delta)
    s_ld, fix_ld, p_ld = rc.oracle_step(J, None, 0.0, A, x, g, xlow, xupp, delta, longdouble=True)
    b, sigma = rc.step_bound(s, s_ld)
    return (J, A, x, g, xlow, xupp, delta), (s, fix, passes), b


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("d", [96, 256])
def test_badly_scaled_instance_stays_within_the_oracles_bound(bh, d, fused):
    """||d|| shrinks by eight decades over 120 breakpoints (tests/refresh_cases.py::bad_instance; the CPU test shows the carried
    float64 recurrence more than 100 b away from the oracle and the one formed again every 16th pass within b).  With R = 16 the
    device step is within b = max(1e-13, 64 sigma) ||s_oracle|| of the oracle, same breakpoints and active set.  R = 0 is recorded in
    the tolerance-use table only: existing behaviour is not under test."""
    (J, A, x, g, xlow, xupp, delta), (s_ref, fix_ref, passes), b = _bad(d)
    H = bh.AlHessian(J, None, 0.0)
    s0, fix0, info0 = _search(bh, H, A, xlow, xupp, x, g, delta, 0, fused)
    note_tol("cauchy_image_refresh = 0 on the badly scaled instance (recorded, not asserted): step vs oracle / b",
             np.linalg.norm(s0 - s_ref), b, "d=%d fused=%d" % (d, fused))
    s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, 16, fused)
    H.close()
    err = float(np.linalg.norm(s - s_ref))
    print("d=%d fused=%d: %d passes; R=0 %.3e b, R=16 %.3e b" % (d, fused, passes, np.linalg.norm(s0 - s_ref) / b, err / b))
    note_tol("cauchy_image_refresh = 16 on the badly scaled instance: step vs oracle, b", err, b, "d=%d fused=%d" % (d, fused))
    assert info["n_hmul"] == passes and info["n_breakpoints"] == passes - 1 and np.array_equal(fix, fix_ref), info
    assert err <= b, (err, b)


def test_badly_scaled_instance_with_equalities(bh):
    """The same J and g with three linear equalities, R = 16: feasible at the level test_cauchy_step_parity asserts, within b of
    the oracle."""
    (J, A, x, g, xlow, xupp, delta), (s_ref, fix_ref, passes), b = _bad(96, 3)
    H = bh.AlHessian(J, None, 0.0)
    s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, 16)
    H.close()
    err = float(np.linalg.norm(s - s_ref))
    feas = float(np.linalg.norm(A @ s))
    print("mA=3: %d passes (device %d); R=16 %.3e b; ||A s|| %.3e of %.3e" % (passes, info["n_hmul"], err / b, feas,
                                                                              1e-10 * np.linalg.norm(A) * np.linalg.norm(s)))
    note_tol("cauchy_image_refresh = 16, badly scaled, mA = 3: step vs oracle, b", err, b)
    assert info["form"] == FORM_ROWSPACE_EQ
    assert np.all(x + s <= xupp + 1e-12) and np.all(x + s >= xlow - 1e-12) and np.max(np.abs(s)) <= delta * (1 + 1e-12)
    assert feas <= 1e-10 * np.linalg.norm(A) * max(np.linalg.norm(s), 1e-300)
    assert info["n_hmul"] == passes and np.array_equal(fix, fix_ref), info
    assert err <= b, (err, b)


# ------------------------------------------------------------------------------------------------------------ 5. R = 1
def _random_instance(d, n, q, nact, delta_scale, seed):
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((d, n)) / np.sqrt(d)
    C = rng.standard_normal((q, n))
    xlow, xupp = -np.ones(n), np.ones(n)
    x = np.clip(0.5 * rng.standard_normal(n), -0.95, 0.95)
    act = rng.choice(n, nact, replace=False)
    x[act] = np.where(rng.random(nact) < 0.5, -1.0, 1.0)
    g = rng.standard_normal(n)
    return J, C, xlow, xupp, x, g, delta_scale * 0.1 * float(np.linalg.norm(g))


@pytest.mark.parametrize("fused", [1, 0])
def test_every_pass_formed_from_j_agrees_with_the_sweeping_form(bh, fused):
    """R = 1 on a random well-scaled instance of test_cauchy_step_in_the_row_space_of_j's size (700 x 257, q = 1): every pass works
    on fresh images; the step agrees with cauchy_image = 0 and with the oracle within that test's 1e-9."""
    J, C, xlow, xupp, x, g, delta = _random_instance(700, 257, 1, 20, 3.0, 12)
    Z = np.zeros((0, 257))
    s_ref, fix_ref, passes = rc.oracle_step(J, C, 2.5, Z, x, g, xlow, xupp, delta)
    H = bh.AlHessian(J, C, 2.5)
    s, fix, info = _search(bh, H, Z, xlow, xupp, x, g, delta, 1, fused)
    bh.set_option("cauchy_image", 0)
    try:
        s_sw, fix_sw, info_sw = _search(bh, H, Z, xlow, xupp, x, g, delta, 0)
    finally:
        bh.set_option("cauchy_image", 1)
    H.close()
    assert info["n_hmul"] == passes == info_sw["n_hmul"] and np.array_equal(fix, fix_ref) and np.array_equal(fix_sw, fix_ref)
    assert info["n_jv"] == _n_jv(passes, 1, fused)
    rel = relnorm(s, s_ref)
    note_tol("cauchy_image_refresh = 1: step vs oracle, 1e-9", rel, 1e-9, "fused=%d, %d passes" % (fused, passes))
    assert rel <= 1e-9 and relnorm(s, s_sw) <= 1e-9, (rel, relnorm(s, s_sw))


# ------------------------------------------------------------------------------------------------------------ 6. option off
_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import benlsip_jl_amd as bh
from test_cauchy_refresh_gpu import _random_instance
bh.init(0)
J, C, xlow, xupp, x, g, delta = _random_instance(300, 130, 2, 10, 3.0, 21)
H = bh.AlHessian(J, C, 2.5)
cons = bh.MixedConstraints(np.zeros((0, 130)), None, None, l=xlow, u=xupp)
jv0 = H.stats()["n_jv"]
s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
print("RESULT", s.tobytes().hex(), info["n_hmul"], info["n_launches"], H.stats()["n_jv"] - jv0)
"""


def test_option_at_zero_is_the_library_that_never_saw_it(bh):
    """After the option was used and set back to 0, step (bit for bit), passes, n_jv and bh_cauchy_info's launch count equal those of
    a fresh process that never touched it."""
    J, C, xlow, xupp, x, g, delta = _random_instance(300, 130, 2, 10, 3.0, 21)
    Z = np.zeros((0, 130))
    H = bh.AlHessian(J, C, 2.5)
    _search(bh, H, Z, xlow, xupp, x, g, delta, 3)
    H.close()
    H = bh.AlHessian(J, C, 2.5)
    s, fix, info = _search(bh, H, Z, xlow, xupp, x, g, delta, 0)
    H.close()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oracle"), os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", _CHILD % (os.path.join(ROOT, "tests"), ROOT)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")][0].split()
    assert line[1] == s.tobytes().hex()
    assert (int(line[2]), int(line[3]), int(line[4])) == (info["n_hmul"], info["n_launches"], info["n_jv"]), (line[2:], info)
