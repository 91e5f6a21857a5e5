"""CPU tests of option cauchy_image_refresh (periodic re-formation of J d and J s_c in the row-space Cauchy search): the conditions the
GPU test relies on, computed with a float64 restatement of the carried recurrence (tests/refresh_cases.py) and the oracle; the option's
value check; the header; the host source counts only the re-formations that ran (no compute without a GPU)."""
import functools
import os
import re

import numpy as np
import pytest

import refresh_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _bad(d):
    J, x, g, xlow, xupp, delta = rc.bad_instance(d)
    s, fix, passes = rc.oracle_step(J, None, 0.0, None, x, g, xlow, xupp, delta)
    s_ld, fix_ld, passes_ld = rc.oracle_step(J, None, 0.0, None, x, g, xlow, xupp, delta, longdouble=True)
    assert np.array_equal(fix, fix_ld) and passes == passes_ld
    b, sigma = rc.step_bound(s, s_ld)
    return (J, x, g, xlow, xupp, delta), (s, fix, passes), b, sigma


@pytest.mark.parametrize("d", [96, 256])
def test_conditions_of_the_badly_scaled_instance(d):
    """(a) the oracle passes >= 100 breakpoints; (b) the carried recurrence (R = 0) leaves the oracle's step by more than 100 b;
    (c) formed again every 16th pass it stays within b — b = max(1e-13, 64 sigma) ||s_oracle||, sigma the oracle's own sensitivity.
    Same breakpoints and active set either way: only the rounding of phi', phi'' differs."""
    (J, x, g, xlow, xupp, delta), (s, fix, passes), b, sigma = _bad(d)
    assert passes - 1 >= 100, passes                                                              # (a)
    s0, fix0, p0 = rc.carried_search(J, None, 0.0, x, g, xlow, xupp, delta, 0)
    s16, fix16, p16 = rc.carried_search(J, None, 0.0, x, g, xlow, xupp, delta, 16)
    assert p0 == passes and p16 == passes and np.array_equal(fix0, fix) and np.array_equal(fix16, fix)
    e0, e16 = float(np.linalg.norm(s0 - s)), float(np.linalg.norm(s16 - s))
    print("d=%d: %d passes, sigma %.2e, b/||s|| %.2e, R=0: %.3e b, R=16: %.3e b" % (d, passes, sigma, b / np.linalg.norm(s), e0 / b, e16 / b))
    assert e0 > 100.0 * b, (e0, b)                                                                # (b)
    assert e16 <= b, (e16, b)                                                                     # (c)


def test_badly_scaled_instance_with_equalities_has_a_trustworthy_oracle():
    """mA = 3 on the same J, g (refresh_cases.bad_equalities): the oracle passes the same 120 breakpoints, its step is feasible at the
    level test_cauchy_step_parity asserts, and a second CPU restatement of the projector (reduced form, the one the device uses)
    gives its step within b — so b is a bound the device can be held to."""
    import benlsip_ref as R
    from _util import ReducedFormOps
    J, x, g, xlow, xupp, delta = rc.bad_instance(96)
    A = rc.bad_equalities(3)
    s, fix, passes = rc.oracle_step(J, None, 0.0, A, x, g, xlow, xupp, delta)
    s_ld, fix_ld, p_ld = rc.oracle_step(J, None, 0.0, A, x, g, xlow, xupp, delta, longdouble=True)
    b, sigma = rc.step_bound(s, s_ld)
    assert passes - 1 >= 100 and p_ld == passes and np.array_equal(fix, fix_ld)
    assert np.linalg.norm(A @ s) <= 1e-10 * np.linalg.norm(A) * np.linalg.norm(s)
    L0 = R.chol_lower(A @ A.T)
    cons = R.make_mixed_constraints(A, L0, l=xlow, u=xupp)
    s2 = R.cauchy_step(x, g, R.AlHessian(J, np.zeros((0, 160)), 0.0), L0, cons, delta, ReducedFormOps())
    assert np.array_equal(cons.fixvars, fix) and np.linalg.norm(s2 - s) <= b


EXACT = [(5, 7, 0, 5), (5, 7, 3, 3), (1100, 192, 3, 33), (5, 192, 0, 33), (1100, 4100, 3, 33), (5, 4100, 0, 32), (1100, 192, 0, 17),
         (1100, 192, 3, 16)]


@pytest.mark.parametrize("rows,n,q,npass", EXACT)
def test_exact_instances_are_exact(rows, n, q, npass):
    """The dyadic instances of the GPU test: the oracle takes exactly npass passes, and the carried recurrence gives the oracle's step
    to the last bit for every R — nothing on the way is rounded but the final quotient, which has the same operands everywhere."""
    J, C, mu, A, x, g, xlow, xupp, delta = rc.exact_instance(rows, n, q, npass)
    s, fix, passes = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
    assert passes == npass
    for R in (0, 1, 2, 5, 16):
        sR, fixR, pR = rc.carried_search(J, C, mu, x, g, xlow, xupp, delta, R)
        assert pR == npass and np.array_equal(fixR, fix) and np.array_equal(sR, s), R


@pytest.mark.parametrize("rows,n,q,npass", [(11, 1000, 0, 6), (11, 2000, 3, 6), (11, 4096, 0, 6), (11, 8200, 3, 6)])
def test_exact_instances_of_the_other_geometries_are_exact(rows, n, q, npass):
    J, C, mu, A, x, g, xlow, xupp, delta = rc.exact_instance(rows, n, q, npass)
    s, fix, passes = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
    assert passes == npass
    for R in (0, 1, 5):
        sR, fixR, pR = rc.carried_search(J, C, mu, x, g, xlow, xupp, delta, R)
        assert pR == npass and np.array_equal(fixR, fix) and np.array_equal(sR, s), R


@pytest.mark.parametrize("rows,mA,per_row", [(1100, 1, 16), (5, 3, 4), (1100, 3, 16), (1100, 17, 4), (5, 17, 4)])
def test_exact_equality_instances_are_exact(rows, mA, per_row):
    """The dyadic equality instances of the GPU test: 40 passes; the oracle's step is the same to the last bit with H*d accumulated in
    long double and with the reduced-form projector (the form the device uses) — nothing on the way is rounded but the last quotient;
    no variable in the support of A is ever fixed."""
    import benlsip_ref as R
    from _util import ReducedFormOps
    J, C, mu, A, x, g, xlow, xupp, delta = rc.exact_equality_instance(rows, 192, 3, 40, mA, per_row)
    assert np.array_equal(A @ A.T, per_row * np.eye(mA))
    s, fix, passes = rc.oracle_step(J, C, mu, A, x, g, xlow, xupp, delta)
    s_ld, fix_ld, p_ld = rc.oracle_step(J, C, mu, A, x, g, xlow, xupp, delta, longdouble=True)
    assert passes == 40 == p_ld and np.array_equal(s, s_ld) and np.array_equal(fix, fix_ld)
    assert not fix[np.abs(A).sum(axis=0) > 0].any()
    L0 = R.chol_lower(A @ A.T)
    cons = R.make_mixed_constraints(A, L0, l=xlow, u=xupp)
    s2 = R.cauchy_step(x, g, R.AlHessian(J, C, mu), L0, cons, delta, ReducedFormOps())
    assert np.array_equal(s2, s) and np.array_equal(cons.fixvars, fix)


def test_option_is_accepted_and_checked():
    import benlsip_jl_amd as bh
    lib = bh.load()
    try:
        assert lib.bh_set_option(b"cauchy_image_refresh", 16) == 0
        assert lib.bh_set_option(b"cauchy_image_refresh", 1) == 0
        assert lib.bh_set_option(b"cauchy_image_refresh", -1) == -1 and b"cauchy_image_refresh" in lib.bh_last_error_detail()
    finally:
        assert lib.bh_set_option(b"cauchy_image_refresh", 0) == 0


def test_header_lists_the_option_with_its_counter_formula():
    hdr = open(os.path.join(ROOT, "include", "benlsip_hip.h")).read()
    m = re.search(r'"cauchy_image_refresh" \[0\](.*?)\n \*   "cauchy_gram"', hdr, re.S)
    assert m
    doc = m.group(1)
    assert "floor((passes - 1) / R)" in doc and "stats.n_jv" in doc and "Several ranks: ignored" in doc and "BH_ERR_INVALID_ARG" in doc


def test_host_counts_only_the_reformations_that_ran():
    """n_jv of the re-formations comes from the progress word after the loop (passes known), not from the launches enqueued — those
    behind the end are gated; the kernel gates before its first load; the gated sweeps carry the loop state."""
    csrc = os.path.join(ROOT, "benlsip.jl_amd", "csrc")
    src = open(os.path.join(csrc, "bh_api.hip")).read()
    impl = src[src.index("struct CauchyPlan {"):src.index("int32_t bh_cauchy_step(")]           # plan, launchers, accounting, cauchy_impl
    account = impl[impl.index("static void cauchy_account("):impl.index("static int32_t cauchy_impl(")]
    assert re.search(r"if \(p\.refresh > 0\) H->stats\.n_jv \+= \(int64_t\)r\.reform_sweeps \* \(std::max\(mw\.n_hmul - 1, 0\) / p\.refresh\);", account)
    assert impl.index("cauchy_account(run, mw, launches_in);") > impl.index("BH_TRY(wait_mirror(c, a.tag, launched - off, &mw));")
    passes = impl[impl.index("static int32_t cauchy_pass_sweep("):impl.index("static int32_t cauchy_launch_pass(")]
    # inside the launchers of a pass the counter moves for pass 0 only
    assert len(re.findall(r"H->stats\.n_jv \+= 1;", passes)) == 3 and "stats.n_jv" not in account.replace("if (p.refresh > 0) H->stats.n_jv", "")
    for m in re.finditer(r"H->stats\.n_jv \+= 1;", passes):
        before = passes[max(0, m.start() - 400):m.start()]
        assert "index == 0" in before or "launch 0" in before, before[-200:]
    rule = open(os.path.join(csrc, "bh_cauchy_plan.h")).read()
    assert re.search(r"if \(image && !in\.comm && [^\n]*\) o\.refresh = ", rule)
    assert "p.refresh = sel.refresh;" in impl
    assert len(re.findall(r"launch_jv\(H, c\.[pw], [^;]*\(const CgState\*\)c\.d_state\)\);", impl)) == 2           # two-kernel box form
    assert re.search(r"launch_jv\(H, c\.w, H->timg \+ rows_cap, true, nullptr, gate\)", impl)                       # equalities: t_s
    ker = open(os.path.join(csrc, "bh_cauchy.hip.h")).read()
    body = ker[ker.index("void cauchy_reform_kernel(CauchyReformArgs a) {"):]
    assert body.index("if (a.gate->done) return;") < body.index("__builtin_nontemporal_load")
    assert "atomic" not in body[:body.index("// M <- M - a a'")]
