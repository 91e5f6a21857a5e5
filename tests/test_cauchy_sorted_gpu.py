"""GPU tests of the sorted form of the box-constrained Cauchy search on a Gram-form handle (bh_hess_set_cauchy_search at
BH_CAUCHY_SORTED, bh_cauchy_info form 5, csrc/bh_cauchysort.hip.h): the whole search of
src/basic_tralcnlss.jl:574-639 from one sorted sweep over G — ranks of the breakpoint times, one read of the free rows of G, one
scan — against hand-derived answers, the oracle, and the device's own stepwise forms."""
import ctypes as ct
import functools

import numpy as np
import pytest

import benlsip_ref as R
import gram_cases as gc
import refresh_cases as rc
import sorted_cases as sc
from _util import closed_form_cauchy_cases, note_tol, relnorm
from hip_ops import HipOpsResident
from test_sorted_cases_cpu import ORACLE_CASES, oracle_instance

pytestmark = pytest.mark.gpu

FORM_HD, FORM_ROWSPACE, FORM_ROWSPACE_EQ, FORM_GRAM, FORM_SORTED = 0, 1, 2, 3, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _gram(bh, J, C=None, mu=0.0, search="sorted"):
    H = bh.AlHessian(J, C if C is not None and C.shape[0] else None, mu)
    H.set_form("gram")
    H.set_cauchy_search(search)
    return H


def _search(bh, H, A, xlow, xupp, x, g, delta, mode, cauchy_gram=0):
    """One search on a fresh constraint handle with the handle's switch at `mode`: (step, set, info, growth of n_hmul, of n_jv)."""
    H.set_cauchy_search(mode)
    bh.set_option("cauchy_gram", cauchy_gram)
    try:
        cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
        try:
            st0 = H.stats()
            s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
            st1 = H.stats()
            fix = np.asarray(cons.fixvars, dtype=bool).copy()
        finally:
            cons.close()
    finally:
        bh.set_option("cauchy_gram", 0)
    return s, fix, info, st1["n_hmul"] - st0["n_hmul"], st1["n_jv"] - st0["n_jv"]


def _inst_search(bh, H, inst, mode, cauchy_gram=0):
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    return _search(bh, H, np.zeros((0, J.shape[1])), xlow, xupp, x, g, delta, mode, cauchy_gram)


# ------------------------------------------------------------------------------------------------------------ 1. hand-derived
def test_closed_form_cases(bh):
    """closed_form_cauchy_cases (H = I in two variables, dyadic data): step bit for bit, active set, number of decisions, form 5."""
    Z = np.zeros((0, 2))
    for case in closed_form_cauchy_cases():
        H = _gram(bh, np.eye(2))
        s, fix, info, _, _ = _search(bh, H, Z, -np.ones(2), np.ones(2), np.zeros(2), case["g"], case["delta"], "sorted")
        assert info["form"] == FORM_SORTED, (case["name"], info)
        assert np.array_equal(bits(s), bits(case["s"])), (case["name"], s, case["s"])
        assert np.array_equal(fix, case["fix"]), (case["name"], fix)
        assert info["n_hmul"] == case["n_hmul"] and info["n_breakpoints"] == int(fix.sum()), (case["name"], info)
        H.close()


# ------------------------------------------------------------------------------------------------------------ 2. family K, the edges
@functools.lru_cache(maxsize=None)
def _exact_cases(n):
    """Family K and, at the edge sizes, the placements of tests/sorted_cases.py, with the oracle's (step, set, products): once, read-only."""
    out = []
    for c in gc.k_cases(n) + (sc.edge_cases(n) if n in sc.EDGE_SIZES else []):
        J, C, mu, A, x, g, xlow, xupp, delta = c.inst
        ref = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
        for arr in (J, C, x, g, xlow, xupp) + ref[:2]:
            arr.setflags(write=False)
        out.append((c, ref))
    return out


@pytest.mark.parametrize("n", gc.K_SIZES)
def test_family_k_and_the_edges_bit_for_bit(bh, n):
    """ONE Gram-form handle per width; every case: s as uint64, set and n_hmul equal to the oracle; the same bits from form 3 on the
    same handle; one build of G; stats.n_hmul + 1 and n_jv + 0 per sorted search; searches_sorted counts every one."""
    cases = _exact_cases(n)
    inst0 = cases[0][0].inst
    H = _gram(bh, inst0[0], inst0[1], inst0[2])
    wrong = []                                                       # every case is run; the cases that differ are reported together
    try:
        for k, (c, ref) in enumerate(cases):
            what = "n=%d %s" % (n, c.name)
            assert np.array_equal(c.inst[0], inst0[0]) and np.array_equal(c.inst[1], inst0[1]) and c.inst[2] == inst0[2]
            s_ref, fix_ref, passes = ref
            try:
                s, fix, info, dh, dj = _inst_search(bh, H, c.inst, "sorted")
                assert info["form"] == FORM_SORTED, (what, info)
                assert (info["n_hmul"], info["n_breakpoints"]) == (passes, int(fix_ref.sum())), (what, info, passes)
                assert np.array_equal(fix, fix_ref), (what, np.flatnonzero(fix != fix_ref)[:8])
                assert np.array_equal(bits(s), bits(s_ref)), (what, np.flatnonzero(bits(s) != bits(s_ref))[:8])
                assert (dh, dj) == (1, 0), (what, dh, dj)
                assert H.searches_sorted == k + 1, (what, H.searches_sorted)
                s3, fix3, info3, _, _ = _inst_search(bh, H, c.inst, "stepwise", cauchy_gram=1)
                assert info3["form"] == FORM_GRAM, (what, info3)
                assert np.array_equal(bits(s3), bits(s)) and np.array_equal(fix3, fix) and info3["n_hmul"] == info["n_hmul"], what
            except AssertionError as e:
                wrong.append(str(e).splitlines()[0])
        assert H.gram_builds == 1
    finally:
        H.close()
    assert not wrong, "\n".join(wrong)


# ------------------------------------------------------------------------------------------------------------ 3. the oracle
def _oracle(J, C, mu, xlow, xupp, x, g, delta):
    return rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_against_the_oracle(bh, case):
    """Same final active set, decisions = the oracle's H*d products, step within 1e-9, feasible, form 5, one read of G
    and one build."""
    d, n = case[0], case[1]
    J, C, xlow, xupp, x, g, delta = oracle_instance(*case)
    mu = 2.5
    s_ref, fix_ref, n_hd = _oracle(J, C, mu, xlow, xupp, x, g, delta)
    H = _gram(bh, J, C, mu)
    s, fix, info, dh, dj = _search(bh, H, np.zeros((0, n)), xlow, xupp, x, g, delta, "sorted")
    assert info["form"] == FORM_SORTED, info
    assert np.array_equal(fix, fix_ref), (np.flatnonzero(fix), np.flatnonzero(fix_ref))
    assert info["n_hmul"] == n_hd, (info, n_hd)
    rel = relnorm(s, s_ref)
    note_tol("cauchy_step from one sorted sweep over G: step vs oracle, 1e-9", rel, 1e-9, "d=%d n=%d, %d breakpoints" % (d, n, info["n_breakpoints"]))
    assert rel <= 1e-9, rel
    assert np.all(x + s <= xupp + 1e-12) and np.all(x + s >= xlow - 1e-12) and np.max(np.abs(s)) <= delta * (1 + 1e-12)
    assert (dh, dj) == (1, 0) and H.gram_builds == 1
    H.close()


# ------------------------------------------------------------------------------------------------------------ 4. launch count
def test_launch_count_does_not_depend_on_the_search_length(bh):
    J, C, xlow, xupp, x, g, _ = oracle_instance(3000, 1024, 0, 100, 1.0, 13)
    Z = np.zeros((0, 1024))
    H = _gram(bh, J, C, 2.5)
    gn = float(np.linalg.norm(g))
    _search(bh, H, Z, xlow, xupp, x, g, 0.1 * gn, "sorted")          # the build of G is behind us
    on = [_search(bh, H, Z, xlow, xupp, x, g, f * gn, "sorted")[2] for f in (0.005, 1.0)]
    assert abs(on[0]["n_breakpoints"] - on[1]["n_breakpoints"]) > 10, on
    assert on[0]["form"] == on[1]["form"] == FORM_SORTED
    assert on[0]["n_launches"] == on[1]["n_launches"] < 16, on
    H.close()


# ------------------------------------------------------------------------------------------------------------ 5. fall-backs
@pytest.mark.parametrize("gram_handle,mA,form", [(False, 0, FORM_ROWSPACE), (True, 3, FORM_ROWSPACE_EQ), (True, 96, FORM_HD)])
def test_fall_backs_are_silent_and_exact(bh, gram_handle, mA, form):
    """Implicit handle, or linear equalities: the switch changes nothing — same form as without it, step and active set bit for bit."""
    n = 200
    J, C, xlow, xupp, x, g, delta = oracle_instance(500, n, 1, 10, 0.3, 31 + mA)
    A = np.random.default_rng(7).standard_normal((mA, n))
    if mA:
        x = x - A.T @ np.linalg.solve(A @ A.T, A @ x)
        x = np.clip(x, -0.95, 0.95)
    H = bh.AlHessian(J, C, 2.5)
    if gram_handle:
        H.set_form("gram")
    s0, f0, i0, _, _ = _search(bh, H, A, xlow, xupp, x, g, delta, "stepwise")
    s1, f1, i1, _, _ = _search(bh, H, A, xlow, xupp, x, g, delta, "sorted")
    assert i0["form"] == form and i1["form"] == form, (i0, i1)
    assert np.array_equal(bits(s1), bits(s0)) and np.array_equal(f1, f0)
    assert (i1["n_breakpoints"], i1["n_hmul"]) == (i0["n_breakpoints"], i0["n_hmul"])
    assert H.searches_sorted == 0 and H.cauchy_search == "sorted"
    H.close()


# ------------------------------------------------------------------------------------------------------------ 6. every variable fixed
def test_every_variable_fixed(bh):
    """block_cases.all_fixed: rank nfree - 1 is reached, decision n + 1 ends on nfix == nmm."""
    for c in gc.k_all_fixed():
        J, C, mu, A, x, g, xlow, xupp, delta = c.inst
        s_ref, fix_ref, passes = rc.oracle_step(J, None, mu, None, x, g, xlow, xupp, delta)
        assert passes == c.n + 1 and fix_ref.all()
        H = _gram(bh, J, None, mu)
        s, fix, info, _, _ = _inst_search(bh, H, c.inst, "sorted")
        assert info["form"] == FORM_SORTED and (info["n_hmul"], info["n_breakpoints"]) == (passes, c.n), (c.name, info)
        assert fix.all() and np.array_equal(bits(s), bits(s_ref)), c.name
        H.close()


# ------------------------------------------------------------------------------------------------------------ 7. no breakpoint left
@pytest.mark.parametrize("n", [1030, 4097])
def test_no_breakpoint_left_is_the_same_error(bh, n):
    """J = 0, infinite bounds and trust region: decision 0 finds no breakpoint (ind < 0) — the code of the stepwise path, non-zero."""
    c = gc.k_no_breakpoint(n)
    H = _gram(bh, c.inst[0], None, c.inst[2])
    codes = []
    try:
        for mode in ("stepwise", "sorted"):
            try:
                _inst_search(bh, H, c.inst, mode)
                codes.append(0)
            except bh.BenlsipHipError as e:
                codes.append(e.code)
        assert H.searches_sorted == 1                                 # decided by the sorted form itself, not handed back
    finally:
        H.close()
    assert codes[0] == codes[1] != 0, codes


# ------------------------------------------------------------------------------------------------------------ 8. hand-back
def _outcome(bh, H, inst, mode):
    """One search as a comparable tuple: (0, bits of s, set, form, n_hmul), or (error code,)."""
    try:
        s, fix, info, _, _ = _inst_search(bh, H, inst, mode)
        return (0, bits(s).tolist(), fix.tolist(), info["form"], info["n_hmul"])
    except bh.BenlsipHipError as e:
        return (e.code,)


@pytest.mark.parametrize("what", ["nan_g", "nan_bound"])
def test_nan_in_g_is_handed_back(bh, what):
    """One NaN in g or in a bound of a free variable (n = 6): the call runs on the stepwise path — its return code and bits,
    searches_sorted unchanged — and the handle serves the next, finite call in the sorted form."""
    n = 6
    rng = np.random.default_rng(3)
    J = rng.standard_normal((20, n)) / np.sqrt(20.0)
    g = rng.standard_normal(n)
    x, xlow, xupp = np.zeros(n), -np.ones(n), np.ones(n)
    if what == "nan_g":
        g[2] = np.nan
    else:
        xupp[4] = np.nan
    H = _gram(bh, J)
    inst = (J, None, 0.0, None, x, g, xlow, xupp, 10.0)
    got = [_outcome(bh, H, inst, mode) for mode in ("stepwise", "sorted")]
    assert got[0] == got[1], got
    assert H.searches_sorted == 0
    g[2], xupp[4] = 0.25, 1.0                                        # the handle serves the next, finite call in the sorted form
    s, fix, info, _, _ = _search(bh, H, np.zeros((0, n)), xlow, xupp, x, g, 10.0, "sorted")
    s0, fix0, info0, _, _ = _search(bh, H, np.zeros((0, n)), xlow, xupp, x, g, 10.0, "stepwise")
    assert info["form"] == FORM_SORTED and H.searches_sorted == 1
    assert np.array_equal(fix, fix0) and info["n_hmul"] == info0["n_hmul"] and relnorm(s, s0) <= 1e-9
    H.close()


def test_nan_bound_past_the_scan_kernels_first_trip(bh):
    """(a) variable 1027 free: handed back — the counter unchanged, code and bits the stepwise path's.  (b) fixed at the start: the
    bound is never looked at — a sorted search, set and decisions of the restatement, the step within 1e-9 of it."""
    assert 1027 >= sc.SCAN_T
    inst = sc.nan_bound_past_the_first_trip(False)
    H = _gram(bh, inst[0])
    try:
        got = [_outcome(bh, H, inst, mode) for mode in ("stepwise", "sorted")]
        assert got[0] == got[1], [t[:1] + t[3:] for t in got]
        assert H.searches_sorted == 0
        inst = sc.nan_bound_past_the_first_trip(True)
        res = sc.sorted_search(inst)
        assert not res.handback
        s, fix, info, _, _ = _inst_search(bh, H, inst, "sorted")
        assert info["form"] == FORM_SORTED and H.searches_sorted == 1
        assert np.array_equal(fix, res.fix) and info["n_hmul"] == res.n_hmul, (info, res.n_hmul)
        assert relnorm(s, res.s) <= 1e-9, relnorm(s, res.s)
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------------ 9. stale G
@pytest.mark.parametrize("asynchronous", [False, True])
def test_stale_g_is_rebuilt_before_the_search(bh, asynchronous):
    d, n, q = 700, 257, 1
    J, C, xlow, xupp, x, g, delta = oracle_instance(d, n, q, 20, 0.3, 12)
    Z = np.zeros((0, n))
    if asynchronous:
        H = bh.AlHessian.create_async(J, C, 2.5)                  # no wait: the build of G is ordered behind the upload
        H.set_form("gram")
        H.set_cauchy_search("sorted")
    else:
        H = _gram(bh, J, C, 2.5)
    for k, mu in enumerate((2.5, 40.0)):
        if k:
            H.mu = mu
        s, fix, info, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
        s_ref, fix_ref, n_hd = _oracle(J, C, mu, xlow, xupp, x, g, delta)
        assert info["form"] == FORM_SORTED and H.gram_builds == k + 1
        assert np.array_equal(fix, fix_ref) and info["n_hmul"] == n_hd
        note_tol("cauchy_step from one sorted sweep over G: step vs oracle, 1e-9", relnorm(s, s_ref), 1e-9,
                 "mu=%g%s" % (mu, ", async ingest" if asynchronous else ""))
        assert relnorm(s, s_ref) <= 1e-9
    H.close()


# ------------------------------------------------------------------------------------------------------------ 10. resident chain
class _GramResident(HipOpsResident):
    search = "stepwise"

    def new_hessian(self, J, C, mu):
        H = self.bh.AlHessian(J, C, mu)
        H.set_form("gram")
        H.set_cauchy_search(self.search)
        return H


class _SortedResident(_GramResident):
    search = "sorted"


def test_resident_inner_step_takes_the_sorted_search(bh):
    """bh.inner_step (box constraints) on a Gram-form handle with the switch on against the oracle's inner_step, under the rule of
    test_resident_inner_step_takes_the_one_launch_search; the PCIe bytes of the loop are those of the switch-off run."""
    d, n = 4096, 512
    J = R.synthetic_J(d, n, seed=1)
    inst = R.synthetic_box_vectors(d, n, fix_every=8)
    A = np.zeros((0, n))
    L0 = R.chol_lower(A @ A.T)
    x = np.clip(inst.x, inst.x_l, inst.x_u)
    g = J.T @ inst.r0
    delta = R.initial_tr(g)

    def run(ops):
        cons = R.make_mixed_constraints(A, L0, l=inst.x_l, u=inst.x_u)
        H = ops.new_hessian(J, np.zeros((0, n)), 10.0)
        log = []
        if hasattr(ops, "inner_step"):
            s, pred = ops.inner_step(x, g, H, L0, cons, delta, 50, 0.1, 0.1, log)
            form = bh.cauchy_info(cons._dev)[0]
        else:
            s, pred = R.inner_step(x, g, H, L0, cons, delta, 50, 0.1, 0.1, ops=ops, log=log)
            form = None
        return s, pred, log, cons.fixvars.copy(), form

    s_ref, pred_ref, log_ref, fix_ref, _ = run(R.NumpyOps())
    off = _GramResident(bh)
    s_off, pred_off, log_off, fix_off, form_off = run(off)
    on = _SortedResident(bh)
    s_on, pred_on, log_on, fix_on, form_on = run(on)
    assert (form_off, form_on) == (FORM_ROWSPACE, FORM_SORTED)
    assert [e[1] for e in log_on] == [e[1] for e in log_ref]
    assert [e[2] for e in log_on] == [e[2] for e in log_ref]
    assert np.array_equal(fix_on, fix_ref)
    note_tol("inner_step with the sorted Cauchy search: s vs oracle, 1e-6", relnorm(s_on, s_ref), 1e-6)
    assert relnorm(s_on, s_ref) <= 1e-6, relnorm(s_on, s_ref)
    assert pred_on == pytest.approx(pred_ref, rel=1e-8)
    assert on.loop_minor == off.loop_minor and on.loop_bytes == off.loop_bytes, (on.loop_bytes, off.loop_bytes)


# ------------------------------------------------------------------------------------------------------------ 11. setter and getter
def test_setter_and_getter(bh):
    lib = bh._lib.lib()
    J, C, xlow, xupp, x, g, delta = oracle_instance(700, 257, 1, 20, 0.3, 12)
    Z = np.zeros((0, 257))
    H = bh.AlHessian(J, C, 2.5)
    assert (H.cauchy_search, H.cauchy_search_served, H.searches_sorted) == ("stepwise", True, 0)
    H.set_cauchy_search("sorted")                                    # callable in the implicit form: remembered
    assert H.cauchy_search == "sorted"
    H.set_form("gram")
    assert H.cauchy_search == "sorted" and H.gram_builds == 0        # the switch builds nothing
    for bad in (-1, 2, 7):
        assert lib.bh_hess_set_cauchy_search(H._h, bad) == bh._lib.BH_ERR_INVALID_ARG
        assert H.cauchy_search == "sorted"
    assert lib.bh_hess_set_cauchy_search(None, 1) == bh._lib.BH_ERR_INVALID_ARG
    assert lib.bh_hess_get_cauchy_search(None, None, None, None) == bh._lib.BH_ERR_INVALID_ARG
    assert lib.bh_hess_get_cauchy_search(H._h, None, None, None) == 0
    m = ct.c_int32(-1)
    assert lib.bh_hess_get_cauchy_search(H._h, ct.byref(m), None, None) == 0 and m.value == bh._lib.BH_CAUCHY_SORTED
    with pytest.raises(ValueError):
        H.set_cauchy_search("fast")
    s1, f1, i1, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
    s2, f2, i2, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
    assert i1["form"] == i2["form"] == FORM_SORTED and H.searches_sorted == 2 and H.gram_builds == 1
    assert np.array_equal(bits(s1), bits(s2)) and np.array_equal(f1, f2) and i1["n_hmul"] == i2["n_hmul"]      # bit-reproducible
    H.set_form("implicit")
    assert H.cauchy_search == "sorted"                               # remembered across bh_hess_set_form
    s0, f0, i0, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
    assert i0["form"] == FORM_ROWSPACE and H.searches_sorted == 2
    H.set_form("gram")
    s3, f3, i3, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
    assert i3["form"] == FORM_SORTED and np.array_equal(bits(s3), bits(s1)) and H.searches_sorted == 3
    H.set_cauchy_search("stepwise")
    s4, f4, i4, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "stepwise")
    assert i4["form"] == FORM_ROWSPACE and np.array_equal(f4, f1) and relnorm(s4, s1) <= 1e-9
    H.close()
    wide = bh.AlHessian(np.zeros((2, 16400)), None, 0.0)
    assert not wide.cauchy_search_served
    wide.close()
