"""GPU tests of the sorted rows form of the box-constrained Cauchy search on an implicit handle (bh_hess_set_cauchy_rows at
BH_CAUCHY_ROWS_SORTED, bh_cauchy_info form 6, csrc/bh_cauchyrowsort.hip.h): the whole search of
src/basic_tralcnlss.jl:574-639 from one sorted sweep over J — ranks of the breakpoint times, one read of J with a suffix and a prefix
scan per row, the slab sums, one scan — against the oracle, the device's own stepwise form 1 and the float64 restatement
(tests/rowsort_cases.py)."""
import ctypes as ct
import functools

import numpy as np
import pytest

import benlsip_ref as R
import gram_cases as gc
import refresh_cases as rc
import rowsort_cases as rw
from _util import closed_form_cauchy_cases, note_tol, relnorm
from hip_ops import HipOpsResident
from test_sorted_cases_cpu import ORACLE_CASES, oracle_instance

pytestmark = pytest.mark.gpu

FORM_HD, FORM_ROWSPACE, FORM_ROWSPACE_EQ, FORM_GRAM, FORM_ROWS_SORTED = 0, 1, 2, 3, 6


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _n_cu(bh):
    n_cu, name, arch = ct.c_int32(0), ct.create_string_buffer(256), ct.create_string_buffer(64)
    assert bh._lib.lib().bh_device_info(name, 256, ct.byref(n_cu), arch, 64) == 0
    return n_cu.value


def _search(bh, H, A, xlow, xupp, x, g, delta, mode):
    """One search on a fresh constraint handle with the handle's switch at `mode` (None: untouched): (step, set, info, growth of
    n_hmul, of n_jv)."""
    if mode is not None:
        H.set_cauchy_rows(mode)
    cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
    try:
        st0 = H.stats()
        s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
        st1 = H.stats()
        fix = np.asarray(cons.fixvars, dtype=bool).copy()
    finally:
        cons.close()
    return s, fix, info, st1["n_hmul"] - st0["n_hmul"], st1["n_jv"] - st0["n_jv"]


def _inst_search(bh, H, inst, mode):
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    return _search(bh, H, np.zeros((0, J.shape[1])), xlow, xupp, x, g, delta, mode)


def _handle(bh, inst, mode="sorted"):
    J, C, mu = inst[:3]
    H = bh.AlHessian(J, C if C is not None and C.shape[0] else None, mu)
    H.set_cauchy_rows(mode)
    return H


# ------------------------------------------------------------------------------------------------------------ 1. hand-derived
def test_closed_form_cases(bh):
    """closed_form_cauchy_cases (H = I in two variables, dyadic data): step bit for bit, active set, number of decisions, form 6."""
    Z = np.zeros((0, 2))
    for case in closed_form_cauchy_cases():
        H = bh.AlHessian(np.eye(2), None, 0.0)
        s, fix, info, _, _ = _search(bh, H, Z, -np.ones(2), np.ones(2), np.zeros(2), case["g"], case["delta"], "sorted")
        assert info["form"] == FORM_ROWS_SORTED, (case["name"], info)
        assert np.array_equal(bits(s), bits(case["s"])), (case["name"], s, case["s"])
        assert np.array_equal(fix, case["fix"]), (case["name"], fix)
        assert info["n_hmul"] == case["n_hmul"] and info["n_breakpoints"] == int(fix.sum()), (case["name"], info)
        H.close()


# ------------------------------------------------------------------------------------------------------------ 2. the exact families
def _with_oracle(cases):
    out = []
    for c in cases:
        J, C, mu, A, x, g, xlow, xupp, delta = c.inst
        ref = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
        for arr in (J, C, x, g, xlow, xupp) + ref[:2]:
            arr.setflags(write=False)
        out.append((c, ref))
    return out


@functools.lru_cache(maxsize=None)
def _exact_cases(n):
    """Family K and the placements of tests/rowsort_cases.py at the kernel-sized widths; exact_instance searches (both orders, with
    variables fixed at the start) at the small ones.  With the oracle's (step, set, products): once, read-only."""
    if n >= 1030:
        return _with_oracle(gc.k_cases(n) + (rw.edge_cases(n) if n in (1030, 4096) else []) + [rw.fixed_at_the_start(gc.k_cases(n)[0])])
    rows, q, npass = (24, 2, min(n, 5) + 1)
    K = gc.KCase
    inst = rc.exact_instance(rows, n, q, npass)
    out = [K("drawn", n, inst, "")]
    if n > 1:
        drawn = np.random.default_rng(1000).permutation(n)[:npass - 1][::-1]
        out.append(K("reversed", n, rc.exact_instance(rows, n, q, npass, order=drawn), ""))
        J, C, mu, A, x, g, xlow, xupp, delta = rc.exact_instance(rows, n, q, npass)
        x = x.copy()
        x[::3] = xlow[::3]                                           # every third variable fixed at the start (active_bounds!)
        out.append(K("fixed_at_the_start", n, (J, C, mu, A, x, g, xlow, xupp, delta), ""))
    return _with_oracle(out)


@pytest.mark.parametrize("n", [1, 5, 33, 257, 1030, 4095, 4096])
def test_exact_families_bit_for_bit(bh, n):
    """ONE implicit handle per width; every case: s as uint64, set, n_hmul and n_breakpoints equal to the oracle's; the same bits and
    counts from form 1 on the same handle; stats.n_jv + 1 and n_hmul + 0 per sorted search; searches_rows_sorted counts every one."""
    cases = _exact_cases(n)
    inst0 = cases[0][0].inst
    H = _handle(bh, inst0)
    assert H.cauchy_rows_served
    wrong = []                                                       # every case is run; the cases that differ are reported together
    try:
        for k, (c, ref) in enumerate(cases):
            what = "n=%d %s" % (n, c.name)
            assert np.array_equal(c.inst[0], inst0[0]) and np.array_equal(c.inst[1], inst0[1]) and c.inst[2] == inst0[2]
            s_ref, fix_ref, passes = ref
            try:
                s, fix, info, dh, dj = _inst_search(bh, H, c.inst, "sorted")
                assert info["form"] == FORM_ROWS_SORTED, (what, info)
                nfix0 = int((((c.inst[4] - c.inst[6]) <= gc.SQRT_EPS) | ((c.inst[7] - c.inst[4]) <= gc.SQRT_EPS)).sum())
                assert (info["n_hmul"], info["n_breakpoints"]) == (passes, int(fix_ref.sum()) - nfix0) == (passes, passes - 1), (what, info, passes)
                assert np.array_equal(fix, fix_ref), (what, np.flatnonzero(fix != fix_ref)[:8])
                assert np.array_equal(bits(s), bits(s_ref)), (what, np.flatnonzero(bits(s) != bits(s_ref))[:8])
                assert (dh, dj) == (0, 1), (what, dh, dj)
                assert H.searches_rows_sorted == k + 1, (what, H.searches_rows_sorted)
                s1, fix1, info1, _, _ = _inst_search(bh, H, c.inst, "stepwise")
                assert info1["form"] == FORM_ROWSPACE, (what, info1)
                assert np.array_equal(bits(s1), bits(s)) and np.array_equal(fix1, fix), what
                assert (info1["n_hmul"], info1["n_breakpoints"]) == (info["n_hmul"], info["n_breakpoints"]), (what, info1, info)
            except AssertionError as e:
                wrong.append(str(e).splitlines()[0])
    finally:
        H.close()
    assert not wrong, "\n".join(wrong)


def test_row_counts_around_the_group_and_workgroup_edges(bh):
    """Rows of the image at, one below and one above a row group and the persistent grid (one row, d = 1 included; q > 0 with
    mu = 1/2): bit for bit against the oracle at n = 33."""
    n = 33
    for rows, q in rw.row_count_cases(_n_cu(bh)):
        q = min(q, rows - 1)
        inst = rc.exact_instance(rows, n, q, 6)
        J, C, mu, A, x, g, xlow, xupp, delta = inst
        s_ref, fix_ref, passes = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
        H = _handle(bh, inst)
        try:
            s, fix, info, _, _ = _inst_search(bh, H, inst, "sorted")
            assert info["form"] == FORM_ROWS_SORTED and info["n_hmul"] == passes, (rows, q, info, passes)
            assert np.array_equal(fix, fix_ref) and np.array_equal(bits(s), bits(s_ref)), (rows, q)
        finally:
            H.close()


# ------------------------------------------------------------------------------------------------------------ 3. stop positions
def test_stop_positions(bh):
    """k = 0 (stationary, ends_at_phi_p_0 is in family K at n = 1030), an interior minimiser, k = nfree (all_fixed)."""
    named = {c.name: (c, ref) for c, ref in _exact_cases(1030)}
    H = _handle(bh, named["stationary"][0].inst)
    try:
        s, fix, info, _, _ = _inst_search(bh, H, named["stationary"][0].inst, "sorted")
        assert (info["form"], info["n_breakpoints"], info["n_hmul"]) == (FORM_ROWS_SORTED, 0, 1) and not s.any() and not fix.any()
        c, ref = named["ends_at_phi_p_0"]
        s, fix, info, _, _ = _inst_search(bh, H, c.inst, "sorted")
        assert info["n_hmul"] == ref[2] and np.array_equal(bits(s), bits(ref[0])) and np.array_equal(fix, ref[1])
        c, ref = named["ascending"]
        s, fix, info, _, _ = _inst_search(bh, H, c.inst, "sorted")
        assert 0 < info["n_breakpoints"] < 1030 and np.array_equal(bits(s), bits(ref[0]))
    finally:
        H.close()
    for c in gc.k_all_fixed():
        J, C, mu, A, x, g, xlow, xupp, delta = c.inst
        s_ref, fix_ref, passes = rc.oracle_step(J, None, mu, None, x, g, xlow, xupp, delta)
        assert passes == c.n + 1 and fix_ref.all()
        H = _handle(bh, c.inst)
        s, fix, info, _, _ = _inst_search(bh, H, c.inst, "sorted")
        assert info["form"] == FORM_ROWS_SORTED and (info["n_hmul"], info["n_breakpoints"]) == (passes, c.n), (c.name, info)
        assert fix.all() and np.array_equal(bits(s), bits(s_ref)), c.name
        H.close()


@pytest.mark.parametrize("n", [1030, 4096])
def test_no_breakpoint_left_is_the_same_error(bh, n):
    """J = 0, infinite bounds and trust region: decision 0 finds no breakpoint (ind < 0) — the code of form 1, non-zero."""
    c = gc.k_no_breakpoint(n)
    H = _handle(bh, c.inst)
    codes = []
    try:
        for mode in ("stepwise", "sorted"):
            try:
                _inst_search(bh, H, c.inst, mode)
                codes.append(0)
            except bh.BenlsipHipError as e:
                codes.append(e.code)
        assert H.searches_rows_sorted == 1                           # decided by the sorted form itself, not handed back
    finally:
        H.close()
    assert codes[0] == codes[1] == bh._lib.BH_ERR_PRECONDITION, codes


# ------------------------------------------------------------------------------------------------------------ 4. the oracle
@pytest.mark.parametrize("case", [c for c in ORACLE_CASES if rw.served(c[1])])
def test_against_the_oracle(bh, case):
    """Same final active set, decisions = the oracle's H*d products, step within 1e-9, feasible, form 6, one read of J;
    a repeated search is bit-identical; the restatement at this device's grid agrees to rounding."""
    d, n = case[0], case[1]
    J, C, xlow, xupp, x, g, delta = oracle_instance(*case)
    mu = 2.5
    s_ref, fix_ref, n_hd = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
    H = bh.AlHessian(J, C, mu)
    Z = np.zeros((0, n))
    s, fix, info, dh, dj = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
    assert info["form"] == FORM_ROWS_SORTED, info
    assert np.array_equal(fix, fix_ref), (np.flatnonzero(fix), np.flatnonzero(fix_ref))
    assert info["n_hmul"] == n_hd and info["n_breakpoints"] == n_hd - 1, (info, n_hd)
    rel = relnorm(s, s_ref)
    note_tol("cauchy_step from one sorted sweep over J: step vs oracle, 1e-9", rel, 1e-9, "d=%d n=%d, %d breakpoints" % (d, n, info["n_breakpoints"]))
    assert rel <= 1e-9, rel
    assert np.all(x + s <= xupp + 1e-12) and np.all(x + s >= xlow - 1e-12) and np.max(np.abs(s)) <= delta * (1 + 1e-12)
    assert (dh, dj) == (0, 1)
    s2, fix2, info2, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
    assert np.array_equal(bits(s2), bits(s)) and np.array_equal(fix2, fix) and info2 == info       # bit-reproducible
    H.close()


@pytest.mark.parametrize("case", rw.LONG_CASES)
def test_long_searches_cross_the_wave_edges(bh, case):
    """A stop beyond rank 64 EPT (924 breakpoints with every variable fixed; 3 764 with an interior stop): the cross-wave carries of
    both scans decide phi' and phi''.  Same set and count as form 1 on the same handle and as the float64 restatement at this
    device's grid; the step within 1e-9 of both."""
    J, C, xlow, xupp, x, g, delta = oracle_instance(*case)
    n = case[1]
    Z = np.zeros((0, n))
    H = bh.AlHessian(J, C, 2.5)
    try:
        s, fix, info, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
        s1, fix1, info1, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "stepwise")
    finally:
        H.close()
    res = rw.rowsort_search((J, C, 2.5, None, x, g, xlow, xupp, delta), grid=rw.grid_of(J.shape[0] + C.shape[0], _n_cu(bh)))
    assert (info["form"], info1["form"]) == (FORM_ROWS_SORTED, FORM_ROWSPACE) and info["n_breakpoints"] > 64 * rw.EPT, (info, info1)
    assert (info["n_hmul"], info["n_breakpoints"]) == (info1["n_hmul"], info1["n_breakpoints"]) == (res.n_hmul, res.kstar), (info, info1, res.kstar)
    assert np.array_equal(fix, fix1) and np.array_equal(fix, res.fix)
    note_tol("cauchy_step from one sorted sweep over J: long search vs form 1, 1e-9", relnorm(s, s1), 1e-9, "n=%d, %d breakpoints" % (n, info["n_breakpoints"]))
    assert relnorm(s, s1) <= 1e-9 and relnorm(s, res.s) <= 1e-9


# ------------------------------------------------------------------------------------------------------------ 5. launch count, counters
def test_launch_count_and_counters(bh):
    J, C, xlow, xupp, x, g, _ = oracle_instance(3000, 1024, 0, 100, 1.0, 13)
    Z = np.zeros((0, 1024))
    H = bh.AlHessian(J, C, 2.5)
    gn = float(np.linalg.norm(g))
    _search(bh, H, Z, xlow, xupp, x, g, 0.1 * gn, "sorted")          # the workspace is allocated
    runs = [_search(bh, H, Z, xlow, xupp, x, gg, gn, "sorted") for gg in (np.zeros(1024), g)]      # g = 0: phi' = 0 >= 0 at decision 0
    infos = [r[2] for r in runs]
    assert infos[0]["n_breakpoints"] == 0 and infos[1]["n_breakpoints"] > 10, infos
    assert infos[0]["form"] == infos[1]["form"] == FORM_ROWS_SORTED
    assert infos[0]["n_launches"] == infos[1]["n_launches"] < 16, infos      # (staging and the mask adoption included)
    for r in runs:
        assert (r[3], r[4]) == (0, 1) and r[2]["n_hmul"] == r[2]["n_breakpoints"] + 1
    assert H.searches_rows_sorted == 3
    H.close()


# ------------------------------------------------------------------------------------------------------------ 6. hand-back
def _outcome(bh, H, inst, mode):
    """One search as a comparable tuple: (0, bits of s, set, form, n_hmul), or (error code,)."""
    try:
        s, fix, info, _, _ = _inst_search(bh, H, inst, mode)
        return (0, bits(s).tolist(), fix.tolist(), info["form"], info["n_hmul"])
    except bh.BenlsipHipError as e:
        return (e.code,)


@pytest.mark.parametrize("what", ["nan_g", "nan_bound"])
def test_non_finite_input_is_handed_back(bh, what):
    """One NaN in g or in a bound of a free variable (n = 6): the call runs on the stepwise path — its return code and bits,
    searches_rows_sorted unchanged — and the handle serves the next, finite call in the sorted form."""
    n = 6
    rng = np.random.default_rng(3)
    J = rng.standard_normal((20, n)) / np.sqrt(20.0)
    g = rng.standard_normal(n)
    x, xlow, xupp = np.zeros(n), -np.ones(n), np.ones(n)
    if what == "nan_g":
        g[2] = np.nan
    else:
        xupp[4] = np.nan
    H = bh.AlHessian(J, None, 0.0)
    inst = (J, None, 0.0, None, x, g, xlow, xupp, 10.0)
    got = [_outcome(bh, H, inst, mode) for mode in ("stepwise", "sorted")]
    assert got[0] == got[1], got
    assert H.searches_rows_sorted == 0
    g[2], xupp[4] = 0.25, 1.0
    s, fix, info, _, _ = _search(bh, H, np.zeros((0, n)), xlow, xupp, x, g, 10.0, "sorted")
    s0, fix0, info0, _, _ = _search(bh, H, np.zeros((0, n)), xlow, xupp, x, g, 10.0, "stepwise")
    assert info["form"] == FORM_ROWS_SORTED and H.searches_rows_sorted == 1
    assert np.array_equal(fix, fix0) and info["n_hmul"] == info0["n_hmul"] and relnorm(s, s0) <= 1e-9
    H.close()


def test_nan_bound_past_the_scan_kernels_first_trip(bh):
    """The instance of test_cauchy_sorted_gpu.py (n = 1030, a NaN upper bound on variable 1027: the second trip of the scan kernel's
    threads over the indices).  (a) the variable free: handed back — the counter unchanged, code and bits the stepwise path's.
    (b) fixed at the start: the bound is never looked at — a sorted search, set and decisions of the restatement at this device's
    grid, the step within 1e-9 of it."""
    inst = rw.sc.nan_bound_past_the_first_trip(False)
    H = _handle(bh, inst)
    try:
        got = [_outcome(bh, H, inst, mode) for mode in ("stepwise", "sorted")]
        assert got[0] == got[1], [t[:1] + t[3:] for t in got]
        assert H.searches_rows_sorted == 0
        inst = rw.sc.nan_bound_past_the_first_trip(True)
        res = rw.rowsort_search(inst, grid=rw.grid_of(inst[0].shape[0], _n_cu(bh)))
        assert not res.handback
        s, fix, info, _, _ = _inst_search(bh, H, inst, "sorted")
        assert info["form"] == FORM_ROWS_SORTED and H.searches_rows_sorted == 1
        assert np.array_equal(fix, res.fix) and info["n_hmul"] == res.n_hmul, (info, res.n_hmul)
        assert relnorm(s, res.s) <= 1e-9, relnorm(s, res.s)
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------------------ 7. setter and getter, switch off
def test_setter_getter_and_switch_off(bh):
    lib = bh._lib.lib()
    J, C, xlow, xupp, x, g, delta = oracle_instance(700, 257, 1, 20, 0.3, 12)
    Z = np.zeros((0, 257))
    H = bh.AlHessian(J, C, 2.5)
    assert (H.cauchy_rows, H.cauchy_rows_served, H.searches_rows_sorted) == ("stepwise", True, 0)
    s0, f0, i0, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, None)          # the switch never touched: today's path
    assert i0["form"] == FORM_ROWSPACE
    H.set_cauchy_rows("sorted")
    for bad in (-1, 2, 7):
        assert lib.bh_hess_set_cauchy_rows(H._h, bad) == bh._lib.BH_ERR_INVALID_ARG
        assert H.cauchy_rows == "sorted"
    assert lib.bh_hess_set_cauchy_rows(None, 1) == bh._lib.BH_ERR_INVALID_ARG
    assert lib.bh_hess_get_cauchy_rows(None, None, None, None) == bh._lib.BH_ERR_INVALID_ARG
    assert lib.bh_hess_get_cauchy_rows(H._h, None, None, None) == 0
    m = ct.c_int32(-1)
    assert lib.bh_hess_get_cauchy_rows(H._h, ct.byref(m), None, None) == 0 and m.value == bh._lib.BH_CAUCHY_ROWS_SORTED
    with pytest.raises(ValueError):
        H.set_cauchy_rows("fast")
    s1, f1, i1, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
    assert i1["form"] == FORM_ROWS_SORTED and H.searches_rows_sorted == 1
    assert np.array_equal(f1, f0) and i1["n_hmul"] == i0["n_hmul"] and relnorm(s1, s0) <= 1e-9
    H.set_form("gram")
    assert H.cauchy_rows == "sorted" and H.gram_builds == 0          # remembered across bh_hess_set_form; builds nothing
    sg, fg, ig, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
    assert ig["form"] == FORM_ROWSPACE and H.searches_rows_sorted == 1          # a Gram-form handle: the path without the switch
    H.set_form("implicit")
    assert H.cauchy_rows == "sorted"
    s2, f2, i2, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "sorted")
    assert i2["form"] == FORM_ROWS_SORTED and np.array_equal(bits(s2), bits(s1)) and H.searches_rows_sorted == 2
    s3, f3, i3, _, _ = _search(bh, H, Z, xlow, xupp, x, g, delta, "stepwise")   # switch off again: form, launches and bits of the start
    assert i3 == i0 and np.array_equal(bits(s3), bits(s0)) and np.array_equal(f3, f0)
    H.close()
    wide = bh.AlHessian(np.zeros((2, 4097)), None, 0.0)
    assert not wide.cauchy_rows_served
    wide.close()


# ------------------------------------------------------------------------------------------------------------ 8. not served
@pytest.mark.parametrize("gram_handle,mA,n,form", [(True, 0, 200, FORM_ROWSPACE), (False, 1, 200, FORM_ROWSPACE_EQ), (False, 0, 4097, FORM_ROWSPACE)])
def test_not_served_is_silent_and_exact(bh, gram_handle, mA, n, form):
    """A Gram-form handle, one linear equality, a width just above the served limit: the switch changes nothing — same form and
    launches as without it, step and active set bit for bit."""
    J, C, xlow, xupp, x, g, delta = oracle_instance(60 if n > 4096 else 500, n, 1, 10, 0.3, 31 + mA)
    A = np.random.default_rng(7).standard_normal((mA, n))
    if mA:
        x = x - A.T @ np.linalg.solve(A @ A.T, A @ x)
        x = np.clip(x, -0.95, 0.95)
    H = bh.AlHessian(J, C, 2.5)
    if gram_handle:
        H.set_form("gram")
    s0, f0, i0, _, _ = _search(bh, H, A, xlow, xupp, x, g, delta, "stepwise")
    s1, f1, i1, _, _ = _search(bh, H, A, xlow, xupp, x, g, delta, "sorted")
    assert i0["form"] == form and i1 == i0, (i0, i1)
    assert np.array_equal(bits(s1), bits(s0)) and np.array_equal(f1, f0)
    assert H.searches_rows_sorted == 0 and H.cauchy_rows == "sorted" and H.cauchy_rows_served == (n <= 4096)
    H.close()


# ------------------------------------------------------------------------------------------------------------ 9. host and device entry points
def test_host_and_device_entry_points_agree(bh):
    lib = bh._lib.lib()
    n = 257
    J, C, xlow, xupp, x, g, delta = oracle_instance(700, n, 1, 20, 0.3, 12)
    H = bh.AlHessian(J, C, 2.5)
    s_h, fix_h, info_h, _, _ = _search(bh, H, np.zeros((0, n)), xlow, xupp, x, g, delta, "sorted")
    cons = bh.MixedConstraints(np.zeros((0, n)), None, None, l=xlow, u=xupp)
    dv = {k: bh.DeviceVector(n, v) for k, v in (("x", x), ("g", g), ("xl", xlow), ("xu", xupp), ("s", np.zeros(n)))}
    try:
        cons._sync()
        chunks = np.zeros((n + 63) // 64, dtype=np.uint64)
        nbp, nh = ct.c_int32(0), ct.c_int32(0)
        bh._lib.check(lib.bh_cauchy_step_dev(H.handle, cons._h, dv["x"].ptr, dv["g"].ptr, dv["xl"].ptr, dv["xu"].ptr, float(delta), dv["s"].ptr,
                                             bh._lib.ptr(chunks), ct.byref(nbp), ct.byref(nh)), "bh_cauchy_step_dev")
        s_d = dv["s"].download()
        fix_d = np.unpackbits(chunks.view(np.uint8), bitorder="little")[:n].astype(bool)
        assert bh.cauchy_info(cons)[0] == FORM_ROWS_SORTED
        assert np.array_equal(bits(s_d), bits(s_h)) and np.array_equal(fix_d, fix_h)
        assert (nbp.value, nh.value) == (info_h["n_breakpoints"], info_h["n_hmul"]) and H.searches_rows_sorted == 2
    finally:
        for v in dv.values():
            v.close()
        cons.close()
        H.close()


# ------------------------------------------------------------------------------------------------------------ 10. resident chain
class _Stepwise(HipOpsResident):
    rows = "stepwise"

    def new_hessian(self, J, C, mu):
        H = self.bh.AlHessian(J, C, mu)
        H.set_cauchy_rows(self.rows)
        return H


class _Sorted(_Stepwise):
    rows = "sorted"


def test_resident_inner_step_ends_at_the_same_active_set(bh):
    """One bh.inner_step (box constraints) with the switch on against the same call with it off: the same final active set and
    minor-loop log, s to 1e-6 (the rule of the other Cauchy forms' inner-step tests)."""
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
        s, pred = ops.inner_step(x, g, H, L0, cons, delta, 50, 0.1, 0.1, log)
        return s, pred, log, cons.fixvars.copy(), bh.cauchy_info(cons._dev)[0]

    s_off, pred_off, log_off, fix_off, form_off = run(_Stepwise(bh))
    s_on, pred_on, log_on, fix_on, form_on = run(_Sorted(bh))
    assert (form_off, form_on) == (FORM_ROWSPACE, FORM_ROWS_SORTED)
    assert np.array_equal(fix_on, fix_off)
    assert [e[1] for e in log_on] == [e[1] for e in log_off] and [e[2] for e in log_on] == [e[2] for e in log_off]
    note_tol("inner_step with the sorted rows Cauchy search: s vs the switch off, 1e-6", relnorm(s_on, s_off), 1e-6)
    assert relnorm(s_on, s_off) <= 1e-6 and pred_on == pytest.approx(pred_off, rel=1e-8)
