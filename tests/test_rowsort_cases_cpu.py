"""CPU proof of tests/rowsort_cases.py: the float64 restatement of the sorted rows form of the Cauchy search
(csrc/bh_cauchyrowsort.hip.h, bh_cauchy_info form 6) against the oracle's cauchy_step — bit for bit on the exact families, every
partial sum proved exact, to 1e-9 with the same active set and product count on the oracle cases of served width — and the five
value-only faults, each of which changes a result."""
import re

import numpy as np
import pytest

import gram_cases as gc
import refresh_cases as rc
import rowsort_cases as rw
import sorted_cases as sc
from _util import closed_form_cauchy_cases, relnorm
from test_sorted_cases_cpu import ORACLE_CASES, oracle_instance

SIZES = tuple(n for n in gc.K_SIZES if rw.served(n))


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _src(name):
    import os
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benlsip.jl_amd", "csrc", name)).read()


def _check_exact(c, prove=True, grid=None):
    J, C, mu, A, x, g, xlow, xupp, delta = c.inst
    res = rw.rowsort_search(c.inst, grid=grid)
    so, fo, po = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
    assert not res.handback and res.err == 0, c.name
    assert res.n_hmul == po and np.array_equal(res.fix, fo) and np.array_equal(bits(res.s), bits(so)), (c.name, res.n_hmul, po)
    led = gc.Ledger()
    if prove:
        rw.prove_exact(res, led)
    return res, led


def test_geometry_constants_are_the_kernels():
    hdr, plan, api = _src("bh_cauchyrowsort.hip.h"), _src("bh_cauchy_rows_plan.h"), _src("bh_api.hip")
    assert rw.T % 64 == 0 and rw.MAXN == rw.T * rw.EPT == 4096 and rw.R >= 1
    assert int(re.search(r"constexpr int64_t kCauchyRowsMaxN = (\d+);", plan).group(1)) == rw.MAXN
    assert "constexpr int RS_MAXN = RS_T * RS_EPT;" in hdr and "ld <= kCauchyRowsMaxN" in plan
    assert "std::min<int64_t>(groups, (int64_t)RS_GRID_PER_CU * g_ctx.n_cu)" in api and "(img_rows + RS_R - 1) / RS_R" in api
    assert SIZES == (1030, 4095, 4096) and not rw.served(4097)
    print("\n".join(rw.describe(n, gc.K_ROWS) for n in SIZES))


def test_closed_form_cases():
    for case in closed_form_cauchy_cases():
        inst = (np.eye(2), np.zeros((0, 2)), 0.0, None, np.zeros(2), case["g"], -np.ones(2), np.ones(2), case["delta"])
        res = rw.rowsort_search(inst)
        assert not res.handback and np.array_equal(bits(res.s), bits(case["s"])), (case["name"], res.s)
        assert np.array_equal(res.fix, case["fix"]) and res.n_hmul == case["n_hmul"], case["name"]


@pytest.mark.parametrize("n", SIZES)
def test_family_k_bit_for_bit_and_exact_in_any_order(n):
    worst = {}
    for c in gc.k_cases(n):
        res, led = _check_exact(c)
        for k, b in led.bits.items():
            worst[k] = max(worst.get(k, 0), b)
        other = rw.rowsort_search(c.inst, grid=3)                    # exact sums: another grid, the same bits
        assert np.array_equal(bits(other.s), bits(res.s)) and other.n_hmul == res.n_hmul
    print("n = %d: widest numerators (bits): %s" % (n, worst))
    assert max(worst.values()) <= gc.MANT


@pytest.mark.parametrize("order", ["drawn", "reversed"])
@pytest.mark.parametrize("rows,n,q,npass", [(24, 160, 0, 6), (43, 1030, 3, 100), (1, 33, 0, 3), (5, 257, 2, 128)])
def test_exact_instances_bit_for_bit(rows, n, q, npass, order):
    inst = rc.exact_instance(rows, n, q, npass)
    if order == "reversed":
        drawn = np.random.default_rng(1000).permutation(n)[:npass - 1][::-1]
        inst = rc.exact_instance(rows, n, q, npass, order=drawn)
    res, led = _check_exact(gc.KCase("exact", n, inst, ""))
    assert res.kstar >= 1 and max(led.bits.values()) <= gc.MANT


@pytest.mark.parametrize("n", (1030, 4096))
def test_edge_placements_bit_for_bit(n):
    names = []
    for c in rw.edge_cases(n):
        res, _ = _check_exact(c)
        names.append(c.name)
        t = res.terms
        if c.name.startswith("stop_after_rank_"):
            assert res.kstar == int(c.name.rsplit("_", 1)[1]) + 1
        if c.name == "infinite_tail":
            nfin = int(np.isfinite(t["T"]).sum())
            assert res.kstar == nfin == len(gc.k_hits(n)) and np.isinf(t["theta"][res.kstar])
        if c.name.startswith("tie_"):
            first, second = (int(v) for v in c.name.split("_")[1:])
            assert t["T"][first] == t["T"][second] and t["rank"][first] == 0 and t["rank"][second] == 1
    ties = [tuple(int(v) for v in nm.split("_")[1:]) for nm in names if nm.startswith("tie_")]
    own = [(rw.column_owner(a), rw.column_owner(b)) for a, b in ties]
    assert any(x[0] != y[0] and x[1] == y[1] and x[2] == y[2] for x, y in own)          # threads of one wave
    assert any(x[1] != y[1] and x[2] == y[2] for x, y in own)                           # waves
    assert any(x[2] != y[2] for x, y in own)                                            # chunks
    stops = sorted(int(nm.rsplit("_", 1)[1]) + 1 for nm in names if nm.startswith("stop_after_rank_"))
    assert {rw.EPT - 1, rw.EPT, rw.EPT + 1} <= set(stops)                               # the stop on both sides of a thread's edge


@pytest.mark.parametrize("n_cu", [2, 256])
def test_row_counts_around_the_group_and_workgroup_edges(n_cu):
    """The row counts of the GPU module at a small device and at 256 compute units: one row, the group edges, the first second group
    of a workgroup.  mu = 1/2 != 1 with q > 0."""
    n = 33
    for rows, q in rw.row_count_cases(n_cu=n_cu):
        q = min(q, rows - 1)
        inst = rc.exact_instance(rows, n, q, 6)
        grid = rw.grid_of(rows, n_cu=n_cu)
        res, led = _check_exact(gc.KCase("rows", n, inst, ""), grid=grid)
        assert res.terms["grid"] == grid <= rw.GRID_PER_CU * n_cu


def test_small_endings():
    for c in gc.k_all_fixed():                                        # rank nfree - 1 is reached: every variable ends fixed
        res, _ = _check_exact(c)
        assert res.fix.all() and res.n_hmul == c.n + 1 and res.kstar == res.terms["order"].size
    for n in (1030, 4096):
        res = rw.rowsort_search(gc.k_no_breakpoint(n).inst)
        assert not res.handback and res.err == 1 and res.n_hmul == 1 and not res.fix.any() and not res.s.any()


def test_non_finite_input_hands_back():
    rng = np.random.default_rng(3)
    n = 6
    J = rng.standard_normal((20, n)) / np.sqrt(20.0)
    g = rng.standard_normal(n)
    g[2] = np.nan
    assert rw.rowsort_search((J, None, 0.0, None, np.zeros(n), g, -np.ones(n), np.ones(n), 10.0)).handback
    g[2] = 0.5
    xupp = np.ones(n)
    xupp[4] = np.nan
    assert rw.rowsort_search((J, None, 0.0, None, np.zeros(n), g, -np.ones(n), xupp, 10.0)).handback


def test_nan_bound_past_the_first_trip_in_both_restatements():
    """sorted_cases.nan_bound_past_the_first_trip (n = 1030, xupp[1027] = NaN): free, both restatements hand back; fixed at the
    start, neither does — 277 decisions, s and the set those of the same instance with a finite bound."""
    assert sc.sorted_search(sc.nan_bound_past_the_first_trip(False)).handback
    assert rw.rowsort_search(sc.nan_bound_past_the_first_trip(False)).handback
    inst = sc.nan_bound_past_the_first_trip(True)
    xupp = inst[7].copy()
    xupp[1027] = 1.0
    for search in (sc.sorted_search, rw.rowsort_search):
        res, fin = search(inst), search(inst[:7] + (xupp,) + inst[8:])
        assert not res.handback and res.n_hmul == fin.n_hmul == 277
        assert np.array_equal(res.s, fin.s) and np.array_equal(res.fix, fin.fix) and res.fix[1027]


SERVED_ORACLE_CASES = [c for c in ORACLE_CASES if rw.served(c[1])]


@pytest.mark.parametrize("case", SERVED_ORACLE_CASES)
def test_oracle_cases(case):
    J, C, xlow, xupp, x, g, delta = oracle_instance(*case)
    so, fo, po = rc.oracle_step(J, C, 2.5, None, x, g, xlow, xupp, delta)
    res = rw.rowsort_search((J, C, 2.5, None, x, g, xlow, xupp, delta))
    assert not res.handback and res.err == 0
    assert np.array_equal(res.fix, fo) and res.n_hmul == po, (res.n_hmul, po)
    rel = relnorm(res.s, so)
    print("sorted rows form vs oracle, n = %d, %d passes: %.2e" % (case[1], po, rel))
    assert rel <= 1e-9, rel


@pytest.mark.parametrize("case", rw.LONG_CASES)
def test_long_searches_cross_the_wave_edges(case):
    """A stop beyond rank 64 EPT: the same set and count as the carried float64 search of the stepwise form (refresh_cases), the
    step within 1e-9; dropping the totals of the waves before a wave from the prefix scan changes the result."""
    J, C, xlow, xupp, x, g, delta = oracle_instance(*case)
    inst = (J, C, 2.5, None, x, g, xlow, xupp, delta)
    so, fo, po = rc.carried_search(J, C, 2.5, x, g, xlow, xupp, delta)
    res = rw.rowsort_search(inst)
    assert not res.handback and res.err == 0 and res.kstar > 64 * rw.EPT, res.kstar
    assert np.array_equal(res.fix, fo) and res.n_hmul == po, (res.n_hmul, po)
    assert relnorm(res.s, so) <= 1e-9
    if case != rw.LONG_CASES[1]:                                     # (with steps of 1e-8 phi' is g'd to rounding: only the interior stop shows it)
        return
    wrong = rw.rowsort_search(inst, fault="wave_prefix_dropped")
    assert wrong.handback or wrong.n_hmul != res.n_hmul or not np.array_equal(wrong.fix, res.fix) or not np.array_equal(bits(wrong.s), bits(res.s))


def test_fixed_at_the_start_at_kernel_width():
    c = rw.fixed_at_the_start(gc.k_cases(4096)[0])
    res, led = _check_exact(c)
    assert (res.terms["rank"] < 0).sum() > 1000 and res.kstar >= 1


def test_the_oracle_cases_are_the_ten_restricted_to_served_widths():
    assert len(ORACLE_CASES) == 10 and [c[1] for c in ORACLE_CASES if not rw.served(c[1])] == [4100, 8200]


@pytest.mark.parametrize("fault", rw.FAULTS)
def test_each_fault_changes_a_result(fault):
    """A wrong kernel of each kind gives another active set, count or step on at least one case the GPU module runs."""
    n = 1030
    k0 = gc.k_cases(n)[0]
    cases = {"tie_order": [c for c in gc.k_cases(n) if c.name.startswith("tie_")],
             "prefix_for_suffix": [k0], "missing_row_weight": [k0], "b_from_the_wrong_side": [k0], "row_group_dropped": [k0],
             "wave_prefix_dropped": [gc.KCase("long", 4096, (lambda J, C, xl, xu, x, g, dl: (J, C, 2.5, None, x, g, xl, xu, dl))(*oracle_instance(*rw.LONG_CASES[1])), "")]}[fault]
    changed = 0
    for c in cases:
        good = rw.rowsort_search(c.inst)
        wrong = rw.rowsort_search(c.inst, fault=fault)
        if wrong.handback or wrong.n_hmul != good.n_hmul or not np.array_equal(wrong.fix, good.fix) or not np.array_equal(bits(wrong.s), bits(good.s)):
            changed += 1
    assert changed == len(cases), (fault, changed, len(cases))
