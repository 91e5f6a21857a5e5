"""CPU proof of tests/sorted_cases.py: the float64 restatement of the sorted Cauchy search (csrc/bh_cauchysort.hip.h, bh_cauchy_info
form 5) against the oracle's cauchy_step — bit for bit on the exact families, to 1e-9 with the same active set and product count on
the oracle cases — and the four value-only faults, each of which changes a result."""
import re

import numpy as np
import pytest

import benlsip_ref as R
import gram_cases as gc
import refresh_cases as rc
import sorted_cases as sc
from _util import closed_form_cauchy_cases, relnorm


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _src(name):
    import os
    return open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benlsip.jl_amd", "csrc", name)).read()


def _check_exact(c, G=None, M=None, prove=True):
    J, C, mu, A, x, g, xlow, xupp, delta = c.inst
    res = sc.sorted_search(c.inst, G=G)
    so, fo, po = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
    assert not res.handback and res.err == 0, c.name
    assert res.n_hmul == po and np.array_equal(res.fix, fo) and np.array_equal(bits(res.s), bits(so)), (c.name, res.n_hmul, po)
    led = gc.Ledger()
    if prove:
        sc.prove_exact(c.inst, res, led, M=M)
    return res, led


def test_geometry_constants_are_the_kernels():
    hdr = _src("bh_cauchysort.hip.h")
    assert (sc.RANK_T, sc.RANK_TILE, sc.ROW_T, sc.ROW_CPT, sc.ROW_R, sc.SCAN_T, sc.MAX_PANELS) == (256, 512, 512, 4, 4, 1024, 4)
    assert sc.PANEL == 4096 and sc.MAX_PANELS * sc.PANEL == 16384                      # the Gram form's own limit
    assert re.search(r"const int E = \(n \+ 1 \+ T - 1\) / T;", hdr)
    assert re.search(r"const int key_tiles = \(int\)\(\(H->n \+ CS_RANK_TILE - 1\) / CS_RANK_TILE\);", _src("bh_api.hip"))
    assert re.search(r"sa\.npanels = \(int\)\(\(ld / 2 \+ CS_ROW_T \* CS_ROW_CPT - 1\) / \(CS_ROW_T \* CS_ROW_CPT\)\);", _src("bh_api.hip"))
    print("\n".join(sc.describe(n) for n in gc.K_SIZES))


def test_closed_form_cases():
    for case in closed_form_cauchy_cases():
        inst = (np.eye(2), np.zeros((0, 2)), 0.0, None, np.zeros(2), case["g"], -np.ones(2), np.ones(2), case["delta"])
        res = sc.sorted_search(inst)
        assert not res.handback and np.array_equal(bits(res.s), bits(case["s"])), (case["name"], res.s)
        assert np.array_equal(res.fix, case["fix"]) and res.n_hmul == case["n_hmul"], case["name"]


@pytest.mark.parametrize("n", gc.K_SIZES)
def test_family_k_bit_for_bit_and_exact_in_any_order(n):
    M, G, worst = None, None, {}
    for c in gc.k_cases(n):
        if M is None:
            M = gc.gram_matrix(c.inst, gc.Ledger())
            G = M["dense"]
        res, led = _check_exact(c, G=G, M=M)
        for k, b in led.bits.items():
            worst[k] = max(worst.get(k, 0), b)
    print("n = %d: widest numerators (bits): %s" % (n, worst))
    assert max(worst.values()) <= gc.MANT


@pytest.mark.parametrize("n", sc.EDGE_SIZES)
def test_edge_placements_bit_for_bit(n):
    M = G = None
    names = []
    for c in sc.edge_cases(n):
        if M is None:
            M = gc.gram_matrix(c.inst, gc.Ledger())
            G = M["dense"]
        res, _ = _check_exact(c, G=G, M=M)
        names.append(c.name)
        t = res.terms
        if c.name == "rank0_on_the_last_index":
            assert list(t["order"][:6]) == [n - 1, sc.RANK_TILE - 1, sc.RANK_TILE, sc.RANK_T - 1, sc.RANK_T, 0] and res.kstar == 6
            assert t["rank"][n - 1] == 0
        if c.name == "row_group_edges":
            last = n - 1
            want = list(dict.fromkeys([sc.ROW_R - 1, sc.ROW_R, 2 * sc.ROW_R - 1, last - last % sc.ROW_R, last]))
            assert list(t["order"][:len(want)]) == want and res.kstar == len(want)
        if c.name.startswith("stop_after_rank_"):
            assert res.kstar == int(c.name.rsplit("_", 1)[1]) + 1
        if c.name == "infinite_tail":
            nfin = int(np.isfinite(t["T"]).sum())
            assert res.kstar == nfin == len(gc.k_hits(n)) and np.isinf(t["theta"][res.kstar])   # the stop behind the last finite breakpoint
            tail = t["order"][nfin:]
            assert tail.size == n - nfin and np.all(np.diff(tail) > 0) and np.all(t["d"][tail] != 0.0)      # T = Inf: index order, d != 0
            assert np.all(res.s[tail] != 0.0)
        if c.name.startswith("tie_"):
            first, second = (int(v) for v in c.name.split("_")[1:])
            assert t["T"][first] == t["T"][second] and t["rank"][first] == 0 and t["rank"][second] == 1
    ties = [tuple(int(v) for v in nm.split("_")[1:]) for nm in names if nm.startswith("tie_")]
    assert any(a < sc.RANK_TILE <= b for a, b in ties) and any(a < sc.RANK_T <= b < sc.RANK_TILE for a, b in ties) and (5, 9) in ties
    assert "row_group_edges" in names


def test_small_endings():
    for c in gc.k_all_fixed():                                        # rank nfree - 1 is reached: every variable ends fixed
        res, _ = _check_exact(c)
        assert res.fix.all() and res.n_hmul == c.n + 1 and res.kstar == res.terms["order"].size
    for n in (1030, 4097):
        res = sc.sorted_search(gc.k_no_breakpoint(n).inst)
        assert not res.handback and res.err == 1 and res.n_hmul == 1 and not res.fix.any() and not res.s.any()


def test_non_finite_input_hands_back():
    rng = np.random.default_rng(3)
    n = 6
    J = rng.standard_normal((20, n)) / np.sqrt(20.0)
    g = rng.standard_normal(n)
    g[2] = np.nan
    res = sc.sorted_search((J, None, 0.0, None, np.zeros(n), g, -np.ones(n), np.ones(n), 10.0))
    assert res.handback


# d, n, q, nact, delta / ||g||, seed, scale of J, column scaling over three decades (tests/test_cauchy_gram_gpu.py)
ORACLE_CASES = [(90, 33, 2, 3, 0.1, 11, 1.0, False), (700, 257, 1, 20, 0.3, 12, 1.0, False), (3000, 1024, 0, 100, 1.0, 13, 1.0, False),
                (257, 4100, 3, 50, 0.1, 14, 1.0, False), (5, 3, 1, 0, 0.5, 15, 1.0, False),
                (1, 1, 0, 0, 0.1, 16, 1.0, False), (37, 5, 2, 1, 0.1, 17, 1.0, False), (2000, 512, 0, 40, 0.2, 5, 1.0, False),
                (400, 150, 1, 10, 0.3, 18, 1.0, True),
                (300, 8200, 2, 100, 0.005, 21, 3.0, False)]


def oracle_instance(d, n, q, nact, delta_factor, seed, jscale=1.0, scaled=False):
    """The generator of tests/test_cauchy_gram_gpu.py (same order of draws)."""
    rng = np.random.default_rng(seed)
    J = jscale * rng.standard_normal((d, n)) / np.sqrt(d)
    C = rng.standard_normal((q, n))
    xlow, xupp = -np.ones(n), np.ones(n)
    x = np.clip(0.5 * rng.standard_normal(n), -0.95, 0.95)
    act = rng.choice(n, nact, replace=False)
    x[act] = np.where(rng.random(nact) < 0.5, -1.0, 1.0)
    g = rng.standard_normal(n)
    if scaled:
        J = J * np.logspace(0.0, -3.0, n)[None, :]
    return J, C, xlow, xupp, x, g, delta_factor * float(np.linalg.norm(g))


@pytest.mark.parametrize("case", ORACLE_CASES)
def test_oracle_cases(case):
    J, C, xlow, xupp, x, g, delta = oracle_instance(*case)
    so, fo, po = rc.oracle_step(J, C, 2.5, None, x, g, xlow, xupp, delta)
    res = sc.sorted_search((J, C, 2.5, None, x, g, xlow, xupp, delta))
    assert not res.handback and res.err == 0
    assert np.array_equal(res.fix, fo) and res.n_hmul == po, (res.n_hmul, po)
    rel = relnorm(res.s, so)
    print("sorted form vs oracle, n = %d, %d passes: %.2e" % (case[1], po, rel))
    assert rel <= 1e-9, rel


@pytest.mark.parametrize("fault", sc.FAULTS)
def test_each_fault_changes_a_result(fault):
    """A wrong kernel of each kind gives another active set, count or step on at least one case the GPU module runs."""
    n = 1030
    cases = {"tie_order": [c for c in gc.k_cases(n) if c.name.startswith("tie_")],
             "own_term_in_U": [gc.k_cases(n)[0]],
             "prefix_for_suffix": [gc.k_cases(n)[0]],
             "b_from_the_wrong_side": [gc.k_cases(n)[0]]}[fault]
    changed = 0
    for c in cases:
        good = sc.sorted_search(c.inst)
        wrong = sc.sorted_search(c.inst, fault=fault)
        if wrong.handback or wrong.n_hmul != good.n_hmul or not np.array_equal(wrong.fix, good.fix) or not np.array_equal(bits(wrong.s), bits(good.s)):
            changed += 1
    assert changed == len(cases), (fault, changed, len(cases))
