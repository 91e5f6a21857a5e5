"""CPU proof of tests/rowsort_ranks_cases.py: the float64 restatement of the sorted rows form of the Cauchy search on a row-sharded
handle (bh_hess_set_cauchy_rows_ranks: every rank scans its own rows, the ranks' phi'' and X summed in rank order, the scan unchanged).
On the exact families of tests/rowsort_cases.py — every partial sum exact by the ledger, so in any association — worlds 1, 2, 3, 5, 8
give the bits of the one-rank restatement and of the oracle, shards with 0 and 1 rows and d_total < world included; on the oracle
instances the oracle's active set and count; and the three faults of the sharding each change a result."""
import numpy as np
import pytest

import gram_cases as gc
import refresh_cases as rc
import rowsort_cases as rw
import rowsort_ranks_cases as rr
from _util import closed_form_cauchy_cases, relnorm
from test_rowsort_cases_cpu import SERVED_ORACLE_CASES, SIZES, bits, _src
from test_sorted_cases_cpu import oracle_instance


def _same(a, b):
    return a.n_hmul == b.n_hmul and np.array_equal(a.fix, b.fix) and np.array_equal(bits(a.s), bits(b.s))


def _check_worlds(c, worlds=rr.WORLDS, prove=True):
    """Case c on every world: the bits, set and count of the one-rank restatement and of the oracle."""
    J, C, mu, A, x, g, xlow, xupp, delta = c.inst
    one = rw.rowsort_search(c.inst)
    so, fo, po = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
    assert not one.handback and one.err == 0 and one.n_hmul == po and np.array_equal(one.fix, fo) and np.array_equal(bits(one.s), bits(so)), c.name
    shapes = set()
    for world in worlds:
        res = rr.ranks_search(c.inst, world)
        assert not res.handback and res.err == 0 and _same(res, one), (c.name, world, res.n_hmul, one.n_hmul)
        assert sum(res.terms["rank_rows"]) == J.shape[0] + (C.shape[0] if C is not None else 0) and len(res.terms["rank_rows"]) == world
        shapes.update(res.terms["rank_rows"])
        if prove and world == worlds[-1]:
            rw.prove_exact(res, gc.Ledger())                         # every sum over rows exact in any order: so over ranks
    return shapes


def test_the_sharding_rule_is_the_library_s():
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benlsip.jl_amd", "distributed.py")).read()
    assert "base, extra = divmod(int(d_total), int(nranks))" in src and "lo = rank * base + min(rank, extra)" in src
    assert "hi = lo + base + (1 if rank < extra else 0)" in src
    for d, world in ((0, 3), (2, 3), (9, 8), (700, 3), (4096, 8)):
        spans = [rr.row_shard(d, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == d and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1
    api, comm = _src("bh_api.hip"), _src("bh_comm.hip.h")
    assert "H->q_eff = (g_ctx.rank == 0) ? H->q : 0;" in api           # the rows of C on rank 0 only
    assert "BH_TRY(allreduce_inplace(ra.red, 2 * ld, H));" in api
    assert "double2 t = sm[0][cl];" in comm and "for (int r = 1; r < pa.nranks; ++r) { t.x += sm[r][cl].x; t.y += sm[r][cl].y; }" in comm


def test_closed_form_cases_on_every_world():
    for case in closed_form_cauchy_cases():
        inst = (np.eye(2), np.zeros((0, 2)), 0.0, None, np.zeros(2), case["g"], -np.ones(2), np.ones(2), case["delta"])
        for world in rr.WORLDS:                                      # d_total = 2: ranks without rows from world 3 on
            res = rr.ranks_search(inst, world)
            assert not res.handback and np.array_equal(bits(res.s), bits(case["s"])), (case["name"], world, res.s)
            assert np.array_equal(res.fix, case["fix"]) and res.n_hmul == case["n_hmul"], (case["name"], world)


@pytest.mark.parametrize("n", SIZES)
def test_family_k_bit_for_bit_on_every_world(n):
    for c in gc.k_cases(n):
        _check_worlds(c)


@pytest.mark.parametrize("rows,n,q,npass", [(24, 160, 0, 6), (43, 1030, 3, 100), (1, 33, 0, 3), (5, 257, 2, 128), (12, 33, 3, 6)])
def test_exact_instances_bit_for_bit_on_every_world(rows, n, q, npass):
    """Few rows: shards of 0 and 1 rows, d_total < world (1 and 3 rows of J over up to 8 ranks), 9 rows of J over 8 ranks."""
    shapes = _check_worlds(gc.KCase("exact", n, rc.exact_instance(rows, n, q, npass), ""))
    if rows - q < 8:
        assert 0 in shapes
    if (rows, q) == (12, 3):
        assert {1, 2} <= shapes                                      # world 8: every rank holds 1 or 2 rows of J, around RS_R


@pytest.mark.parametrize("n", (1030, 4096))
def test_edge_placements_and_fixed_at_the_start_on_every_world(n):
    for c in rw.edge_cases(n) + [rw.fixed_at_the_start(gc.k_cases(n)[0])]:
        _check_worlds(c, worlds=(2, 8), prove=False)


def test_a_rank_makes_a_second_trip_through_its_row_loop():
    """More than 2 RS_R n_cu rows on one rank at a small device (n_cu = 2): the persistent grid of that rank wraps; still exact."""
    n, n_cu = 33, 2
    rows = 3 * (2 * rw.R * rw.GRID_PER_CU * n_cu + 2) + 1             # q = 1: 30 rows of J, 10 on each of three ranks
    inst = rc.exact_instance(rows, n, 1, 6)
    one = rw.rowsort_search(inst)
    for world in (2, 3):
        res = rr.ranks_search(inst, world, n_cu=n_cu)
        assert min(res.terms["rank_rows"]) > 2 * rw.R * rw.GRID_PER_CU * n_cu and _same(res, one)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_the_exact_cases_of_the_gpu_module_are_exact(world):
    """The instances tests/test_cauchy_rowsort_ranks_gpu.py holds to the oracle's bits, at the row counts of a 256-CU device."""
    names = []
    for name, kind, inst in rr.gpu_cases(world, n_cu=256):
        names.append(name)
        if kind == "exact":
            shapes = _check_worlds(gc.KCase(name, inst[0].shape[1], inst, ""), worlds=(world,))
            if name == "second_trip":
                assert min(shapes) > 2 * rw.R * rw.GRID_PER_CU * 256
            if name == "rank_without_rows":
                assert 0 in shapes
            if name == "one_or_two_rows":
                assert shapes == {1, 2 + 3}                          # rank 0: its two rows of J and the three of C; every other rank one
    assert ("rank_without_rows" in names) == (world == 3) and ("one_or_two_rows" in names) == (world == 8)


def test_small_endings_on_every_world():
    for c in gc.k_all_fixed():
        _check_worlds(c, prove=False)
    res = rr.ranks_search(gc.k_no_breakpoint(1030).inst, 3)
    assert not res.handback and res.err == 1 and res.n_hmul == 1 and not res.fix.any() and not res.s.any()


def test_non_finite_input_hands_back_on_every_rank_count():
    rng = np.random.default_rng(3)
    n = 6
    J = rng.standard_normal((20, n)) / np.sqrt(20.0)
    g = rng.standard_normal(n)
    g[2] = np.nan
    for world in (2, 8):
        assert rr.ranks_search((J, None, 0.0, None, np.zeros(n), g, -np.ones(n), np.ones(n), 10.0), world).handback
    g[2] = 0.5
    Jn = J.copy()
    Jn[19, 1] = np.nan                                               # a NaN in the last rank's rows reaches the scan through the sum
    assert rr.ranks_search((Jn, None, 0.0, None, np.zeros(n), g, -np.ones(n), np.ones(n), 10.0), 3).handback


@pytest.mark.parametrize("case", SERVED_ORACLE_CASES)
def test_oracle_cases_on_every_world(case):
    J, C, xlow, xupp, x, g, delta = oracle_instance(*case)
    so, fo, po = rc.oracle_step(J, C, 2.5, None, x, g, xlow, xupp, delta)
    for world in rr.WORLDS:
        res = rr.ranks_search((J, C, 2.5, None, x, g, xlow, xupp, delta), world)
        assert not res.handback and res.err == 0
        assert np.array_equal(res.fix, fo) and res.n_hmul == po, (world, res.n_hmul, po)
        rel = relnorm(res.s, so)
        assert rel <= 1e-9, (world, rel)


@pytest.mark.parametrize("fault", rr.FAULTS)
def test_each_fault_changes_a_result(fault):
    """A wrong sharding of each kind gives another active set, count or step on a case the GPU module runs (q = 3 rows of C)."""
    k0 = gc.k_cases(1030)[0]
    changed = 0
    for world in (2, 3, 8):
        good = rr.ranks_search(k0.inst, world)
        wrong = rr.ranks_search(k0.inst, world, fault=fault)
        changed += 1 if wrong.handback or not _same(wrong, good) else 0
    assert changed == 3, (fault, changed)
