"""The sorted rows form of the box-constrained Cauchy search on a ROW-SHARDED implicit handle (bh_hess_set_cauchy_rows_ranks;
csrc/bh_api.hip: cauchy_launch_sorted) restated in float64 NumPy on top of tests/rowsort_cases.py, which is not edited.  Helper
of tests/test_cauchy_rowsort_ranks_gpu.py, proved on the CPU by tests/test_rowsort_ranks_cases_cpu.py.  Not a test.

    1. the rows of J are sharded by the rule of bh.row_shard; the rows of C (weight mu) are on rank 0 only, behind its rows of J
    2. per rank: cauchy_rowsort_rows_kernel as it is (rowsort_cases.row_scan) on grid_of(rows of the rank) workgroups — a rank
       without rows: a grid of 1, one slab of +0 — and cauchy_rowsort_reduce_kernel, the slabs in ascending order from +0
    3. reduce_exchange_kernel with G = 0: the ranks' phi'' and X in rank order — rank 0's value first, then += rank r — and then
       the scan of rowsort_cases.rowsort_search, unchanged

Step 3 reuses rowsort_search itself: while it runs, its row_scan is replaced by one that returns the per-rank sums as `world` slabs;
its own kernel-3 loop (+0, + slab 0, + slab 1, ...) is then the sum in rank order (+0 + v = v bit for bit: no per-rank sum is -0,
each starts from +0), and everything behind it is the one-rank code."""
import numpy as np

import rowsort_cases as rw

FAULTS = ("rank_dropped", "c_rows_on_every_rank", "ranks_summed_into_the_wrong_segment")
WORLDS = (1, 2, 3, 5, 8)


def row_shard(d_total, rank, world):
    """benlsip.jl_amd/distributed.py: row_shard — contiguous blocks, the first d_total % world ranks get one extra row."""
    base, extra = divmod(int(d_total), int(world))
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def rank_rows(d, q, world, fault=None):
    """Per rank the indices into the image [J; C] of the rows it scans, in its own order: its rows of J, then (rank 0) those of C."""
    out = []
    for r in range(world):
        lo, hi = row_shard(d, r, world)
        idx = list(range(lo, hi))
        if r == 0 or fault == "c_rows_on_every_rank":
            idx += list(range(d, d + q))
        out.append(np.asarray(idx, dtype=np.int64))
    return out


def gpu_cases(world, n_cu=256, full_width=True):
    """The instances of tests/test_cauchy_rowsort_ranks_gpu.py on `world` ranks of a device with n_cu compute units, the smallest at
    which the sharded form can still go wrong: [(name, kind, inst)], kind "exact" (bit for bit against the oracle: proved exact by
    tests/test_rowsort_ranks_cases_cpu.py) or "oracle" (random data: the oracle's set and count, the step to 1e-9).
    full_width = False leaves out the n = 4096 instance: the GPU module runs it where the exchange is an ncclAllReduce and keeps it away
    from several processes that share ONE device over the peer buffers (see its docstring)."""
    import refresh_cases as rc
    from test_sorted_cases_cpu import oracle_instance
    J, C, xlow, xupp, x, g, delta = oracle_instance(700, 257, 1, 20, 0.3, 12)
    trip = 2 * rw.R * rw.GRID_PER_CU * n_cu                          # rows of one rank beyond which its persistent row loop has made a second trip
    out = [("oracle_257", "oracle", (J, C, 2.5, None, x, g, xlow, xupp, delta)),               # the instance of test_cauchy_rowsort_gpu.py
           ("full_width_few_rows", "exact", rc.exact_instance(24 + 3, 4096, 3, 100)),          # n = 4096, d_total = 24
           ("second_trip", "exact", rc.exact_instance(world * (trip + 3) + 1, 64, 1, 6))]      # n = 64, more than `trip` rows on every rank
    if not full_width:
        del out[1]
    if world == 3:
        out.append(("rank_without_rows", "exact", rc.exact_instance(2 + 1, 33, 1, 4)))         # d_total = 2 over 3 ranks
    if world == 8:
        out.append(("one_or_two_rows", "exact", rc.exact_instance(9 + 3, 33, 3, 6)))           # d_total = 9 over 8 ranks, around RS_R = 2
    return out


def ranks_search(inst, world, fault=None, n_cu=256):
    """rowsort_search with the rows of J over `world` ranks.  terms["grid"] = world; terms["rank_rows"]: rows scanned per rank."""
    assert fault is None or fault in FAULTS, fault
    J, C = inst[0], inst[1]
    d, q = J.shape[0], (C.shape[0] if C is not None else 0)
    shards = rank_rows(d, q, world, fault)
    one_rank_scan = rw.row_scan

    def sharded_scan(Jt, w, dr, br, grid, scan_fault=None, rows_per_step=256):
        assert grid == world and Jt.shape[0] == d + q
        per_rank = np.zeros((world, 2, rw.MAXN))
        for r, idx in enumerate(shards):
            g_r = rw.grid_of(idx.size, n_cu)                          # (no rows: 1)
            slabs = one_rank_scan(Jt[idx], w[idx], dr, br, g_r, None, rows_per_step)
            red = np.zeros((2, rw.MAXN))
            for gi in range(g_r):                                    # kernel 3 of rank r: ascending from +0
                red = red + slabs[gi]
            if fault == "ranks_summed_into_the_wrong_segment" and r == world - 1:
                red = red[::-1].copy()                               # phi'' of rank r added into X and X into phi''
            if fault == "rank_dropped" and r == world - 1:
                red[:] = 0.0
            per_rank[r] = red
        return per_rank

    rw.row_scan = sharded_scan
    try:
        res = rw.rowsort_search(inst, grid=world)
    finally:
        rw.row_scan = one_rank_scan
    res.terms["rank_rows"] = [int(i.size) for i in shards]
    return res
