"""GPU tests of the sorted rows form of the box-constrained Cauchy search on a ROW-SHARDED implicit handle
(bh_hess_set_cauchy_rows_ranks, bh_cauchy_info form 6 with a communicator): every rank scans its own rows, ONE
all-reduce of 2 ld doubles sums phi'' and X in rank order, the scan runs replicated.  Several processes on the one GPU of the test box
over both transports of tests/test_multirank_gpu.py (peer buffers; the staged stand-in behind the RCCL call site), every rank a fresh
child process (tests/multirank/rowsort_worker.py).  Checked: form 6 and exactly one collective per search on every rank, replicas bit
for bit, the oracle's and the one-process form's bits on exact data, the oracle's set and count and the step to 1e-9 on random data.
What is shown is correctness and COUNTS (launches, collectives): several processes on one GPU measure no several-rank time.

The n = 4096 instance runs where the exchange is an ncclAllReduce (the staged stand-in, the real librccl) and not on several processes
that share ONE device over the peer buffers.  At that width the exchange is 256 workgroups per process, each waiting on the device for
its peers, and between three processes on one device it ran into its time-out (BH_ERR_RCCL: by design an error, not a hang); between
two it did not.  The same happens on a path that does not involve this form: H*v at n = 8192 over three such processes, the same
256-workgroup exchange, times out in its first products.  So it is a limit of the peer-buffer exchange between processes that share a device (the cause is
not established), not of the search, and narrower exchanges (n = 257, n = 64, n = 33) run here with up to 8 processes (DESIGN.md §7:
the known limit of the peer buffers between processes that share a device).  By that account two processes at full width are a matter of
placement and timing as well — one early rank is 256 waiting workgroups on 256 compute units, and cauchy_rowsort_rows_kernel needs a unit
to itself — so that case is not kept as a test either."""
import ctypes as ct
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import refresh_cases as rc
import rowsort_ranks_cases as rr
import test_multirank_gpu as mr
from _util import note_tol, relnorm

pytestmark = pytest.mark.gpu

FORM_ROWSPACE, FORM_ROWS_SORTED = 1, 6
REC = ("code", "form", "n_launches", "n_hmul", "n_breakpoints", "d_allreduce", "d_jv", "d_hmul", "d_sorted")
LIMIT = 150                                                          # seconds per run_ranks: process start-up and bh.init dominate


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rec(z, key):
    return dict(zip(REC, (int(v) for v in z[key + "_rec"])))


def load(tmp_path, mode, world):
    return [np.load(os.path.join(tmp_path, "rowsort_%s_rank%d.npz" % (mode, r))) for r in range(world)]


def replicas_agree(res, key):
    for r in range(1, len(res)):
        assert np.array_equal(bits(res[0][key + "_s"]), bits(res[r][key + "_s"])), "rank %d differs from rank 0 in the step of %s" % (r, key)
        assert np.array_equal(res[0][key + "_fix"], res[r][key + "_fix"]), (r, key)
        assert np.array_equal(res[0][key + "_rec"], res[r][key + "_rec"]), (r, key, res[0][key + "_rec"], res[r][key + "_rec"])


@functools.lru_cache(maxsize=None)
def _oracle(world, n_cu, full_width):
    """name -> (kind, inst, the oracle's (step, set, products)); once per world."""
    out = {}
    for name, kind, inst in rr.gpu_cases(world, n_cu, full_width):
        J, C, mu, A, x, g, xlow, xupp, delta = inst
        out[name] = (kind, inst, rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta))
    return out


def _one_process(bh, inst):
    """Form 6 in this process, no communicator: (step, set, record of the call)."""
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    H = bh.AlHessian(J, C if C is not None and C.shape[0] else None, mu)
    H.set_cauchy_rows("sorted")
    cons = bh.MixedConstraints(np.zeros((0, J.shape[1])), None, None, l=xlow, u=xupp)
    try:
        s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
        return s, np.asarray(cons.fixvars, dtype=bool).copy(), info
    finally:
        cons.close()
        H.close()


# ------------------------------------------------------------------------------------------------------------ 1. the shapes, both transports
@pytest.mark.parametrize("comm,world", [("ipc", 2), ("ipc", 3), ("staged", 2), ("ipc", 8)])
def test_row_sharded_sorted_search(bh, tmp_path, comm, world):
    """Per shape of rowsort_ranks_cases.gpu_cases (n = 257 with d_total = 700, q = 1; n = 4096 with d_total = 24 — over the RCCL call site
    only, see the module's docstring; n = 64 with a second trip
    of every rank's row loop; d_total = 2 over 3 ranks; d_total = 9 over 8 ranks) on every rank: form 6, searches_rows_sorted + 1,
    stats.n_allreduce + EXACTLY 1, n_jv + 1, n_hmul + 0; the exchange is one launch more than one process enqueues over the peer buffers
    and none over the RCCL call site; a repeated search has the same bits; with the switch at 0 on the same handle form 1 and at least
    one collective per pass.  Replicas bit for bit; exact data: the oracle's and the one-process form's bits; random data: the
    oracle's set and count, the step within 1e-9."""
    full_width = comm != "ipc"
    mr.run_ranks("rowsort_worker.py", world, tmp_path, comm, extra=["cases"] + ([] if full_width else ["narrow"]), timeout=LIMIT)
    res = load(tmp_path, "cases", world)
    n_cu = int(res[0]["n_cu"])
    cases = _oracle(world, n_cu, full_width)
    assert ("full_width_few_rows" in cases) == full_width
    assert all(int(z["n_cu"]) == n_cu for z in res)
    for name, (kind, inst, (s_ref, fix_ref, passes)) in cases.items():
        what = "%s x%d %s" % (comm, world, name)
        rows = [int(z[name + "_rows"]) for z in res]
        assert sum(rows) == inst[0].shape[0], (what, rows)
        if name == "rank_without_rows":
            assert rows == [1, 1, 0]
        if name == "one_or_two_rows":
            assert rows == [2, 1, 1, 1, 1, 1, 1, 1]
        if name == "second_trip":
            assert min(rows) > 2 * rr.rw.R * rr.rw.GRID_PER_CU * n_cu, (what, rows)
        for key in (name + "_on", name + "_again", name + "_off"):
            replicas_agree(res, key)
        z = res[0]
        on, again, off = rec(z, name + "_on"), rec(z, name + "_again"), rec(z, name + "_off")
        s, fix = z[name + "_on_s"], z[name + "_on_fix"]
        s1, fix1, info1 = _one_process(bh, inst)
        print("[%s] %d passes: form %d, %d launches (one process: %d), %d all-reduce; switch off: form %d, %d launches, %d all-reduces"
              % (what, on["n_hmul"], on["form"], on["n_launches"], info1["n_launches"], on["d_allreduce"], off["form"], off["n_launches"], off["d_allreduce"]))
        assert (on["code"], on["form"], on["d_sorted"]) == (0, FORM_ROWS_SORTED, 1), (what, on)
        assert on["d_allreduce"] == 1, (what, on)                    # one collective per search, whatever its length
        assert (on["d_jv"], on["d_hmul"]) == (1, 0), (what, on)
        assert info1["form"] == FORM_ROWS_SORTED and on["n_launches"] == info1["n_launches"] + (1 if comm == "ipc" else 0), (what, on, info1)
        assert again == on and np.array_equal(bits(z[name + "_again_s"]), bits(s)) and np.array_equal(z[name + "_again_fix"], fix), what
        # the switch at 0: today's path — the stepwise row-space form, one collective per pass at the least
        assert (off["code"], off["form"], off["d_sorted"]) == (0, FORM_ROWSPACE, 0) and off["d_allreduce"] >= off["n_hmul"] >= 1, (what, off)
        assert (off["n_hmul"], off["n_breakpoints"]) == (on["n_hmul"], on["n_breakpoints"]) and np.array_equal(z[name + "_off_fix"], fix), (what, on, off)
        assert relnorm(z[name + "_off_s"], s) <= 1e-9, what
        # against the oracle on the unsharded instance and the one-process form
        assert np.array_equal(fix, fix_ref), (what, np.flatnonzero(fix != fix_ref)[:8])
        assert (on["n_hmul"], on["n_breakpoints"]) == (passes, passes - 1) == (info1["n_hmul"], info1["n_breakpoints"]), (what, on, passes, info1)
        assert np.array_equal(fix1, fix), what
        if kind == "exact":
            assert np.array_equal(bits(s), bits(s_ref)), (what, np.flatnonzero(bits(s) != bits(s_ref))[:8])
            assert np.array_equal(bits(s), bits(s1)), (what, np.flatnonzero(bits(s) != bits(s1))[:8])
        else:
            rel = relnorm(s, s_ref)
            note_tol("row-sharded cauchy_step from one sorted sweep over J: step vs oracle, 1e-9", rel, 1e-9, what)
            assert rel <= 1e-9, (what, rel)
            assert relnorm(s, s1) <= 1e-9, what


# ------------------------------------------------------------------------------------------------------------ 2. hand-back
def test_nan_in_g_is_handed_back_by_every_rank(tmp_path):
    """A NaN in g on a free variable (n = 6, two ranks): every rank hands back together, reports the stepwise form, counts no sorted
    search and returns the bits (or the code) of the stepwise path; no rank waits for another (the workers exit 0 within the
    limit); the handle then serves a finite call in the sorted form."""
    world = 2
    mr.run_ranks("rowsort_worker.py", world, tmp_path, "ipc", extra=["nan"], timeout=LIMIT)
    res = load(tmp_path, "nan", world)
    for key in ("nan_off", "nan_on", "finite_on"):
        replicas_agree(res, key)
    z = res[0]
    off, on, fin = rec(z, "nan_off"), rec(z, "nan_on"), rec(z, "finite_on")
    assert off["form"] == FORM_ROWSPACE and on["form"] == FORM_ROWSPACE and on["d_sorted"] == 0, (off, on)
    assert (on["code"], on["n_hmul"], on["n_breakpoints"]) == (off["code"], off["n_hmul"], off["n_breakpoints"]), (off, on)
    assert np.array_equal(bits(z["nan_on_s"]), bits(z["nan_off_s"])) and np.array_equal(z["nan_on_fix"], z["nan_off_fix"])
    assert on["d_allreduce"] >= 1                                     # the one exchange of the sorted attempt, then the stepwise path's own
    assert (fin["code"], fin["form"], fin["d_sorted"], fin["d_allreduce"]) == (0, FORM_ROWS_SORTED, 1, 1), fin


# ------------------------------------------------------------------------------------------------------------ 3. the real librccl
def test_one_rank_communicator_over_the_real_librccl(tmp_path):
    """BH_FORCE_COMM=1 BH_COMM=rccl (as tests/multirank/rccl_one_rank_worker.py): a one-rank communicator of the real librccl.  With the
    ranks switch on: form 6 with the communicator active, one ncclAllReduce (stats.n_allreduce + 1, no launch more than without a
    communicator), the bits of the no-communicator form-6 search on an exact instance; with it off: the stepwise path."""
    env = {k: v for k, v in os.environ.items() if k not in ("BH_RCCL_LIB",)}
    env.update(BH_FORCE_COMM="1", BH_COMM="rccl")
    out = subprocess.run([sys.executable, os.path.join(mr.MR, "rowsort_worker.py"), "0", "1", str(tmp_path), "rccl_one"], env=env,
                         capture_output=True, text=True, timeout=LIMIT)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    z = load(tmp_path, "rccl_one", 1)[0]
    alone, off, on = rec(z, "alone"), rec(z, "rccl_off"), rec(z, "rccl_on")
    assert z["comm"].tolist() == [0, 1]
    assert (alone["code"], alone["form"], alone["d_allreduce"], alone["d_sorted"]) == (0, FORM_ROWS_SORTED, 0, 1), alone
    assert (off["code"], off["form"], off["d_sorted"]) == (0, FORM_ROWSPACE, 0) and off["d_allreduce"] >= off["n_hmul"], off
    assert (on["code"], on["form"], on["d_allreduce"], on["d_sorted"], on["d_jv"]) == (0, FORM_ROWS_SORTED, 1, 1, 1), on
    assert on["n_launches"] == alone["n_launches"] and (on["n_hmul"], on["n_breakpoints"]) == (alone["n_hmul"], alone["n_breakpoints"]), (on, alone)
    assert np.array_equal(bits(z["rccl_on_s"]), bits(z["alone_s"])) and np.array_equal(z["rccl_on_fix"], z["alone_fix"])
    J, C, mu, A, x, g, xlow, xupp, delta = rr.gpu_cases(2)[1][2]
    s_ref, fix_ref, passes = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
    assert np.array_equal(bits(z["rccl_on_s"]), bits(s_ref)) and np.array_equal(z["rccl_on_fix"], fix_ref) and on["n_hmul"] == passes


# ------------------------------------------------------------------------------------------------------------ 4. setter and getter
def test_setter_getter_and_no_communicator(bh):
    """Bad values and a NULL handle: BH_ERR_INVALID_ARG, the state unchanged; remembered across bh_hess_set_form; with no communicator
    the switch leaves form, launches and bits of a form-6 search (and of a stepwise one) as they are."""
    lib = bh._lib.lib()
    J, C, mu, A, x, g, xlow, xupp, delta = rr.gpu_cases(2)[0][2]
    n = J.shape[1]

    def search(H):
        cons = bh.MixedConstraints(np.zeros((0, n)), None, None, l=xlow, u=xupp)
        try:
            a0 = H.stats()["n_allreduce"]
            s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
            return s, np.asarray(cons.fixvars, dtype=bool).copy(), info, H.stats()["n_allreduce"] - a0
        finally:
            cons.close()

    H = bh.AlHessian(J, C, mu)
    try:
        assert H.cauchy_rows_ranks is False
        s_step, f_step, i_step, _ = search(H)
        H.set_cauchy_rows("sorted")
        assert H.cauchy_rows_ranks is False                          # ranks=None leaves the switch alone
        s0, f0, i0, a0 = search(H)
        assert i0["form"] == FORM_ROWS_SORTED and a0 == 0
        for bad in (-1, 2, 7):
            assert lib.bh_hess_set_cauchy_rows_ranks(H._h, bad) == bh._lib.BH_ERR_INVALID_ARG
            assert H.cauchy_rows_ranks is False
        assert lib.bh_hess_set_cauchy_rows_ranks(None, 1) == bh._lib.BH_ERR_INVALID_ARG
        assert lib.bh_hess_get_cauchy_rows_ranks(None, None) == bh._lib.BH_ERR_INVALID_ARG
        assert lib.bh_hess_get_cauchy_rows_ranks(H._h, None) == 0
        H.set_cauchy_rows("sorted", ranks=True)
        on = ct.c_int32(-1)
        assert lib.bh_hess_get_cauchy_rows_ranks(H._h, ct.byref(on)) == 0 and on.value == 1 and H.cauchy_rows_ranks is True
        for bad in (-1, 2):
            assert lib.bh_hess_set_cauchy_rows_ranks(H._h, bad) == bh._lib.BH_ERR_INVALID_ARG and H.cauchy_rows_ranks is True
        assert lib.bh_hess_set_cauchy_rows(H._h, 2) == bh._lib.BH_ERR_INVALID_ARG and H.cauchy_rows == "sorted"      # the old setter: 0 | 1 only
        s1, f1, i1, a1 = search(H)                                   # no communicator: form, launches and bits unchanged
        assert i1 == i0 and a1 == 0 and np.array_equal(bits(s1), bits(s0)) and np.array_equal(f1, f0)
        H.set_form("gram")
        assert H.cauchy_rows_ranks is True and H.cauchy_rows == "sorted"
        H.set_form("implicit")
        assert H.cauchy_rows_ranks is True
        H.set_cauchy_rows("sorted")
        assert H.cauchy_rows_ranks is True                           # None again: untouched
        H.set_cauchy_rows("stepwise", ranks=True)
        s2, f2, i2, _ = search(H)                                    # the rows switch off: the ranks switch alone selects nothing
        assert i2 == i_step and np.array_equal(bits(s2), bits(s_step)) and np.array_equal(f2, f_step)
        H.set_cauchy_rows("sorted", ranks=False)
        assert H.cauchy_rows_ranks is False
    finally:
        H.close()
    wide = bh.AlHessian(np.zeros((2, 4097)), None, 0.0)              # an unserved width: the switch is remembered, nothing is allocated or taken
    try:
        wide.set_cauchy_rows("sorted", ranks=True)
        assert wide.cauchy_rows_ranks is True and not wide.cauchy_rows_served
    finally:
        wide.close()


# ------------------------------------------------------------------------------------------------------------ 5. the device-pointer entry point
def test_host_and_device_entry_points_agree_on_two_ranks(tmp_path):
    world = 2
    mr.run_ranks("rowsort_worker.py", world, tmp_path, "ipc", extra=["dev"], timeout=LIMIT)
    res = load(tmp_path, "dev", world)
    replicas_agree(res, "host")
    for r, z in enumerate(res):
        host = rec(z, "host")
        code, form, nh, nbp, d_allreduce, d_sorted = (int(v) for v in z["dev_rec"])
        assert (host["code"], host["form"]) == (0, FORM_ROWS_SORTED) and (code, form, d_allreduce, d_sorted) == (0, FORM_ROWS_SORTED, 1, 1), (r, host, z["dev_rec"])
        assert (nh, nbp) == (host["n_hmul"], host["n_breakpoints"]), (r, nh, nbp, host)
        assert np.array_equal(bits(z["dev_s"]), bits(z["host_s"])) and np.array_equal(z["dev_fix"], z["host_fix"]), r
    assert np.array_equal(bits(res[0]["dev_s"]), bits(res[1]["dev_s"]))
