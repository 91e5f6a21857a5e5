"""One rank of tests/test_cauchy_rowsort_ranks_gpu.py: the sorted rows form of the box-constrained Cauchy search on a row-sharded
implicit handle (bh_hess_set_cauchy_rows_ranks).  Modes (argv[4]):
    cases     the instances of rowsort_ranks_cases.gpu_cases (argv[5] = "narrow": without the n = 4096 one): the search with the ranks
              switch on (twice), then off, with the counters
    nan       a NaN in g on a free variable: the collective hand-back
    dev       bh_cauchy_step_dev against the host entry point
    rccl_one  (one process, BH_FORCE_COMM=1 BH_COMM=rccl) form 6 without a communicator, then over a one-rank communicator of the
              real librccl
The instances come from tests/rowsort_ranks_cases.py (whose generators import the oracle package); every comparison is the parent's."""
import ctypes as ct
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, os.path.join(ROOT, "oracle"), TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import rowsort_ranks_cases as rr                               # noqa: E402


def n_cu_of(bh):
    n_cu, name, arch = ct.c_int32(0), ct.create_string_buffer(256), ct.create_string_buffer(64)
    assert bh._lib.lib().bh_device_info(name, 256, ct.byref(n_cu), arch, 64) == 0
    return n_cu.value


def search(bh, H, inst, out, key):
    """One host-pointer search on a fresh constraint handle; the step, the set, the call's record and the growth of the counters."""
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    cons = bh.MixedConstraints(np.zeros((0, H.n)), None, None, l=xlow, u=xupp)
    try:
        st0, n0 = H.stats(), H.searches_rows_sorted
        try:
            s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
            code = 0
        except bh.BenlsipHipError as e:
            s, info, code = np.full(H.n, np.nan), {"form": -1, "n_launches": -1, "n_hmul": -1, "n_breakpoints": -1}, e.code
            try:
                info["form"], info["n_launches"] = bh.cauchy_info(cons)  # (a call that got as far as its epilogue has left its record)
            except bh.BenlsipHipError:
                pass
        st1 = H.stats()
        out[key + "_s"] = s
        out[key + "_fix"] = np.asarray(cons.fixvars, dtype=bool).copy() if code == 0 else np.zeros(H.n, dtype=bool)
        out[key + "_rec"] = np.array([code, info["form"], info["n_launches"], info["n_hmul"], info["n_breakpoints"],
                                      st1["n_allreduce"] - st0["n_allreduce"], st1["n_jv"] - st0["n_jv"], st1["n_hmul"] - st0["n_hmul"],
                                      H.searches_rows_sorted - n0], dtype=np.int64)
    finally:
        cons.close()


def shard(bh, inst, rank, world):
    J, C, mu = inst[:3]
    lo, hi = bh.row_shard(J.shape[0], rank, world)
    return bh.AlHessian(J[lo:hi], C if C is not None and C.shape[0] else None, mu), lo, hi


def run_cases(bh, rank, world, out):
    out["n_cu"] = n_cu_of(bh)
    for name, kind, inst in rr.gpu_cases(world, int(out["n_cu"]), full_width=sys.argv[5:6] != ["narrow"]):
        H, lo, hi = shard(bh, inst, rank, world)
        out[name + "_rows"] = hi - lo
        assert (H.cauchy_rows, H.cauchy_rows_ranks) == ("stepwise", False)
        H.set_cauchy_rows("sorted", ranks=True)
        assert (H.cauchy_rows, H.cauchy_rows_ranks, H.cauchy_rows_served) == ("sorted", True, True)
        search(bh, H, inst, out, name + "_on")
        search(bh, H, inst, out, name + "_again")
        H.set_cauchy_rows("sorted", ranks=False)                     # the same handle, the switch at 0: today's path
        search(bh, H, inst, out, name + "_off")
        H.close()


def run_nan(bh, rank, world, out):
    rng = np.random.default_rng(3)
    n, d = 6, 20
    J = rng.standard_normal((d, n)) / np.sqrt(20.0)
    g = rng.standard_normal(n)
    g[2] = np.nan
    inst = (J, None, 0.0, None, np.zeros(n), g, -np.ones(n), np.ones(n), 10.0)
    H, lo, hi = shard(bh, inst, rank, world)
    H.set_cauchy_rows("sorted", ranks=False)
    search(bh, H, inst, out, "nan_off")
    H.set_cauchy_rows("sorted", ranks=True)
    search(bh, H, inst, out, "nan_on")
    g = g.copy()
    g[2] = 0.25                                                      # the handle serves the next, finite call in the sorted form
    search(bh, H, (J, None, 0.0, None, np.zeros(n), g, -np.ones(n), np.ones(n), 10.0), out, "finite_on")
    H.close()


def run_dev(bh, rank, world, out):
    inst = rr.gpu_cases(world)[0][2]
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    n = J.shape[1]
    H, lo, hi = shard(bh, inst, rank, world)
    H.set_cauchy_rows("sorted", ranks=True)
    search(bh, H, inst, out, "host")
    lib = bh._lib.lib()
    cons = bh.MixedConstraints(np.zeros((0, n)), None, None, l=xlow, u=xupp)
    dv = {k: bh.DeviceVector(n, v) for k, v in (("x", x), ("g", g), ("xl", xlow), ("xu", xupp), ("s", np.zeros(n)))}
    try:
        cons._sync()
        chunks = np.zeros((n + 63) // 64, dtype=np.uint64)
        nbp, nh = ct.c_int32(0), ct.c_int32(0)
        a0, n0 = H.stats()["n_allreduce"], H.searches_rows_sorted
        bh._lib.check(lib.bh_cauchy_step_dev(H.handle, cons._h, dv["x"].ptr, dv["g"].ptr, dv["xl"].ptr, dv["xu"].ptr, float(delta), dv["s"].ptr,
                                             bh._lib.ptr(chunks), ct.byref(nbp), ct.byref(nh)), "bh_cauchy_step_dev")
        out["dev_s"] = dv["s"].download()
        out["dev_fix"] = np.unpackbits(chunks.view(np.uint8), bitorder="little")[:n].astype(bool)
        out["dev_rec"] = np.array([0, bh.cauchy_info(cons)[0], nh.value, nbp.value, H.stats()["n_allreduce"] - a0, H.searches_rows_sorted - n0], dtype=np.int64)
    finally:
        for v in dv.values():
            v.close()
        cons.close()
        H.close()


def run_rccl_one(bh, out):
    inst = rr.gpu_cases(2)[1][2]                                     # full_width_few_rows: exact
    H = bh.AlHessian(inst[0], inst[1], inst[2])
    H.set_cauchy_rows("sorted", ranks=True)                          # no communicator: the switch changes nothing
    search(bh, H, inst, out, "alone")
    H.close()
    bh.init_distributed(0, 1, lambda b: b)
    rank, nranks = ct.c_int32(-1), ct.c_int32(-1)
    bh._lib.check(bh._lib.lib().bh_comm_info(ct.byref(rank), ct.byref(nranks)), "bh_comm_info")
    out["comm"] = np.array([rank.value, nranks.value])
    H = bh.AlHessian(inst[0], inst[1], inst[2])
    H.set_cauchy_rows("sorted")
    search(bh, H, inst, out, "rccl_off")                             # a communicator and the ranks switch at 0: the stepwise path
    H.set_cauchy_rows("sorted", ranks=True)
    search(bh, H, inst, out, "rccl_on")
    H.close()


def main():
    rank, world, workdir, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import benlsip_jl_amd as bh
    bh.init(0)
    out = {}
    if mode == "rccl_one":
        run_rccl_one(bh, out)
    else:
        idfile = os.path.join(workdir, "unique_id_rowsort_%s.bin" % mode)

        def bcast(buf):
            if rank == 0:
                with open(idfile + ".tmp", "wb") as f:
                    f.write(buf)
                os.rename(idfile + ".tmp", idfile)
                return buf
            t0 = time.time()
            while not os.path.exists(idfile):
                if time.time() - t0 > 60:
                    raise RuntimeError("no unique id from rank 0")
                time.sleep(0.01)
            return open(idfile, "rb").read()

        bh.init_distributed(rank, world, bcast)
        {"cases": run_cases, "nan": run_nan, "dev": run_dev}[mode](bh, rank, world, out)
    np.savez(os.path.join(workdir, "rowsort_%s_rank%d.npz" % (mode, rank)), **out)
    bh._lib.check(bh._lib.lib().bh_comm_destroy(), "bh_comm_destroy")
    print("rank %d of %d, %s: done" % (rank, world, mode), flush=True)


if __name__ == "__main__":
    main()
