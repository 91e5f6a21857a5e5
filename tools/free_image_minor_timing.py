#!/usr/bin/env python3
"""What option free_image_minor saves a minor iterate, on the bench instances (config 3: 65536 x 4096, config 2: 8192 x 1024; every
8th variable fixed, mu = 10, kappa2 = 0.1): bh_minor_iterate_dev on resident vectors, under free_image = 2 with the image in place
(built by one bh_pcg_dev), free_image_minor alternated 0 / 1 in one process on one handle.

  40 preheat calls, then per side the median over BLOCKS blocks of 20 synchronised calls, with the min - max spread; n_hmul per call;
  stats.bytes_per_hmul of each side (side 1 must read 8 (d + q) nfree + 16 nfree: its loop streamed the compact image).

--baseline-only never names the option: the same tool then runs on a commit that does not have it (one side, the full image)."""
import argparse
import ctypes as ct
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benlsip_jl_amd as bh  # noqa: E402
import bench  # noqa: E402

KAPPA2 = 0.1
PREHEAT = 40
CALLS = 20


def make_caller(H, cons, dv, delta):
    lib = bh._lib.lib()
    status, iters, n_hmul, alpha = ct.c_int32(-1), ct.c_int32(0), ct.c_int32(0), ct.c_double(0.0)
    args = (H.handle, cons.handle, dv["x"].ptr, dv["s"].ptr, dv["g"].ptr, dv["xl"].ptr, dv["xu"].ptr, ct.c_double(delta), ct.c_double(KAPPA2),
            ct.c_double(bh.operators.SQRT_EPS), ct.c_double(1e-10), dv["w"].ptr, ct.byref(status), ct.byref(iters), ct.byref(n_hmul),
            ct.byref(alpha))
    fn = lib.bh_minor_iterate_dev

    def call(count):
        for _ in range(count):
            rc = fn(*args)
            if rc != 0:
                bh._lib.check(rc, "bh_minor_iterate_dev")
        return status.value, iters.value, n_hmul.value, alpha.value
    return call


def block(call):
    lib = bh._lib.lib()
    lib.bh_synchronize()
    t0 = time.perf_counter()
    out = call(CALLS)
    lib.bh_synchronize()
    return (time.perf_counter() - t0) / CALLS, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-only", action="store_true", help="one side, the option is never named")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--configs", default="3,2")
    args = ap.parse_args()
    assert args.blocks >= 5
    bh.init(0, flags=bh._lib.BH_FLAG_PROFILE)              # as bench.py: stats.bytes_per_hmul follows the sampled launches
    sides = (None,) if args.baseline_only else (0, 1)
    for label, d, n in (("3", 65536, 4096), ("2", 8192, 1024)):
        if label not in args.configs.split(","):
            continue
        H, cons, dv, host = bench.setup_instance(bh, 0, 1, 0, d_per_gpu=d, n=n)
        nfree = n - int(host["fix"].sum())
        delta = bh.synthetic.initial_tr(host["g"])
        for k, v in (("x", host["x"]), ("s", np.zeros(n)), ("xl", host["x_l"]), ("xu", host["x_u"])):
            dv[k] = bh.DeviceVector(n, v)
        call = make_caller(H, cons, dv, delta)
        print("== config %s: J %d x %d, %d of %d variables fixed, kappa2 = %g, %d blocks of %d calls per side" % (
            label, d, n, n - nfree, n, KAPPA2, args.blocks, CALLS), flush=True)
        bh.set_option("free_image", 2)
        bench.run_steps(bh, H, cons, dv, KAPPA2, 1)                    # builds the image
        info = H.free_image_info(cons)
        assert info["builds"] == 1 and info["state"] == "valid" and info["width"] == nfree, info
        for side in sides:
            if side is not None:
                bh.set_option("free_image_minor", side)
            call(PREHEAT // len(sides))
        times = {side: [] for side in sides}
        outs = {}
        for _ in range(args.blocks):
            for side in sides:                                          # alternated: both sides see the same clocks
                if side is not None:
                    bh.set_option("free_image_minor", side)
                t, outs[side] = block(call)
                times[side].append(t)
        w = {}
        for side in sides:
            if side is not None:
                bh.set_option("free_image_minor", side)
            served = H.free_image_info(cons)["calls_served"]
            H.reset_stats()
            call(8)
            w[side] = dv["w"].download()
            st = H.stats()
            ts = 1e6 * np.array(times[side])
            name = "parent / baseline-only" if side is None else "free_image_minor = %d" % side
            print("%s: %.1f us per call (median of %d blocks, min %.1f max %.1f, spread %.1f); status %d iters %d n_hmul %d alpha %r; "
                  "bytes_per_hmul %.0f (%d sampled); calls served from the image %d of 8" % (
                      name, np.median(ts), len(ts), ts.min(), ts.max(), ts.max() - ts.min(), outs[side][0], outs[side][1], outs[side][2],
                      outs[side][3], st["bytes_per_hmul"], st["hmul_timed"], H.free_image_info(cons)["calls_served"] - served), flush=True)
            if side == 1:
                want = 8.0 * (d + H.q) * nfree + 16.0 * nfree
                print("    8 (d + q) nfree + 16 nfree = %.0f: %s" % (want, "equal" if st["bytes_per_hmul"] == want else "DIFFERENT"))
        if len(sides) == 2:
            m0, m1 = (1e6 * float(np.median(times[s])) for s in sides)
            dw = np.linalg.norm(w[1] - w[0]) / np.linalg.norm(w[0])
            print("side 1 against side 0: %.1f -> %.1f us per call (%+.1f %%); ||dw|| / ||w|| = %.2e" % (m0, m1, 100.0 * (m1 - m0) / m0, dw))
            bh.set_option("free_image_minor", 0)
        sys.stdout.flush()
        bh.set_option("free_image", 1)
        for v in dv.values():
            v.close()
        H.close()
        cons.close()


if __name__ == "__main__":
    main()
