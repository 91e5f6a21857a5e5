#!/usr/bin/env python3
"""What the compact image of the free columns (option free_image) costs and saves, on the bench instances (config 3:
65536 x 4096, config 2: 8192 x 1024; every 8th variable fixed):

  - the streaming kernel on the full and on the compact image (bh_time_kernel kind 0, which follows the handle's image);
  - a build, as the caller sees it: a bh_pcg_dev call that builds first against calls served from the image;
  - the moves of k = 1, 8, 64 newly fixed variables, the same way;
  - the subproblem itself on either image.

The constants of csrc/bh_free_image_plan.h are taken from this tool's output (profiles/rNN_free_image_timing.txt), in sweeps of
the full image."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benlsip_jl_amd as bh  # noqa: E402
import bench  # noqa: E402


def timed_call(H, cons, dv):
    lib = bh._lib.lib()
    _ = cons.handle                                   # a changed active set is pushed here, outside the timed window
    lib.bh_synchronize()
    t0 = time.perf_counter()
    out = bench.run_steps(bh, H, cons, dv, 0.1, 1)
    lib.bh_synchronize()
    return time.perf_counter() - t0, out


def served(H, cons, dv, reps=9):
    """Median time of a call served from whatever image the handle has now."""
    bench.run_steps(bh, H, cons, dv, 0.1, 3)
    return float(np.median([timed_call(H, cons, dv)[0] for _ in range(reps)]))


def main():
    bh.init(0)
    for label, d, n in (("config 3", 65536, 4096), ("config 2", 8192, 1024)):
        H, cons, dv, host = bench.setup_instance(bh, 0, 1, 0, d_per_gpu=d, n=n)
        fix0 = host["fix"].copy()
        print("== %s: J %d x %d, %d of %d variables fixed" % (label, d, n, int(fix0.sum()), n), flush=True)
        bh.set_option("free_image", 0)
        bench.run_steps(bh, H, cons, dv, 0.1, 20)                    # clocks up
        full_ms = min(H.time_kernel(0, 20) for _ in range(3))
        t_full = served(H, cons, dv)
        bh.set_option("free_image", 2)
        t_first, out = timed_call(H, cons, dv)                       # builds
        info = H.free_image_info(cons)
        assert info["builds"] == 1 and info["state"] == "valid", info
        compact_ms = min(H.time_kernel(0, 20) for _ in range(3))
        t_compact = served(H, cons, dv)
        print("streaming kernel: full image %.4f ms, compact image (width %d) %.4f ms, ratio %.4f (bytes ratio %.4f)" % (
            full_ms, info["width"], compact_ms, compact_ms / full_ms, info["width"] / n))
        print("subproblem (%d H*p): full image %.1f us, compact image %.1f us" % (out[2], 1e6 * t_full, 1e6 * t_compact))
        # builds: free one variable (the image cannot grow: option 2 builds it again), then fix it again (one move)
        builds, moves1 = [], []
        free_one = int(np.flatnonzero(fix0)[5])
        for rep in range(5):
            fix = fix0.copy()
            fix[free_one] = False
            cons.fixvars = fix
            t, _ = timed_call(H, cons, dv)
            builds.append(t - t_compact)
            cons.fixvars = fix0
            t, _ = timed_call(H, cons, dv)
            moves1.append(t - t_compact)
        assert H.free_image_info(cons)["builds"] == 6 and H.free_image_info(cons)["moves"] == 5
        print("build (first call, includes the allocation): %.1f us; rebuilds: %s us -> median %.1f us = %.2f sweeps" % (
            1e6 * (t_first - t_compact), " ".join("%.1f" % (1e6 * b) for b in builds), 1e6 * np.median(builds), 1e3 * np.median(builds) / full_ms))
        print("moves k = 1: %s us -> median %.1f us = %.3f sweeps" % (" ".join("%.1f" % (1e6 * m) for m in moves1), 1e6 * np.median(moves1),
                                                                     1e3 * np.median(moves1) / full_ms))
        rng = np.random.default_rng(0)
        fix = fix0.copy()
        for k in (8, 64):
            ts = []
            for rep in range(5):
                fix = fix.copy()
                fix[rng.choice(np.flatnonzero(~fix), k, replace=False)] = True
                cons.fixvars = fix
                m0 = H.free_image_info(None)["moves"]
                t, _ = timed_call(H, cons, dv)
                assert H.free_image_info(cons)["moves"] == m0 + k
                ts.append(t - served(H, cons, dv, reps=5))
            print("moves k = %d: %s us -> median %.1f us = %.3f sweeps" % (k, " ".join("%.1f" % (1e6 * m) for m in ts), 1e6 * np.median(ts),
                                                                           1e3 * np.median(ts) / full_ms))
        sys.stdout.flush()
        bh.set_option("free_image", 1)
        H.close()
        cons.close()


if __name__ == "__main__":
    main()
