#!/usr/bin/env python3
"""The row-space Cauchy search with K breakpoints per launch (option cauchy_block = K, cauchy_block_kernel<K>) against the same search
with one breakpoint per launch (K = 0), K in {0, 2, 4, 8, 16} alternated in one process on ONE implicit-form handle.
Instance of tools/cauchy_gram_timing.py (synthetic 65536 x 4096, fix_every = 8) at three trust-region radii, and config 2
(8192 x 1024).  Wall time around a host-pointer call (it returns synchronised), REPS >= 5 searches per K after a warm-up search each;
median, min - max spread, us per pass and launches per search.  A K counts as faster than 0 only beyond the larger of the two
spreads.  The steps are compared bit for bit on the way.  Needs a GPU.

    python tools/cauchy_block_timing.py [--out FILE] [--reps N] [--one K]      (--one K: a single config-3 search, for rocprofv3)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benlsip_jl_amd as bh  # noqa: E402

LINES = []
KS = (0, 2, 4, 8, 16)


def say(s):
    print(s, flush=True)
    LINES.append(s)


def search(H, v, delta, K):
    bh.set_option("cauchy_block", K)
    try:
        cons = bh.MixedConstraints(np.zeros((0, H.n)), None, None, l=v["x_l"], u=v["x_u"])
        t0 = time.perf_counter()
        s, info = bh.cauchy_step(v["x"], v["g"], H, cons, delta, full_output=True)
        el = time.perf_counter() - t0
        cons.close()
    finally:
        bh.set_option("cauchy_block", 0)
    return el, s, info


def instance(d, n):
    syn = bh.synthetic
    H = bh.AlHessian.synthetic(d, n, seed=1, mu=10.0)
    x, x_l, x_u, fix = syn.box_vectors(n, fix_every=8)
    g = H.jtv(syn.residual_rows(0, d))
    return H, dict(x=x, x_l=x_l, x_u=x_u, g=g)


def shape(label, d, n, radii, reps):
    H, v = instance(d, n)
    say("%s (d = %d, n = %d)" % (label, d, n))
    for dscale in radii:
        delta = dscale * bh.synthetic.initial_tr(v["g"])
        t = {K: [] for K in KS}
        res = {}
        for K in KS:
            search(H, v, delta, K)                                      # warm-up search of the same shape
        for _ in range(reps):
            for K in KS:                                                # alternated
                el, s, info = search(H, v, delta, K)
                t[K].append(el)
                res[K] = (s, info)
        med, spread = {}, {}
        for K in KS:
            s, info = res[K]
            a = 1e3 * np.array(t[K])
            med[K], spread[K] = float(np.median(a)), float(a.max() - a.min())
            same = np.array_equal(s.view(np.uint64), res[0][0].view(np.uint64)) and info["n_hmul"] == res[0][1]["n_hmul"]
            say("    delta = %.3g, cauchy_block = %2d: %d breakpoints, %d passes, %d launches; median %.3f ms (min %.3f, max %.3f, %d searches), "
                "%.2f us per pass, step %s option 0's"
                % (delta, K, info["n_breakpoints"], info["n_hmul"], info["n_launches"], med[K], a.min(), a.max(), len(a),
                   1e3 * med[K] / max(info["n_hmul"], 1), "bit-equal to" if same else "DIFFERS FROM"))
        for K in KS[1:]:
            diff, bar = med[0] - med[K], max(spread[0], spread[K])
            verdict = "faster" if diff > bar else "slower" if -diff > bar else "within the spreads"
            say("    -> K = %2d against 0: %.2fx, %+.3f ms per search against a larger spread of %.3f ms: %s" % (K, med[0] / med[K], -diff, bar, verdict))
    H.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", type=int, default=None, metavar="K", help="one config-3 search with cauchy_block = K and nothing else (kernel trace runs)")
    args = ap.parse_args()
    bh.init(0)
    if args.one is not None:
        H, v = instance(65536, 4096)
        el, s, info = search(H, v, 0.1 * bh.synthetic.initial_tr(v["g"]), args.one)
        print("one search: %d breakpoints, %d passes, %d launches, form %d" % (info["n_breakpoints"], info["n_hmul"], info["n_launches"], info["form"]))
        return
    say("# tools/cauchy_block_timing.py: row-space Cauchy search, cauchy_block = 0 / 2 / 4 / 8 / 16 alternated in one process, one implicit-form "
        "handle, one MI355X; wall times")
    shape("config 3", 65536, 4096, (0.1, 1.0, 10.0), max(args.reps, 5))
    shape("config 2", 8192, 1024, (1.0,), max(args.reps, 5))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
