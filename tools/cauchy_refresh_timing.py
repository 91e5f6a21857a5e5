#!/usr/bin/env python3
"""Option cauchy_image_refresh = R of the row-space Cauchy search (the carried images J d, J s_c — with equalities a = J D g,
B = J D A', J s_c — formed again from J every R-th pass): R in {0, 64, 256, 1024} alternated in one process on one handle, at the
config-3 shape (synthetic 65536 x 4096, box constraints, one kernel per breakpoint) and at the config-5 shape (the same J with
mA = 64 linear equalities).  Wall time around a host-pointer call (it returns synchronised), REPS searches per R after a warm-up
search of each; median and min - max spread.  From them: the cost of one re-formation ((median_R - median_0) / re-formations that
ran), the per-pass time of R = 0 in the same run, and the recommended R — the smallest power of two whose re-formation cost / R is
at most 10 % of that per-pass time.  Needs a GPU.

    python tools/cauchy_refresh_timing.py [--out FILE] [--reps N]      (FILE defaults to profiles/r08_cauchy_refresh_timing.txt)
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
INTERVALS = (0, 64, 256, 1024)
D, N = 65536, 4096


def say(s):
    print(s, flush=True)
    LINES.append(s)


def search(H, A, v, delta, R):
    bh.set_option("cauchy_image_refresh", R)
    try:
        cons = bh.MixedConstraints(A, None, None, l=v["x_l"], u=v["x_u"])
        jv0 = H.stats()["n_jv"]
        t0 = time.perf_counter()
        s, info = bh.cauchy_step(v["x"], v["g"], H, cons, delta, full_output=True)
        el = time.perf_counter() - t0
        info["n_jv"] = H.stats()["n_jv"] - jv0
        cons.close()
    finally:
        bh.set_option("cauchy_image_refresh", 0)
    return el, s, info


def shape(label, H, A, v, delta, reps):
    say("%s: delta = %.3g" % (label, delta))
    t = {R: [] for R in INTERVALS}
    res = {}
    for R in INTERVALS:
        search(H, A, v, delta, R)                                       # warm-up search of the same shape
    for _ in range(reps):
        for R in INTERVALS:                                             # alternated
            el, s, info = search(H, A, v, delta, R)
            t[R].append(el)
            res[R] = (s, info)
    med = {R: 1e3 * float(np.median(t[R])) for R in INTERVALS}
    s0, info0 = res[0]
    per_pass = 1e3 * med[0] / max(info0["n_hmul"], 1)
    costs = []
    for R in INTERVALS:
        s, info = res[R]
        a = 1e3 * np.array(t[R])
        m = (info["n_hmul"] - 1) // R if R else 0
        line = ("    R = %4d: %d breakpoints, %d passes, %d launches, %d sweeps over J, %d re-formations; median %.3f ms (min %.3f, max %.3f, %d searches), "
                "%.2f us per pass; |s - s(R=0)| / |s| = %.1e"
                % (R, info["n_breakpoints"], info["n_hmul"], info["n_launches"], info["n_jv"], m, med[R], a.min(), a.max(), len(a),
                   1e3 * med[R] / max(info["n_hmul"], 1), np.linalg.norm(s - s0) / max(np.linalg.norm(s0), 1e-300)))
        if m > 0:
            cost = 1e3 * (med[R] - med[0]) / m
            costs.append(cost)
            line += "; %.1f us per re-formation, %.2f us per pass (%.1f %% of R = 0's %.2f us)" % (cost, cost / R, 100.0 * cost / R / per_pass, per_pass)
        say(line)
    if costs:
        cost = float(np.median(costs))
        R = 1
        while cost / R > 0.1 * per_pass:
            R *= 2
        spread = max(1e3 * (max(t[k]) - min(t[k])) for k in INTERVALS)
        say("    -> one re-formation %.1f us (median over the intervals), one pass of R = 0 %.2f us; largest min - max spread of a search %.3f ms; "
            "recommended R (smallest power of two with re-formation / R <= 10 %% of a pass): %d" % (cost, per_pass, spread, R))
    else:
        say("    -> no search was long enough to run a re-formation")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_cauchy_refresh_timing.txt"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    bh.init(0)
    syn = bh.synthetic
    H = bh.AlHessian.synthetic(D, N, seed=1, mu=10.0)
    x, x_l, x_u, fix = syn.box_vectors(N, fix_every=8)
    g = H.jtv(syn.residual_rows(0, D))
    v = dict(x=x, x_l=x_l, x_u=x_u, g=g)
    say("# tools/cauchy_refresh_timing.py: row-space Cauchy search (%d x %d), cauchy_image_refresh = %s alternated in one process on one handle, "
        "one MI355X; wall times" % (D, N, " / ".join(str(R) for R in INTERVALS)))
    say("one J v sweep %.1f us (bh_time_kernel kind 1)" % (1e3 * H.time_kernel(1, reps=20)))
    reps = max(args.reps, 5)
    shape("config 3 (box constraints, one kernel per breakpoint)", H, np.zeros((0, N)), v, 10.0 * syn.initial_tr(g), reps)
    A = syn.splitmix_uniform(4, np.arange(64 * N)).reshape((64, N), order="F")
    shape("config 5 (mA = 64, B by the GEMM)", H, A, v, 10.0 * syn.initial_tr(g), reps)
    H.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
