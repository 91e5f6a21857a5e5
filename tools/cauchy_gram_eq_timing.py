#!/usr/bin/env python3
"""The Cauchy search with linear equalities on a Gram-form handle: from G (option cauchy_gram_eq = 1, cauchy_gram_eq_kernel, form 4)
against the search the same handle runs without the option (row space of J with equalities, form 2), alternated in one process.
Config-5 shape (synthetic 65536 x 4096, fix_every = 8, A = u(4, .) as in bench.py) at mA = 8, 16, 64 and three trust-region radii.
Wall time around a host-pointer call (it returns synchronised), REPS searches per form after a warm-up search of the same shape.
"Faster" / "slower" is only said beyond the larger min-max spread of the two forms.

Set-up and re-formation: a = G D g and B = G D A' are formed at the start and again every kCauchyGramEqRefresh-th pass by the same
three launches (mask, G v, GEMM over the n rows of G).  The tool prints the G v launch (bh_time_kernel kind 10) and the cost per
search that does not scale with the passes (intercept of the two longest searches); the GEMM's own duration comes from
`rocprofv3 --kernel-trace --stats -- python tools/cauchy_gram_eq_timing.py --one MA`.  Needs a GPU.

    python tools/cauchy_gram_eq_timing.py [--out FILE] [--reps N] [--one MA]
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benlsip_jl_amd as bh  # noqa: E402

LINES = []
FORMS = {0: "one H*d per breakpoint", 1: "row space of J", 2: "row space of J (equalities)", 3: "from G in one launch", 4: "from G (equalities)"}
D, N = 65536, 4096


def say(s):
    print(s, flush=True)
    LINES.append(s)


def refresh_interval():
    src = open(os.path.join(ROOT, "benlsip.jl_amd", "csrc", "bh_api.hip")).read()
    return int(re.search(r"constexpr int kCauchyGramEqRefresh = (\d+);", src).group(1))


def search(H, A, v, delta, eq):
    bh.set_option("cauchy_gram_eq", eq)
    try:
        cons = bh.MixedConstraints(A, None, None, l=v["x_l"], u=v["x_u"])
        t0 = time.perf_counter()
        s, info = bh.cauchy_step(v["x"], v["g"], H, cons, delta, full_output=True)
        el = time.perf_counter() - t0
        cons.close()
    finally:
        bh.set_option("cauchy_gram_eq", 0)
    return el, s, info


def instance():
    syn = bh.synthetic
    H = bh.AlHessian.synthetic(D, N, seed=1, mu=10.0)
    x, x_l, x_u, fix = syn.box_vectors(N, fix_every=8)
    g = H.jtv(syn.residual_rows(0, D))
    H.set_form("gram")
    return H, dict(x=x, x_l=x_l, x_u=x_u, g=g)


def lineq(mA):
    return bh.synthetic.splitmix_uniform(4, np.arange(mA * N)).reshape((mA, N), order="F")


def shape(H, v, mA, radii, reps, interval):
    syn = bh.synthetic
    A = lineq(mA)
    say("mA = %d" % mA)
    pts = {0: [], 1: []}
    for dscale in radii:
        delta = dscale * syn.initial_tr(v["g"])
        t = {0: [], 1: []}
        res = {}
        for eq in (0, 1):
            search(H, A, v, delta, eq)                                   # warm-up search of the same shape
        for _ in range(reps):
            for eq in (0, 1):                                           # alternated
                el, s, info = search(H, A, v, delta, eq)
                t[eq].append(el)
                res[eq] = (s, info)
        med = {}
        for eq in (0, 1):
            s, info = res[eq]
            a = 1e3 * np.array(t[eq])
            med[eq] = float(np.median(a))
            pts[eq].append((info["n_hmul"], med[eq]))
            say("    delta = %.3g, cauchy_gram_eq = %d (%s): %d breakpoints, %d passes, %d launches; median %.3f ms (min %.3f, max %.3f, %d searches), "
                "%.2f us per pass, |s| = %.12e"
                % (delta, eq, FORMS[info["form"]], info["n_breakpoints"], info["n_hmul"], info["n_launches"], med[eq], a.min(), a.max(), len(a),
                   1e3 * med[eq] / max(info["n_hmul"], 1), np.linalg.norm(s)))
        same = res[0][1]["n_hmul"] == res[1][1]["n_hmul"] and res[0][1]["n_breakpoints"] == res[1][1]["n_breakpoints"]
        spread = max(1e3 * (max(t[k]) - min(t[k])) for k in (0, 1))
        saved = med[0] - med[1]
        verdict = "faster" if saved > spread else "slower" if -saved > spread else "no difference beyond the spread"
        say("    -> %.2fx (%s): %.3f ms per search against a larger spread of %.3f ms; same passes and breakpoints: %s; |s| differs by %.1e"
            % (med[0] / med[1], verdict, saved, spread, same, np.linalg.norm(res[0][0] - res[1][0]) / max(np.linalg.norm(res[0][0]), 1e-300)))
    for eq in (0, 1):
        p = sorted(pts[eq])
        if len(p) >= 2 and p[-1][0] > p[-2][0]:
            slope = (p[-1][1] - p[-2][1]) / (p[-1][0] - p[-2][0])
            say("    cauchy_gram_eq = %d: %.2f us per additional pass between the two longest searches%s; %.3f ms per search do not scale with the passes "
                "(set-up, init, adoption of the mask)"
                % (eq, 1e3 * slope, " (one formation of a, B per %d passes included)" % interval if eq else "", p[-1][1] - slope * p[-1][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", type=int, default=0, metavar="MA", help="one search with cauchy_gram_eq = 1 at this mA and nothing else (kernel trace runs)")
    args = ap.parse_args()
    bh.init(0)
    interval = refresh_interval()
    H, v = instance()
    if args.one:
        el, s, info = search(H, lineq(args.one), v, 1.0 * bh.synthetic.initial_tr(v["g"]), 1)
        print("one search, mA = %d: %d breakpoints, %d passes, form %d, %d G v launches" % (args.one, info["n_breakpoints"], info["n_hmul"], info["form"],
                                                                                          H.stats()["n_hmul"]))
        return
    say("# tools/cauchy_gram_eq_timing.py: Cauchy search with linear equalities on a Gram-form handle (%d x %d), cauchy_gram_eq = 0 / 1 alternated in one "
        "process, one MI355X; wall times" % (D, N))
    say("build of G %.3f ms; one G v launch %.2f us; a, B formed again every %d passes" % (H.time_kernel(9, reps=3), 1e3 * H.time_kernel(10, reps=50), interval))
    for mA in (8, 16, 64):
        shape(H, v, mA, (0.1, 1.0, 10.0), max(args.reps, 5), interval)
    H.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
