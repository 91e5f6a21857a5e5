#!/usr/bin/env python3
"""The Cauchy search on a Gram-form handle: the whole search from G in one launch (option cauchy_gram = 1, cauchy_gram_kernel)
against the search the same handle runs without the option (row space of J, one kernel per breakpoint), alternated in one process.
Instance of tools/cauchy_timing.py (synthetic 65536 x 4096, fix_every = 8, three trust-region radii) and one wide shape
(16384 x 16384).  Wall time around a host-pointer call (it returns synchronised), REPS searches per form after a warm-up search
of the same shape; the build of G (bh_time_kernel kind 9) is printed beside them.  Needs a GPU.

    python tools/cauchy_gram_timing.py [--out FILE] [--reps N] [--one]      (--one: a single config-3 search, for rocprofv3)
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
FORMS = {0: "one H*d per breakpoint", 1: "row space of J", 2: "row space of J (equalities)", 3: "from G in one launch"}


def say(s):
    print(s, flush=True)
    LINES.append(s)


def search(H, v, delta, gram):
    bh.set_option("cauchy_gram", gram)
    try:
        cons = bh.MixedConstraints(np.zeros((0, H.n)), None, None, l=v["x_l"], u=v["x_u"])
        t0 = time.perf_counter()
        s, info = bh.cauchy_step(v["x"], v["g"], H, cons, delta, full_output=True)
        el = time.perf_counter() - t0
        cons.close()
    finally:
        bh.set_option("cauchy_gram", 0)
    return el, s, info


def shape(label, d, n, radii, reps):
    syn = bh.synthetic
    H = bh.AlHessian.synthetic(d, n, seed=1, mu=10.0)
    x, x_l, x_u, fix = syn.box_vectors(n, fix_every=8)
    g = H.jtv(syn.residual_rows(0, d))
    v = dict(x=x, x_l=x_l, x_u=x_u, g=g)
    H.set_form("gram")
    ms_build = H.time_kernel(9, reps=3)
    say("%s (d = %d, n = %d): build of G %.3f ms" % (label, d, n, ms_build))
    for dscale in radii:
        delta = dscale * syn.initial_tr(g)
        t = {0: [], 1: []}
        res = {}
        for gram in (0, 1):
            search(H, v, delta, gram)                                   # warm-up search of the same shape
        for _ in range(reps):
            for gram in (0, 1):                                        # alternated
                el, s, info = search(H, v, delta, gram)
                t[gram].append(el)
                res[gram] = (s, info)
        med = {}
        for gram in (0, 1):
            s, info = res[gram]
            a = 1e3 * np.array(t[gram])
            med[gram] = float(np.median(a))
            say("    delta = %.3g, cauchy_gram = %d (%s): %d breakpoints, %d passes, %d launches; median %.3f ms (min %.3f, max %.3f, %d searches), "
                "%.2f us per pass, |s| = %.12e"
                % (delta, gram, FORMS[info["form"]], info["n_breakpoints"], info["n_hmul"], info["n_launches"], med[gram], a.min(), a.max(), len(a),
                   1e3 * med[gram] / max(info["n_hmul"], 1), np.linalg.norm(s)))
        spread = max(1e3 * (max(t[k]) - min(t[k])) for k in (0, 1))
        saved = med[0] - med[1]
        say("    -> %.2fx; saving %.3f ms per search against a larger spread of %.3f ms; the build of G is paid for after %s searches per J"
            % (med[0] / med[1], saved, spread, "%.1f" % (ms_build / saved) if saved > 0 else "no number of"))
    H.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", action="store_true", help="one config-3 search with cauchy_gram = 1 and nothing else (kernel trace runs)")
    args = ap.parse_args()
    bh.init(0)
    if args.one:
        syn = bh.synthetic
        H = bh.AlHessian.synthetic(65536, 4096, seed=1, mu=10.0)
        x, x_l, x_u, fix = syn.box_vectors(4096, fix_every=8)
        g = H.jtv(syn.residual_rows(0, 65536))
        H.set_form("gram")
        el, s, info = search(H, dict(x=x, x_l=x_l, x_u=x_u, g=g), 0.1 * syn.initial_tr(g), 1)
        print("one search: %d breakpoints, %d passes, form %d" % (info["n_breakpoints"], info["n_hmul"], info["form"]))
        return
    say("# tools/cauchy_gram_timing.py: Cauchy search on a Gram-form handle, cauchy_gram = 0 / 1 alternated in one process, one MI355X; wall times")
    shape("config 3", 65536, 4096, (0.1, 1.0, 10.0), max(args.reps, 5))
    shape("wide", 16384, 16384, (1.0,), max(args.reps, 5))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
