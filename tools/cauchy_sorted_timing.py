#!/usr/bin/env python3
"""The Cauchy search on a Gram-form handle: the sorted form (bh_hess_set_cauchy_search at BH_CAUCHY_SORTED, form 5: ranks, one read of
the free rows of G, one scan — the same launches for every search length) against the fastest stepwise form the same handle has
(BH_CAUCHY_STEPWISE with cauchy_gram = 1, form 3: one launch that walks the breakpoints), alternated in one process.
Instance of tools/cauchy_gram_timing.py (synthetic 65536 x 4096, fix_every = 8, three trust-region radii), config 2 (8192 x 1024) and a
sweep of short searches (0 .. 256 breakpoints) that looks for the search length at which the two forms cost the same.  Wall time around a host-pointer call
(it returns synchronised); ROUNDS rounds of REPS alternated searches after a warm-up search of each form.  At every radius the two
forms must agree: same breakpoint count, same active set, step within 1e-9.  Needs a GPU.

    python tools/cauchy_sorted_timing.py [--out FILE] [--reps N] [--one]      (--one: three sorted config-3 searches, for a kernel trace)
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
ROUNDS = 3
FORMS = {3: "from G in one launch, stepwise", 5: "from G in one sorted sweep"}


def say(s):
    print(s, flush=True)
    LINES.append(s)


def search(H, v, delta, sorted_form):
    H.set_cauchy_search("sorted" if sorted_form else "stepwise")
    bh.set_option("cauchy_gram", 1)
    try:
        cons = bh.MixedConstraints(np.zeros((0, H.n)), None, None, l=v["x_l"], u=v["x_u"])
        t0 = time.perf_counter()
        s, info = bh.cauchy_step(v["x"], v["g"], H, cons, delta, full_output=True)
        el = time.perf_counter() - t0
        fix = np.asarray(cons.fixvars, dtype=bool).copy()
        cons.close()
    finally:
        bh.set_option("cauchy_gram", 0)
        H.set_cauchy_search("stepwise")
    return el, s, fix, info


def instance(d, n):
    syn = bh.synthetic
    H = bh.AlHessian.synthetic(d, n, seed=1, mu=10.0)
    x, x_l, x_u, fix = syn.box_vectors(n, fix_every=8)
    g = H.jtv(syn.residual_rows(0, d))
    H.set_form("gram")
    return H, dict(x=x, x_l=x_l, x_u=x_u, g=g), syn.initial_tr(g)


def compare(H, v, delta, reps):
    """ROUNDS x reps alternated searches of both forms; returns the medians in us and the breakpoint count."""
    t = {0: [], 1: []}
    res = {}
    for f in (0, 1):
        search(H, v, delta, f)                                          # warm-up search of the same shape
    for _ in range(ROUNDS):
        for _ in range(reps):
            for f in (0, 1):                                           # alternated
                el, s, fix, info = search(H, v, delta, f)
                t[f].append(el)
                res[f] = (s, fix, info)
    (s0, f0, i0), (s1, f1, i1) = res[0], res[1]
    assert (i0["form"], i1["form"]) == (3, 5), (i0, i1)
    assert (i0["n_breakpoints"], i0["n_hmul"]) == (i1["n_breakpoints"], i1["n_hmul"]) and np.array_equal(f0, f1), (i0, i1)
    rel = float(np.linalg.norm(s1 - s0) / max(np.linalg.norm(s0), 1e-300))
    assert rel <= 1e-9, rel
    med = {}
    for f in (0, 1):
        a = 1e6 * np.array(t[f])
        per_round = [float(np.median(a[r * reps:(r + 1) * reps])) for r in range(ROUNDS)]
        med[f] = float(np.median(a))
        say("    delta = %.3g, form %d (%s): %d breakpoints, %d launches; median %.1f us per search (rounds %s; min %.1f, max %.1f, %d searches)"
            % (delta, res[f][2]["form"], FORMS[res[f][2]["form"]], res[f][2]["n_breakpoints"], res[f][2]["n_launches"], med[f],
               " ".join("%.1f" % m for m in per_round), a.min(), a.max(), len(a)))
    say("    -> stepwise / sorted = %.2fx; the two forms agree: same set, same count, step within %.1e" % (med[0] / med[1], rel))
    return med, i1["n_breakpoints"]


def shape(label, d, n, radii, reps):
    H, v, tr = instance(d, n)
    say("%s (d = %d, n = %d)" % (label, d, n))
    for dscale in radii:
        compare(H, v, dscale * tr, reps)
    return H, v, tr


def short_instance(v, m):
    """The vectors of `v` with wide bounds (+-1e6 around x) on every free variable but the first m, which meet a bound at
    T = 1e-5, 2e-5, ...: the search passes those m breakpoints and ends at the minimiser of the next segment."""
    x, g = v["x"], v["g"]
    free = (x - v["x_l"] > 1e-7) & (v["x_u"] - x > 1e-7)
    x_l, x_u = np.where(free, x - 1e6, v["x_l"]), np.where(free, x + 1e6, v["x_u"])
    for k, i in enumerate(np.flatnonzero(free & (g != 0.0))[:m]):
        if g[i] < 0:
            x_u[i] = x[i] + 1e-5 * (k + 1) * -g[i]
        else:
            x_l[i] = x[i] - 1e-5 * (k + 1) * g[i]
    return dict(x=x, x_l=x_l, x_u=x_u, g=g)


def break_even(H, v, reps):
    """Short searches (short_instance, an infinite radius in effect): the search length at which the sorted form costs what the
    one-launch walk costs."""
    say("break-even (config 3 shape, wide bounds but for m variables, delta = 1e12)")
    rows = []
    for m in (0, 8, 16, 32, 64, 128, 256):
        med, nb = compare(H, short_instance(v, m), 1e12, reps)
        rows.append((nb, med[0], med[1]))
    wins = [nb for nb, a, b in rows if b < a]
    loses = [nb for nb, a, b in rows if b >= a]
    say("    sorted form faster at %s breakpoints, not faster at %s" % (wins or "no length measured", loses or "no length measured"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", action="store_true", help="three sorted config-3 searches and nothing else (kernel trace runs)")
    args = ap.parse_args()
    bh.init(0)
    if args.one:
        H, v, tr = instance(65536, 4096)
        for _ in range(3):
            el, s, fix, info = search(H, v, 1.0 * tr, 1)
        print("sorted search: %d breakpoints, form %d, %d launches" % (info["n_breakpoints"], info["form"], info["n_launches"]))
        return
    say("# tools/cauchy_sorted_timing.py: Cauchy search on a Gram-form handle, form 3 (cauchy_gram = 1) / form 5 (sorted) alternated in one "
        "process, one MI355X; wall times of a synchronised host-pointer call, measured")
    H, v, tr = shape("config 3", 65536, 4096, (0.1, 1.0, 10.0), max(args.reps, 5))
    break_even(H, v, max(args.reps, 5))
    H.close()
    H, v, tr = shape("config 2", 8192, 1024, (0.1, 1.0, 10.0), max(args.reps, 5))
    H.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
