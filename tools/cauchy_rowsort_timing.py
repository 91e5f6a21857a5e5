#!/usr/bin/env python3
"""The box-constrained Cauchy search on an implicit handle: the sorted rows form (bh_hess_set_cauchy_rows at BH_CAUCHY_ROWS_SORTED,
form 6: ranks, one read of J with a suffix and a prefix scan per row, the slab sums, one scan — the same launches for every search
length) against the stepwise row-space form the same handle runs by default (form 1) and against that form with cauchy_block = 16,
alternated in one process.  Instance of tools/cauchy_sorted_timing.py (synthetic 65536 x 4096, fix_every = 8, three trust-region
radii), config 2 (8192 x 1024) and a sweep of short searches (0 .. 256 breakpoints) that looks for the search length at which the
forms cost the same.  Wall time around a host-pointer call (it returns synchronised); ROUNDS rounds of REPS alternated searches after
a warm-up search of each form.  At every radius the forms must agree: same breakpoint count, same active set, step within 1e-9.
The read-only probe of the same image (bh_time_kernel kinds 3 - 6) is printed beside them.  Needs a GPU.

    python tools/cauchy_rowsort_timing.py [--out FILE] [--reps N] [--one]     (--one: three sorted config-3 searches, for a kernel trace;
                                                                               it prints the bytes the row scan reads, for its GB/s)
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
VARIANTS = (("form 1", "stepwise", 0), ("form 1, cauchy_block = 16", "stepwise", 16), ("form 6, sorted rows", "sorted", 0))


def say(s):
    print(s, flush=True)
    LINES.append(s)


def search(H, v, delta, variant):
    _, rows, block = VARIANTS[variant]
    H.set_cauchy_rows(rows)
    bh.set_option("cauchy_block", block)
    try:
        cons = bh.MixedConstraints(np.zeros((0, H.n)), None, None, l=v["x_l"], u=v["x_u"])
        t0 = time.perf_counter()
        s, info = bh.cauchy_step(v["x"], v["g"], H, cons, delta, full_output=True)
        el = time.perf_counter() - t0
        fix = np.asarray(cons.fixvars, dtype=bool).copy()
        cons.close()
    finally:
        bh.set_option("cauchy_block", 0)
        H.set_cauchy_rows("stepwise")
    return el, s, fix, info


def instance(d, n):
    syn = bh.synthetic
    H = bh.AlHessian.synthetic(d, n, seed=1, mu=10.0)
    x, x_l, x_u, fix = syn.box_vectors(n, fix_every=8)
    g = H.jtv(syn.residual_rows(0, d))
    return H, dict(x=x, x_l=x_l, x_u=x_u, g=g), syn.initial_tr(g)


def compare(H, v, delta, reps):
    """ROUNDS x reps alternated searches of the three variants; returns the medians in us and the breakpoint count."""
    t = {f: [] for f in range(len(VARIANTS))}
    res = {}
    for f in t:
        search(H, v, delta, f)                                          # warm-up search of the same shape
    for _ in range(ROUNDS):
        for _ in range(reps):
            for f in t:                                                # alternated
                el, s, fix, info = search(H, v, delta, f)
                t[f].append(el)
                res[f] = (s, fix, info)
    s0, f0, i0 = res[0]
    assert [res[f][2]["form"] for f in t] == [1, 1, 6], [res[f][2] for f in t]
    med = {}
    for f in t:
        s, fix, info = res[f]
        assert (info["n_breakpoints"], info["n_hmul"]) == (i0["n_breakpoints"], i0["n_hmul"]) and np.array_equal(fix, f0), (i0, info)
        rel = float(np.linalg.norm(s - s0) / max(np.linalg.norm(s0), 1e-300))
        assert rel <= 1e-9, rel
        a = 1e6 * np.array(t[f])
        per_round = [float(np.median(a[r * reps:(r + 1) * reps])) for r in range(ROUNDS)]
        med[f] = float(np.median(a))
        say("    delta = %.3g, %-26s %d breakpoints, %d launches; median %.1f us per search (rounds %s; min %.1f, max %.1f, %d searches; "
            "step vs form 1 %.1e)" % (delta, VARIANTS[f][0] + ":", info["n_breakpoints"], info["n_launches"], med[f],
                                      " ".join("%.1f" % m for m in per_round), a.min(), a.max(), len(a), rel))
    say("    -> form 1 / form 6 = %.2fx, cauchy_block = 16 / form 6 = %.2fx; same set, same count" % (med[0] / med[2], med[1] / med[2]))
    return med, i0["n_breakpoints"]


def probe(H):
    for kind in (3, 4, 5, 6):
        ms = H.time_kernel(kind, reps=10)
        say("    read-only probe of the image, bh_time_kernel kind %d: %.1f us, %.0f GB/s" % (kind, 1e3 * ms, 8.0 * H.d * H.n / (1e6 * ms)))


def shape(label, d, n, radii, reps):
    H, v, tr = instance(d, n)
    say("%s (d = %d, n = %d; the image is %.0f MiB)" % (label, d, n, 8.0 * d * n / 2 ** 20))
    probe(H)
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
    say("break-even (config 3 shape, wide bounds but for m variables, delta = 1e12)")
    rows = []
    for m in (0, 8, 16, 32, 256):
        med, nb = compare(H, short_instance(v, m), 1e12, reps)
        rows.append((nb, med[0], med[1], med[2]))
    say("    sorted rows form faster than form 1 at %s breakpoints, than cauchy_block = 16 at %s (of %s measured)"
        % ([nb for nb, a, b, c in rows if c < a] or "no length", [nb for nb, a, b, c in rows if c < b] or "no length", [r[0] for r in rows]))


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
            el, s, fix, info = search(H, v, 1.0 * tr, 2)
        print("sorted rows search: %d breakpoints, form %d, %d launches" % (info["n_breakpoints"], info["form"], info["n_launches"]))
        print("cauchy_rowsort_rows_kernel reads the image once: %d B; its achieved rate is that over its duration in the trace, to be set "
              "against the read-only probe (bh_time_kernel kind 3: %.1f us)" % (8 * H.d * H.n, 1e3 * H.time_kernel(3, reps=10)))
        return
    say("# tools/cauchy_rowsort_timing.py: Cauchy search on an implicit handle, form 1 / form 1 with cauchy_block = 16 / form 6 (sorted "
        "rows) alternated in one process, one MI355X; wall times of a synchronised host-pointer call, measured")
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
