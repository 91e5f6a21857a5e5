#!/usr/bin/env python3
"""Everything a bh_pcg / bh_cauchy_step call hands back, bit for bit, over the shapes of the two host drivers — to be run on builds
of two commits and compared with diff (a change of the host drivers that must not change a result):

    python tools/launch_schedule_dump.py [--lib OTHER/libbenlsip_hip.so] > dump.txt

bh_pcg: status, iters, n_hmul, stats.cg_kernels, the trace and w as 64-bit words; two calls per handle (the second one's first batch
is sized by the first one's count).  Cells: every stats.cg_kernels value one rank reaches — 0 with fold_init on and off and with
equalities, 2 on J, on G (gram_cg_fused) and on the compact image (free_image = 2), 3, 4 (cg_fused = 2) — at n = 2, 33, 256
(d = 2 n: max_iter = 2, an odd n through the staging path, more than one launch-ahead batch); one cell that ends at max_iter; one
free_image cell whose g is not finite on a fixed variable (the call is handed back to the full image).
bh_cauchy_step: s, the fix chunks, n_breakpoints, n_hmul and bh_cauchy_info's launch count for each of the five forms at n = 33 (about
ten passes: more than one launch-ahead batch; every decision of that driver is lock-step, so the launch count is deterministic).
The instances are made here from a seeded generator; nothing outside the repository is read."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benlsip_jl_amd as bh  # noqa: E402

PCG_DEFAULTS = {"cg_fused": 1, "fold_init": 1, "gram_cg_fused": 0, "free_image": 1}
CAUCHY_DEFAULTS = {"cauchy_image": 1, "cauchy_fused": 1, "cauchy_gram": 0, "cauchy_gram_eq": 0}
# label -> (options, equalities, Gram handle)
PCG_CELLS = [
    ("cg_kernels 0, fold_init 1", {"cg_fused": 0, "free_image": 0}, 0, False),
    ("cg_kernels 0, fold_init 0", {"cg_fused": 0, "fold_init": 0, "free_image": 0}, 0, False),
    ("cg_kernels 0, equalities", {"cg_fused": 0}, 1, False),
    ("cg_kernels 2, box", {"free_image": 0}, 0, False),
    ("cg_kernels 2, Gram", {"gram_cg_fused": 1}, 0, True),
    ("cg_kernels 2, free_image 2", {"free_image": 2}, 0, False),
    ("cg_kernels 3", {}, 1, False),
    ("cg_kernels 4", {"cg_fused": 2}, 1, False),
]
CAUCHY_CELLS = [
    ("form 0", {"cauchy_image": 0}, 0, False),
    ("form 1, one kernel per pass", {}, 0, False),
    ("form 1, two kernels per pass", {"cauchy_fused": 0}, 0, False),
    ("form 2", {}, 3, False),
    ("form 3", {"cauchy_gram": 1}, 0, True),
    ("form 4", {"cauchy_gram_eq": 1}, 3, True),
]


def words(a):
    return " ".join("%016x" % v for v in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel())


def instance(n, mA, seed):
    """J (2n x n, columns scaled over three decades), g, a box around 0 that some variables reach, every 4th variable fixed (n = 2:
    the second one; with equalities at n = 2: none, so that something stays free)."""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((2 * n, n)) * np.logspace(0, -3, n)
    g = J.T @ rng.standard_normal(2 * n)
    fix = np.zeros(n, dtype=bool)
    if n == 2:
        fix[1] = mA == 0
    else:
        fix[3::4] = True
    w_u = np.where(fix, 0.0, rng.uniform(0.05, 50.0, n))
    w_l = -np.where(fix, 0.0, rng.uniform(0.05, 50.0, n))
    A = rng.standard_normal((min(mA, 1) if n == 2 else mA, n)) if mA else np.zeros((0, n))
    return J, g, w_l, w_u, fix, A


def with_options(opts, defaults, fn):
    try:
        for k, v in opts.items():
            bh.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            bh.set_option(k, defaults[k])


def pcg_cell(label, opts, mA, gram, n, kappa2=0.1, wide=False, nan_on_fixed=False):
    J, g, w_l, w_u, fix, A = instance(n, 3 * mA, 1000 + n)
    if wide:
        w_l, w_u = np.where(fix, 0.0, -1e12), np.where(fix, 0.0, 1e12)
    if nan_on_fixed:
        g = g.copy()
        g[np.flatnonzero(fix)[0]] = np.nan

    def run():
        H = bh.AlHessian(J, None, 10.0)
        if gram:
            H.set_form("gram")
        cons = bh.MixedConstraints(A, None, fix, l=w_l, u=w_u)
        for call in (1, 2):
            try:
                w, st, info = bh.projected_cg(g, H, w_l, w_u, cons, kappa2, trace_cap=2 * n + 2, full_output=True)
                print("pcg | %s | n %d | call %d | status %d iters %d n_hmul %d cg_kernels %d" % (
                    label, n, call, int(st), info["iters"], info["n_hmul"], H.stats()["cg_kernels"]))
                print("  trace", words(info["trace"]))
                print("  w", words(w))
            except bh.BenlsipHipError as e:
                print("pcg | %s | n %d | call %d | error %s" % (label, n, call, e))
        cons.close()
        H.close()
    with_options(opts, PCG_DEFAULTS, run)


def cauchy_cell(label, opts, mA, gram, n=33):
    rng = np.random.default_rng(7)
    J = 0.2 * rng.standard_normal((2 * n, n))          # a flat model: the path meets about ten bounds before its minimum
    x = rng.uniform(0.2, 0.8, n)
    g = rng.standard_normal(n)
    xlow, xupp = np.zeros(n), np.ones(n)
    A = rng.standard_normal((mA, n))

    def run():
        H = bh.AlHessian(J, None, 10.0)
        if gram:
            H.set_form("gram")
        for call in (1, 2):
            cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
            try:
                s, info = bh.cauchy_step(x, g, H, cons, 0.5 * np.sqrt(n), full_output=True)
                fix = np.packbits(np.asarray(cons.fixvars, dtype=bool), bitorder="little")
                print("cauchy | %s | call %d | form %d n_breakpoints %d n_hmul %d n_launches %d" % (
                    label, call, info["form"], info["n_breakpoints"], info["n_hmul"], info["n_launches"]))
                print("  fix", fix.tobytes().hex())
                print("  s", words(s))
            except bh.BenlsipHipError as e:
                print("cauchy | %s | call %d | error %s" % (label, call, e))
            cons.close()
        H.close()
    with_options(opts, CAUCHY_DEFAULTS, run)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="load this build of the library instead of the tree's")
    args = ap.parse_args()
    if args.lib:
        bh.build.OUT = os.path.abspath(args.lib)
    bh.init(0)
    for n in (2, 33, 256):
        for label, opts, mA, gram in PCG_CELLS:
            pcg_cell(label, opts, mA, gram, n)
    pcg_cell("ends at max_iter", {"free_image": 0}, 0, False, 33, kappa2=0.0, wide=True)
    pcg_cell("free_image 2, g not finite on a fixed variable", {"free_image": 2}, 0, False, 33, nan_on_fixed=True)
    for label, opts, mA, gram in CAUCHY_CELLS:
        cauchy_cell(label, opts, mA, gram)


if __name__ == "__main__":
    main()
