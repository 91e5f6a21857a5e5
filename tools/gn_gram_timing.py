#!/usr/bin/env python3
"""The explicit Gram form of the Gauss-Newton Hessian (bh_hess_set_form) against the implicit one, on synthetic instances:
build of G (ms, TFLOP/s of the useful lower-triangle flop 2 (d+q) n (n+1)/2), one G·v launch
(us, GB/s of its 8 n ld bytes), us per CG iteration of projected_cg (bench instance, "ic" columns: long runs) in both
forms, whole projected_cg on the "ic" variant, us per breakpoint of an H*d Cauchy search with mA = 96, and the break-even
number of products per J.  (Not to be confused with tools/gram_timing.py, which times A_free A_free'.)

    python tools/gn_gram_timing.py [--out FILE] [--quick]
    python tools/gn_gram_timing.py --cg-fused [--out FILE] [--one]
    python tools/gn_gram_timing.py --gram-read [--out FILE]

--cg-fused: the CG iteration on a Gram-form handle with option gram_cg_fused 0 / 1 alternated in one process (same handle, same
subproblem): median of 5 bh_pcg_dev calls each, wall time per call / H*p products, with the min - max spread; box constraints
at config 2, config 3 and n = 8192, and config 3 with 64 ("config-5 shape") and 8 linear equalities (A = u(4, .)).
--one: a single pair of calls on the config-5 shape with the option on, nothing else (rocprofv3 kernel traces).
--gram-read: the three read modes of a Gram-form handle (bh_hess_set_gram_read) at config 3 and n = 8192 (wider handles are not served): back-to-back
bh_time_kernel kind 10 (the product the handle performs), kind 11 (one quadratic form from G) and, for comparison, kind 1 (the J v
sweep a vthv costs); median of 5 blocks of 20 launches (min - max), with the bytes each one is specified to read.  A library built
before the switch existed gives the "full" rows only (A/B against an older commit in one session).
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


def say(s):
    print(s, flush=True)
    LINES.append(s)


def pcg_us(H, cons, dv, reps):
    """Average wall time of one device-resident projected_cg (bh_pcg_dev) and its iteration count."""
    st, it, nh = bh.operators.projected_cg_dev(dv["g"], H, dv["wl"], dv["wu"], cons, 0.1, dv["w"])     # warm-up (and the build of G)
    t0 = time.perf_counter()
    for _ in range(reps):
        st, it, nh = bh.operators.projected_cg_dev(dv["g"], H, dv["wl"], dv["wu"], cons, 0.1, dv["w"])
    return 1e6 * (time.perf_counter() - t0) / reps, int(st), it, nh


def instance(d, n, kind):
    syn = bh.synthetic
    H = bh.AlHessian.synthetic(d, n, seed=1, colscale=syn.column_scale(n, kind), mu=10.0)
    x, x_l, x_u, fix = syn.box_vectors(n, fix_every=8)
    cons = bh.MixedConstraints(np.zeros((0, n)), None, fix, l=x_l, u=x_u)
    g = H.jtv(syn.residual_rows(0, d))
    w_l, w_u = syn.step_bounds(x, x_l, x_u, fix, syn.initial_tr(g))
    dv = {k: bh.DeviceVector(n, v) for k, v in (("g", g), ("wl", w_l), ("wu", w_u))}
    dv["w"] = bh.DeviceVector(n)
    return H, cons, dv, dict(x=x, x_l=x_l, x_u=x_u, g=g)


def cg_fused_mode(args):
    syn = bh.synthetic
    shapes = [("config 2", 8192, 1024, [0]), ("config 3", 65536, 4096, [0, 64, 8]), ("n = 8192", 32768, 8192, [0])]
    if args.one:
        shapes = [("config 3", 65536, 4096, [64])]
    say("# tools/gn_gram_timing.py --cg-fused: CG iteration on a Gram-form handle, option gram_cg_fused 0 / 1 alternated in one process, one "
        "MI355X; wall time of bh_pcg_dev / H*p products, median of 5 calls (min - max); ic columns, kappa2 = 0.1")
    for label, d, n, mas in shapes:
        H, cons_box, dv, v = instance(d, n, 1)
        H.set_form("gram")
        _, _, _, fix = syn.box_vectors(n, fix_every=8)
        for mA in mas:
            cons = cons_box
            if mA:
                A = syn.splitmix_uniform(4, np.arange(mA * n)).reshape((mA, n), order="F")
                cons = bh.MixedConstraints(A, None, fix, l=v["x_l"], u=v["x_u"])
            run = lambda: bh.operators.projected_cg_dev(dv["g"], H, dv["wl"], dv["wu"], cons, 0.1, dv["w"])
            times, seen = {0: [], 1: []}, {}
            try:
                for opt in ((1, 1) if args.one else (0, 1)):         # preheat: the build of G, both shapes once
                    bh.set_option("gram_cg_fused", opt)
                    run()
                for _ in range(0 if args.one else 5):
                    for opt in (0, 1):
                        bh.set_option("gram_cg_fused", opt)
                        t0 = time.perf_counter()
                        st, it, nh = run()
                        times[opt].append(1e6 * (time.perf_counter() - t0) / max(nh, 1))
                        seen[opt] = (int(st), it, nh, H.stats()["cg_kernels"])
            finally:
                bh.set_option("gram_cg_fused", 0)
            if args.one:
                continue
            med = {o: float(np.median(times[o])) for o in (0, 1)}
            spread = max(max(times[o]) - min(times[o]) for o in (0, 1))
            verdict = "faster" if med[0] - med[1] > spread else "slower" if med[1] - med[0] > spread else "no difference beyond the spread"
            say("%s (d = %d, n = %d, mA = %d): option 0: status %d, %d H*p, cg_kernels %d, %.1f us per iteration (%.1f - %.1f); "
                "option 1: status %d, %d H*p, cg_kernels %d, %.1f us per iteration (%.1f - %.1f); %.2fx, %s"
                % (label, d, n, mA, seen[0][0], seen[0][2], seen[0][3], med[0], min(times[0]), max(times[0]),
                   seen[1][0], seen[1][2], seen[1][3], med[1], min(times[1]), max(times[1]), med[0] / med[1], verdict))
            if mA:
                cons.close()
        H.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


def gram_read_mode(args):
    import ctypes as ct
    lib = bh._lib.lib()
    setter = getattr(lib, "bh_hess_set_gram_read", None)
    if setter is not None:
        setter.argtypes, setter.restype = [ct.c_void_p, ct.c_int32], ct.c_int32
    say("# tools/gn_gram_timing.py --gram-read: G·v (bh_time_kernel kind 10), v'Gv from G (kind 11) and the J v sweep (kind 1) under the "
        "read modes of bh_hess_set_gram_read, one MI355X; us per launch, median of 5 blocks of 20 back-to-back launches (min - max)")

    def med(H, kind):
        t = [1e3 * H.time_kernel(kind, reps=20) for _ in range(5)]
        return "%.1f us (%.1f - %.1f)" % (float(np.median(t)), min(t), max(t))

    for label, d, n in [("config 3", 65536, 4096), ("n = 8192", 32768, 8192)]:          # (8192 < n <= 16384 is not served)
        ld = (n + 15) // 16 * 16
        H = bh.AlHessian.synthetic(d, n, seed=1, colscale=bh.synthetic.column_scale(n, 1), mu=10.0)
        H.set_form("gram")
        full, tri = 8.0 * n * ld + 16.0 * n, 16.0 * sum(i // 2 + 1 for i in range(n)) + 16.0 * n
        say("%s (d = %d, n = %d): J v sweep %s, %.0f bytes; full read %.0f bytes, lower triangle %.0f bytes (slab traffic not "
            "counted)" % (label, d, n, med(H, 1), 8.0 * d * ld + 8.0 * n, full, tri))
        for mode, name in enumerate(("full", "lower", "lower+quad")):
            if mode and setter is None:
                say("    (this library has no bh_hess_set_gram_read: the full read only)")
                break
            if setter is not None:
                bh._lib.check(setter(H.handle, mode), "bh_hess_set_gram_read")
            row = "    %-10s G·v %s, bytes_per_hmul %.0f" % (name, med(H, 10), H.stats()["bytes_per_hmul"])
            if setter is not None:
                try:
                    row += "; v'Gv from G %s" % med(H, 11)
                except bh.BenlsipHipError:
                    row += "; v'Gv from G: width not served"
            say(row)
        H.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="config 2 and 3 only, no Cauchy search (rocprofv3 runs)")
    ap.add_argument("--cg-fused", action="store_true", help="option gram_cg_fused 0 / 1 alternated on Gram-form handles")
    ap.add_argument("--one", action="store_true", help="with --cg-fused: two calls on the config-5 shape with the option on, nothing else")
    ap.add_argument("--gram-read", action="store_true", help="bh_time_kernel kinds 10, 11 and 1 under the three read modes of bh_hess_set_gram_read")
    args = ap.parse_args()
    bh.init(0)
    if args.cg_fused:
        cg_fused_mode(args)
        return
    if args.gram_read:
        gram_read_mode(args)
        return
    shapes = [("config 2", 8192, 1024), ("config 3", 65536, 4096)]
    if not args.quick:
        shapes += [("n = 8192", 32768, 8192), ("n = 16384", 16384, 16384)]
    say("# tools/gn_gram_timing.py: explicit Gram form (bh_hess_set_form) vs implicit, one MI355X; times are hipEvent (kernels) or wall (calls)")
    for label, d, n in shapes:
        ld = (n + 15) // 16 * 16
        H, cons, dv, _ = instance(d, n, 1)                  # "ic": columns scaled 10^(-3j/n), long CG runs
        t_imp_hmul = 1e3 * H.time_kernel(0, reps=10)
        us_imp, st_imp, it_imp, nh_imp = pcg_us(H, cons, dv, 3)
        H.set_form("gram")
        ms_build = H.time_kernel(9, reps=3)
        flop = 2.0 * d * n * (n + 1) / 2
        gv = 1e3 * H.time_kernel(10, reps=50)
        us_gram, st_gram, it_gram, nh_gram = pcg_us(H, cons, dv, 3)
        per_imp, per_gram = us_imp / max(nh_imp, 1), us_gram / max(nh_gram, 1)
        say("%s (d = %d, n = %d, ic): build of G %.3f ms = %.1f TFLOP/s (useful lower-triangle flop %.3g); G·v %.1f us = %.0f GB/s; "
            "implicit fused H*p %.1f us"
            % (label, d, n, ms_build, flop / (ms_build * 1e-3) / 1e12, flop, gv, 8.0 * n * ld / (gv * 1e-6) / 1e9, t_imp_hmul))
        say("    projected_cg (bh_pcg_dev): implicit %.1f us, status %d, %d iterations, %d H*p = %.1f us per H*p; Gram %.1f us, status %d, "
            "%d iterations, %d H*p = %.1f us per H*p  (%.2fx per iteration)"
            % (us_imp, st_imp, it_imp, nh_imp, per_imp, us_gram, st_gram, it_gram, nh_gram, per_gram, per_imp / per_gram))
        saved = per_imp - per_gram
        say("    break-even: the build (%.3f ms) pays for itself after %s products per J (saving %.1f us per CG iteration)"
            % (ms_build, "%.0f" % (1e3 * ms_build / saved) if saved > 0 else "never", saved))
        H.close()
    if args.quick:
        return
    # Cauchy search with 96 linear equalities at config-3 scale: one H*d per breakpoint (the row-space form stops at 64)
    syn = bh.synthetic
    d, n, mA = 65536, 4096, 96
    H, cons0, dv, v = instance(d, n, 0)
    A = syn.splitmix_uniform(4, np.arange(mA * n)).reshape((mA, n), order="F")
    for form in ("implicit", "gram"):
        H.set_form(form)
        cons = bh.MixedConstraints(A, None, None, l=v["x_l"], u=v["x_u"])
        delta = 1.0 * syn.initial_tr(v["g"])
        bh.cauchy_step(v["x"], v["g"], H, cons, delta)
        cons = bh.MixedConstraints(A, None, None, l=v["x_l"], u=v["x_u"])
        t0 = time.perf_counter()
        s, info = bh.cauchy_step(v["x"], v["g"], H, cons, delta, full_output=True)
        el = time.perf_counter() - t0
        say("cauchy_step config 3, mA = 96, %s form: %d breakpoints, %d passes, %.2f ms, %.1f us per pass, |s| = %.12e"
            % (form, info["n_breakpoints"], info["n_hmul"], 1e3 * el, 1e6 * el / max(info["n_hmul"], 1), np.linalg.norm(s)))
    H.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
