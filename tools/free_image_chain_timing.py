#!/usr/bin/env python3
"""What option free_image_chain saves the resident inner-step chain, at the config-3 shape (65536 x 4096, every 8th variable fixed,
mu = 10, kappa2 = 0.1): on resident vectors under step_from_cg = 1, one chain is

    ITERATES x (bh_minor_iterate_dev, bh_step_accumulate_dev), then bh_model_reduction_dev

started from s = 0 and g_minor = H s + g written by bh_hmul_add_dev (outside the timed region, as is the reset of the active set).
free_image_chain is alternated 0 / 1 in one process on one handle.

Regime 1, a stationary active set under free_image = 2 with the image in place: the well-conditioned instance (2 products per call)
and the ill-conditioned one (columns scaled by 10^(-3j/n), about 23 products in the first call).
Regime 2, a set that grows by 1 / 8 / 64 variables between the iterates under free_image = 1: the policy of bh_free_image_plan.h decides
per call whether the columns are moved out or the call streams J.  Before every chain the initial set is pushed again and bh_pcg_dev
calls run (untimed) until the policy has the image in place for it, on both sides alike.

Per side: the median over BLOCKS blocks of CHAINS chains, with the min - max spread, the products of every iterate of the last chain,
how many minor iterates of a chain were served from the image, and the growth of n_hmul / n_jv outside the CG loops.

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
ITERATES = 4
CHAINS = 5
PREHEAT = 4
D, N = 65536, 4096


class Chain:
    def __init__(self, H, cons, dv, host, delta):
        self.H, self.cons, self.dv, self.host, self.delta = H, cons, dv, host, delta
        self.lib = bh._lib.lib()
        self.status, self.iters, self.n_hmul, self.alpha = ct.c_int32(-1), ct.c_int32(0), ct.c_int32(0), ct.c_double(0.0)
        self.mr = ct.c_double(0.0)
        self.zero = np.zeros(N)
        self.fix0 = host["fix"].copy()

    def check(self, rc, what):
        if rc != 0:
            bh._lib.check(rc, what)

    def reset(self, regime2):
        """s = 0, g_minor = H s + g by the library's own hand, the initial active set (and, regime 2, the image in place for it)."""
        lib, dv = self.lib, self.dv
        bh.set_option("step_from_cg", 0)
        if regime2:
            self.cons.fixvars = self.fix0.copy()
            self.cons._sync()
            for _ in range(64):
                if self.H.free_image_info(self.cons)["state"] == "valid":
                    break
                bench.run_steps(bh, self.H, self.cons, dv, KAPPA2, 1)
        dv["s"].upload(self.zero)
        self.check(lib.bh_hmul_add_dev(self.H.handle, dv["s"].ptr, dv["g"].ptr, dv["gm"].ptr), "bh_hmul_add_dev")
        bh.set_option("step_from_cg", 1)
        lib.bh_synchronize()

    def run(self, grow, order):
        """One chain; grow > 0: that many more variables are fixed between two iterates.  -> (seconds, products per iterate)."""
        lib, dv, H, P = self.lib, self.dv, self.H.handle, self.cons
        products = []
        fix = self.fix0.copy()
        taken = 0
        t0 = time.perf_counter()
        for it in range(ITERATES):
            if grow > 0 and it > 0:
                fix[order[taken:taken + grow]] = True
                taken += grow
                P.fixvars = fix.copy()
                P._sync()
            self.check(lib.bh_minor_iterate_dev(H, P.handle, dv["x"].ptr, dv["s"].ptr, dv["gm"].ptr, dv["xl"].ptr, dv["xu"].ptr,
                                                ct.c_double(self.delta), ct.c_double(KAPPA2), ct.c_double(bh.operators.SQRT_EPS),
                                                ct.c_double(1e-10), dv["w"].ptr, ct.byref(self.status), ct.byref(self.iters),
                                                ct.byref(self.n_hmul), ct.byref(self.alpha)), "bh_minor_iterate_dev")
            products.append(self.n_hmul.value)
            self.check(lib.bh_step_accumulate_dev(H, dv["s"].ptr, dv["w"].ptr, dv["g"].ptr, dv["gm"].ptr), "bh_step_accumulate_dev")
        self.check(lib.bh_model_reduction_dev(H, dv["g"].ptr, dv["s"].ptr, ct.byref(self.mr)), "bh_model_reduction_dev")
        lib.bh_synchronize()
        return time.perf_counter() - t0, products


def measure(ch, sides, blocks, regime2, grow, order):
    def side_on(side):
        if side is not None:
            bh.set_option("free_image_chain", side)

    for side in sides:
        side_on(side)
        for _ in range(PREHEAT):
            ch.reset(regime2)
            ch.run(grow, order)
    times = {side: [] for side in sides}
    for _ in range(blocks):
        for side in sides:                                              # alternated: both sides see the same clocks
            side_on(side)
            total = 0.0
            for _ in range(CHAINS):
                ch.reset(regime2)
                t, _p = ch.run(grow, order)
                total += t
            times[side].append(total / CHAINS)
    res = {}
    for side in sides:
        side_on(side)
        ch.reset(regime2)
        served, st0 = ch.H.free_image_info(None)["calls_served"], ch.H.stats()
        _t, products = ch.run(grow, order)
        st1 = ch.H.stats()
        ts = 1e6 * np.array(times[side])
        name = "parent / baseline-only" if side is None else "free_image_chain = %d" % side
        print("%s: %.1f us per chain (median of %d blocks of %d chains, min %.1f max %.1f, spread %.1f) = %.1f us per iterate; products per "
              "iterate %s; minor iterates served from the image %d of %d; n_hmul outside the CG loops %+d, n_jv %+d; model reduction %r" % (
                  name, np.median(ts), len(ts), CHAINS, ts.min(), ts.max(), ts.max() - ts.min(), np.median(ts) / ITERATES, products,
                  ch.H.free_image_info(None)["calls_served"] - served, ITERATES, st1["n_hmul"] - st0["n_hmul"] - sum(products),
                  st1["n_jv"] - st0["n_jv"], ch.mr.value), flush=True)
        res[side] = (float(np.median(ts)), ch.mr.value, ch.dv["s"].download())
    if len(sides) == 2:
        (m0, q0, s0), (m1, q1, s1) = res[0], res[1]
        print("side 1 against side 0: %.1f -> %.1f us per chain (%+.1f %%); ||ds|| / ||s|| = %.2e; model reduction differs by %.2e (relative)" % (
            m0, m1, 100.0 * (m1 - m0) / m0, np.linalg.norm(s1 - s0) / np.linalg.norm(s0), abs(q1 - q0) / abs(q0)), flush=True)
        bh.set_option("free_image_chain", 0)
    bh.set_option("step_from_cg", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-only", action="store_true", help="one side, the option is never named")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--regimes", default="1,2")
    args = ap.parse_args()
    assert args.blocks >= 5
    bh.init(0)
    sides = (None,) if args.baseline_only else (0, 1)
    regimes = args.regimes.split(",")
    for kind, label in ((0, "well-conditioned"), (1, "ill-conditioned")):
        if kind == 1 and "1" not in regimes:
            continue
        H, cons, dv, host = bench.setup_instance(bh, 0, 1, kind, d_per_gpu=D, n=N)
        nfix = int(host["fix"].sum())
        delta = bh.synthetic.initial_tr(host["g"])
        for k, v in (("x", host["x"]), ("s", np.zeros(N)), ("gm", np.zeros(N)), ("xl", host["x_l"]), ("xu", host["x_u"])):
            dv[k] = bh.DeviceVector(N, v)
        ch = Chain(H, cons, dv, host, delta)
        order = np.random.default_rng(7).permutation(np.flatnonzero(~host["fix"]))
        if "1" in regimes:
            print("== regime 1, %s: J %d x %d, %d of %d variables fixed throughout, free_image = 2, kappa2 = %g, %d iterates per chain" % (
                label, D, N, nfix, N, KAPPA2, ITERATES), flush=True)
            bh.set_option("free_image", 2)
            bench.run_steps(bh, H, cons, dv, KAPPA2, 1)                  # builds the image
            info = H.free_image_info(cons)
            assert info["builds"] == 1 and info["state"] == "valid", info
            measure(ch, sides, args.blocks, False, 0, order)
        if "2" in regimes and kind == 0:
            bh.set_option("free_image", 1)
            for grow in (1, 8, 64):
                print("== regime 2, %s: %d fixed at the start, %d more between two iterates, free_image = 1 (the policy decides), %d iterates "
                      "per chain" % (label, nfix, grow, ITERATES), flush=True)
                measure(ch, sides, args.blocks, True, grow, order)
                info = H.free_image_info(None)
                print("    the handle's image so far: %d builds, %d columns moved, %d calls served" % (info["builds"], info["moves"],
                                                                                                    info["calls_served"]), flush=True)
        bh.set_option("free_image", 1)
        for v in dv.values():
            v.close()
        H.close()
        cons.close()


if __name__ == "__main__":
    main()
