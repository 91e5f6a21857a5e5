#!/usr/bin/env python3
"""Option gram_ingest (bh_hess_create_async builds G = J'J + mu C'C during the upload of J) against the sequence without it, from a
pageable host J at config 3 (65536 x 4096, 2 GiB) and config 2 (8192 x 1024, 64 MiB), alternated in one process:

    (a) option 0:  bh_hess_create_async -> bh_hess_wait -> bh_hess_set_form(GRAM) -> one bh_hmul_dev -> synchronise
    (b) option 1:  bh_hess_create_async -> bh_hess_wait ->                            one bh_hmul_dev -> synchronise

for upload_chunk_mb in {16, 64, 256}.  Per sequence: wall time from the create call to the end, and the time bh_hess_wait blocks
(it is called right after the create: in (a) that is the upload, in (b) the upload and whatever of the build is left behind the last
chunk — the tail is the difference).  Median of REPS >= 5 with the min - max spread after one warm-up of each; (b) is called faster
only when the medians differ by more than the larger of the two spreads.  Needs a GPU.

    python tools/gram_ingest_timing.py [--out FILE] [--reps N]      (FILE defaults to profiles/r11_gram_ingest_timing.txt)
    python tools/gram_ingest_timing.py --one                        (two (b) sequences at config 3, for a rocprofv3 kernel trace)
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
SHAPES = (("config 3", 65536, 4096), ("config 2", 8192, 1024))
CHUNKS_MB = (16, 64, 256)


def say(s):
    print(s, flush=True)
    LINES.append(s)


def host_jacobian(d, n):
    """Column-major, pageable, cheap to fill: 64 random columns repeated with a different scale per block of columns."""
    J = np.empty((d, n), order="F")
    base = np.random.default_rng(0).standard_normal((d, 64)) / np.sqrt(d)
    for c0 in range(0, n, 64):
        w = min(64, n - c0)
        J[:, c0:c0 + w] = base[:, :w] * (1.0 + 1e-3 * (c0 // 64))
    return J


def sequence(J, option, v_dev, out_dev):
    """One (a) or (b) sequence: (wall seconds, seconds blocked in bh_hess_wait, gram_builds at the end, the product)."""
    lib = bh._lib.lib()
    bh.set_option("gram_ingest", option)
    try:
        t0 = time.perf_counter()
        H = bh.AlHessian.create_async(J, None, 10.0)
        t1 = time.perf_counter()
        H.wait()
        t_wait = time.perf_counter() - t1
        if not option:
            H.set_form("gram")
        bh._lib.check(lib.bh_hmul_dev(H.handle, v_dev.ptr, out_dev.ptr), "bh_hmul_dev")
        bh._lib.check(lib.bh_synchronize(), "bh_synchronize")
        el = time.perf_counter() - t0
    finally:
        bh.set_option("gram_ingest", 0)
    builds = H.gram_builds
    hv = out_dev.download()
    H.close()
    return el, t_wait, builds, hv


def shape(label, d, n, reps):
    J = host_jacobian(d, n)
    v_dev, out_dev = bh.DeviceVector(n, np.random.default_rng(1).standard_normal(n)), bh.DeviceVector(n)
    say("%s: J %d x %d (%.0f MiB, pageable host memory)" % (label, d, n, J.nbytes / 2.0 ** 20))
    for mb in CHUNKS_MB:
        bh.set_option("upload_chunk_mb", mb)
        cc = max(32, ((mb << 20) // (8 * d)) // 32 * 32)
        cc = min(cc, (n + 31) // 32 * 32)
        t = {0: [], 1: []}
        w = {0: [], 1: []}
        hv = {}
        for opt in (0, 1):
            sequence(J, opt, v_dev, out_dev)                            # warm-up of each
        for _ in range(reps):
            for opt in (0, 1):                                          # alternated
                el, tw, builds, hv[opt] = sequence(J, opt, v_dev, out_dev)
                assert builds == 1
                t[opt].append(1e3 * el)
                w[opt].append(1e3 * tw)
        med = {o: float(np.median(t[o])) for o in (0, 1)}
        spread = {o: max(t[o]) - min(t[o]) for o in (0, 1)}
        wmed = {o: float(np.median(w[o])) for o in (0, 1)}
        rel = np.linalg.norm(hv[1] - hv[0]) / max(np.linalg.norm(hv[0]), 1e-300)
        say("    upload_chunk_mb = %3d (%d chunks of %d columns):" % (mb, -(-n // cc), cc))
        for o, name in ((0, "(a) option 0"), (1, "(b) option 1")):
            say("        %s: create -> end median %.2f ms (min %.2f, max %.2f, %d sequences); bh_hess_wait blocks %.2f ms (min %.2f, max %.2f)"
                % (name, med[o], min(t[o]), max(t[o]), len(t[o]), wmed[o], min(w[o]), max(w[o])))
        gain = med[0] - med[1]
        bar = max(spread.values())
        verdict = "(b) faster" if gain > bar else "(b) slower" if -gain > bar else "no difference beyond the spread"
        say("        -> (a) - (b) = %.2f ms against the larger spread %.2f ms: %s; tail of the build behind the upload (wait (b) - wait (a)) = %.2f ms; "
            "|G v (b) - G v (a)| / |G v| = %.1e" % (gain, bar, verdict, wmed[1] - wmed[0], rel))
    bh.set_option("upload_chunk_mb", 64)
    v_dev.close()
    out_dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_gram_ingest_timing.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", action="store_true", help="two (b) sequences at config 3 and nothing else (rocprofv3 kernel trace)")
    args = ap.parse_args()
    bh.init(0)
    if args.one:
        label, d, n = SHAPES[0]
        J = host_jacobian(d, n)
        v_dev, out_dev = bh.DeviceVector(n, np.ones(n)), bh.DeviceVector(n)
        for _ in range(2):
            el, tw, builds, _hv = sequence(J, 1, v_dev, out_dev)
            print("%s, option 1, 64 MiB chunks: create -> end %.2f ms, bh_hess_wait %.2f ms, gram_builds %d" % (label, 1e3 * el, 1e3 * tw, builds), flush=True)
        return
    say("# tools/gram_ingest_timing.py: option gram_ingest 0 / 1 alternated in one process, one MI355X; wall times")
    for label, d, n in SHAPES:
        shape(label, d, n, max(args.reps, 5))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
