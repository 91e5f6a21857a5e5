"""The launch-ahead schedule (csrc/bh_launch_ahead.h: launch_ahead, no HIP in it) against literal transcriptions of the five host
loops it replaced: a stand-alone program built by the host compiler (with the address and undefined-behaviour sanitizers) drives the
header against a scripted device and prints every event — `L i` (launch unit i) and `W n_hmul_target iter_target` with the word the
wait returned — and each event list is compared with what the transcribed loop does against the same device.

The device: the loop ends at product K.  A unit stands for one product (`off` units later in the one-kernel Cauchy pass): after u units
the word holds n_hmul = min(u - off, K) and done = (u - off >= K).  In the shapes that await `iter`, S(1) goes out in front of the loop
and unit u enqueues S(u + 1): S(j) publishes iter = j while the loop goes on, S(K + 1) publishes `done`.  A wait returns either the
least advanced word that satisfies it ("eager": the host polled as early as it could) or the word after everything enqueued has run
("drained": the host polled late).  "Never ends early" is the loop that stops at its own bound, the last product the units allow."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")

MAX_UNITS = (1, 2, 3, 7, 33, 70)
HISTORY = (0, 1, 5, 32, 33, 40)
BATCH = (1, 2, 4, 8)
VIEWS = ("eager", "drained")
FIRST_BATCH_CAP = 32
NEVER = 0x7fffffff
# name -> (off, awaits iter, lock-step)
SETS = {
    "fused": (0, True, False),
    "fused_rccl_eq": (0, True, True),
    "rccl_box": (0, False, True),
    "separate": (0, False, True),
    "separate_rccl": (0, False, True),
    "cauchy": (0, False, True),
    "cauchy_fused": (1, False, True),
}

PROGRAM = r"""
#include "bh_launch_ahead.h"
#include <cstdio>
#include <string>
using namespace bh;

struct Device {
    int K, off; bool iter_shape, drained;
    int enq = 0, seen = 0;
    std::string log;
    MirrorWord word(int u) const {
        const int prod = u > off ? u - off : 0;
        MirrorWord m{};
        m.done = prod >= K ? 1 : 0; m.status = 0; m.n_hmul = prod < K ? prod : K;
        m.iter = iter_shape ? (prod < K ? prod + 1 : K + 1) : m.n_hmul;
        return m;
    }
    int launch(int i) {
        log += "L " + std::to_string(i) + ";";
        if (i != enq) log += "X out of order;";
        enq += 1;
        return 0;
    }
    int wait(int nt, int it, MirrorWord* out) {
        auto ok = [&](const MirrorWord& m) { return m.done != 0 || m.n_hmul >= nt || (it > 0 && m.iter >= it); };
        int u = drained ? enq : seen;
        while (u < enq && !ok(word(u))) ++u;
        log += "W " + std::to_string(nt) + " " + std::to_string(it);
        if (!ok(word(u))) { log += " X stream drained but the loop state did not reach the launch target;"; return 1; }
        seen = u; *out = word(u);
        log += " -> " + std::to_string(out->done) + " " + std::to_string(out->n_hmul) + " " + std::to_string(out->iter) + ";";
        return 0;
    }
};

int main() {
    const int maxes[] = {1, 2, 3, 7, 33, 70}, hists[] = {0, 1, 5, 32, 33, 40}, batches[] = {1, 2, 4, 8};
    // fused, fused_rccl_eq, rccl_box, separate, separate_rccl, cauchy, cauchy_fused
    for (int set = 0; set < 7; ++set) for (int M : maxes) for (int hist : hists) for (int batch : batches) {
        LaunchAhead s{};
        s.max_units = M; s.batch = batch; s.off = set == 6 ? 1 : 0;
        s.await_iter = set <= 1; s.lock_step = set != 0; s.look_first = set < 5;
        const int cold = set == 0 ? (batch < 2 ? batch : 2) : set == 3 ? (batch < 2 ? batch : 2) : 1;
        s.first = set < 5 ? launch_ahead_first(hist, cold) : 2 + s.off;
        const int last = M - s.off;                       // the last product the units allow
        for (int k = 1; k <= last + 1; ++k) for (int view = 0; view < 2; ++view) {
            Device dev{k <= last ? k : last, s.off, s.await_iter, view == 1};      // (k = last + 1: never ends early)
            MirrorWord mw{};
            const int rc = launch_ahead(s, [&](int i) { return dev.launch(i); }, [&](int nt, int it, MirrorWord* m) { return dev.wait(nt, it, m); }, &mw);
            std::printf("%d %d %d %d %d %d|%d %d|%s\n", set, M, hist, batch, k <= last ? k : -1, view, rc, mw.done, dev.log.c_str());
        }
    }
    return 0;
}
"""


class Device:
    """The scripted device of the module docstring, once more (the program has its own)."""

    def __init__(self, K, off, iter_shape, drained):
        self.K, self.off, self.iter_shape, self.drained = K, off, iter_shape, drained
        self.enq = self.seen = 0
        self.log = []

    def word(self, u):
        prod = max(u - self.off, 0)
        done = int(prod >= self.K)
        n_hmul = min(prod, self.K)
        it = min(prod + 1, self.K + 1) if self.iter_shape else n_hmul
        return done, n_hmul, it

    def launch(self, i):
        assert i == self.enq
        self.log.append("L %d" % i)
        self.enq += 1

    def wait(self, nt, it=0):
        def ok(w):
            return w[0] != 0 or w[1] >= nt or (it > 0 and w[2] >= it)
        u = self.enq if self.drained else self.seen
        while u < self.enq and not ok(self.word(u)):
            u += 1
        assert ok(self.word(u)), "stream drained but the loop state did not reach the launch target"
        self.seen = u
        w = self.word(u)
        self.log.append("W %d %d -> %d %d %d" % (nt, it, w[0], w[1], w[2]))
        return w


class Mw:
    def __init__(self):
        self.done = self.n_hmul = self.iter = 0

    def set(self, w):
        self.done, self.n_hmul, self.iter = w


# ---- the parent's loops, line by line (csrc/bh_api.hip of the commit before the scheduler) ---------------------------------

def parent_fused(dev, max_iter, last_n_hmul, batch):
    """bh_api.hip:2710-2723, 2747-2761: the fused shape on one rank / over the peer buffers."""
    launched = 0                                                     # :2710
    mw = Mw()

    def launch_batch(nb):                                            # :2711-2720
        nonlocal launched
        nb = min(nb, max_iter - launched)
        for _ in range(nb):
            dev.launch(launched)                                     # launch_update(launched + 1), launch_stream(launched + 2)
            launched += 1
    first = min(last_n_hmul, FIRST_BATCH_CAP) if last_n_hmul > 0 else min(batch, 2)     # :2747
    launch_batch(first)                                              # :2748
    mw.set(dev.wait(NEVER, launched + 1))                            # :2750
    if not mw.done and launched < max_iter:                          # :2751
        launch_batch(batch)                                          # :2752
        while True:                                                  # :2753
            target = launched                                        # :2754
            more = launched < max_iter                               # :2755
            if more:
                launch_batch(batch)                                  # :2756
            mw.set(dev.wait(NEVER, target + 1))                      # :2757
            if mw.done or not more:                                  # :2758
                break
    mw.set(dev.wait(NEVER))                                          # :2761
    return mw


def parent_fused_rccl_eq(dev, max_iter, last_n_hmul, batch):
    """bh_api.hip:2710-2745: the fused shape with equalities over RCCL."""
    launched = 0
    mw = Mw()

    def launch_batch(nb):                                            # :2711-2720
        nonlocal launched
        nb = min(nb, max_iter - launched)
        for _ in range(nb):
            dev.launch(launched)
            launched += 1

    def done_by(target):                                             # :2728
        return mw.done and mw.n_hmul <= target
    launch_batch(min(last_n_hmul, FIRST_BATCH_CAP) if last_n_hmul > 0 else 1)      # :2729
    mw.set(dev.wait(NEVER, launched + 1))                            # :2730
    if not done_by(launched) and launched < max_iter:                # :2731
        launch_batch(batch)                                          # :2732
        while True:                                                  # :2733
            target = launched                                        # :2734
            more = launched < max_iter                               # :2735
            if more:
                launch_batch(batch)                                  # :2736
            mw.set(dev.wait(NEVER, target + 1))                      # :2737
            if done_by(target) or not more:                          # :2738
                break
    mw.set(dev.wait(NEVER))                                          # :2741
    return mw


def parent_rccl_box(dev, max_iter, last_n_hmul, batch):
    """bh_api.hip:2826-2849: box constraints over RCCL, two kernels and the collective."""
    launched = 0                                                     # :2827
    mw = Mw()

    def launch_batch(nb):                                            # :2828-2833
        nonlocal launched
        nb = min(nb, max_iter - launched)
        for i in range(nb):
            dev.launch(launched + i)
        launched += nb

    def done_by(target):                                             # :2835
        return mw.done and mw.n_hmul <= target
    first = min(last_n_hmul, FIRST_BATCH_CAP) if last_n_hmul > 0 else 1           # :2836
    launch_batch(first)                                              # :2837
    mw.set(dev.wait(launched))                                       # :2838
    if not done_by(launched) and launched < max_iter:                # :2839
        launch_batch(batch)                                          # :2840
        while True:                                                  # :2841
            target = launched                                        # :2842
            more = launched < max_iter                               # :2843
            if more:
                launch_batch(batch)                                  # :2844
            mw.set(dev.wait(target))                                 # :2845
            if done_by(target) or not more:                          # :2846
                break
    mw.set(dev.wait(launched))                                       # :2849
    return mw


def parent_separate(dev, max_iter, last_n_hmul, batch, rccl_path):
    """bh_api.hip:2894-2926: the separate-kernel shape."""
    launched = 0                                                     # :2895
    mw = Mw()

    def launch_batch(nb):                                            # :2896-2901
        nonlocal launched
        nb = min(nb, max_iter - launched)
        for i in range(nb):
            dev.launch(launched + i)
        launched += nb

    def done_by(target):                                             # :2908
        return mw.done and mw.n_hmul <= target
    first = min(last_n_hmul, FIRST_BATCH_CAP) if last_n_hmul > 0 else min(batch, 1 if rccl_path else 2)     # :2913
    launch_batch(first)                                              # :2914
    mw.set(dev.wait(launched))                                       # :2915
    if not done_by(launched) and launched < max_iter:                # :2916
        launch_batch(batch)                                          # :2917
        while True:                                                  # :2918
            target = launched                                        # :2919
            more = launched < max_iter                               # :2920
            if more:
                launch_batch(batch)                                  # :2921
            mw.set(dev.wait(target))                                 # :2922
            if done_by(target) or not more:                          # :2923
                break
    mw.set(dev.wait(launched))                                       # :2926
    return mw


def parent_cauchy(dev, max_launch, batch, off):
    """bh_api.hip:3835-3856: cauchy_impl (max_launch = max_pass + off; the history of the handle plays no part)."""
    launched = 0                                                     # :3822
    mw = Mw()

    def launch_batch(nb):                                            # :3839-3844
        nonlocal launched
        nb = min(nb, max_launch - launched)
        for i in range(nb):
            dev.launch(launched + i)
        launched += nb

    def done_by(target):                                             # :3847
        return mw.done and mw.n_hmul <= target
    launch_batch(2 + off)                                            # :3848
    while True:                                                      # :3849
        target = launched - off                                      # :3850
        more = launched < max_launch                                 # :3851
        if more:
            launch_batch(batch)                                      # :3852
        mw.set(dev.wait(target))                                     # :3853
        if done_by(target) or not more:                              # :3854
            break
    mw.set(dev.wait(launched - off))                                 # :3856
    return mw


def transcription(name, dev, M, hist, batch):
    if name == "fused":
        return parent_fused(dev, M, hist, batch)
    if name == "fused_rccl_eq":
        return parent_fused_rccl_eq(dev, M, hist, batch)
    if name == "rccl_box":
        return parent_rccl_box(dev, M, hist, batch)
    if name == "separate":
        return parent_separate(dev, M, hist, batch, False)
    if name == "separate_rccl":
        return parent_separate(dev, M, hist, batch, True)
    return parent_cauchy(dev, M, batch, SETS[name][0])


@pytest.fixture(scope="module")
def header_runs(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("launch_ahead")
    src, exe = d / "sched.cpp", d / "sched"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    runs = {}
    for line in out:
        key, res, log = line.split("|")
        rc, done = (int(x) for x in res.split())
        runs[tuple(int(x) for x in key.split())] = (rc, done, [e for e in log.split(";") if e])
    return runs


def cases():
    for si, name in enumerate(SETS):
        off = SETS[name][0]
        for M in MAX_UNITS:
            for hist in HISTORY:
                for batch in BATCH:
                    last = M - off
                    for k in list(range(1, last + 1)) + [-1]:
                        for vi, view in enumerate(VIEWS):
                            yield (si, M, hist, batch, k, vi), name, (k if k > 0 else last), view


def test_every_case_ran(header_runs):
    keys = [c[0] for c in cases()]
    assert len(keys) == len(set(keys)) == len(header_runs)
    assert set(keys) == set(header_runs)
    # 6 histories x 4 batches x 2 views x (sum over the maxima of K = 1..last and "never"), over the seven parameter sets
    assert len(keys) == 6 * 4 * 2 * (6 * sum(m + 1 for m in MAX_UNITS) + sum(m for m in MAX_UNITS))


def test_events_equal_the_transcribed_loops(header_runs):
    for key, name, K, view in cases():
        off, iter_shape, _ = SETS[name]
        dev = Device(K, off, iter_shape, view == "drained")
        mw = transcription(name, dev, key[1], key[2], key[3])
        rc, done, log = header_runs[key]
        assert rc == 0, (name, key, log)
        assert log == dev.log, (name, key, log, dev.log)
        assert done == mw.done == 1, (name, key)                     # the final wait sees `done`
        assert log[-1].startswith("W ") and " -> 1 " in log[-1], (name, key, log[-1])


def test_lock_step_launches_do_not_depend_on_when_the_host_polled(header_runs):
    """Rank independence: what a lock-step loop enqueues, and in which order against its waits' targets, is the same whether
    every wait saw the least or the most advanced word."""
    compared = 0
    for key, name, K, view in cases():
        if view != "eager" or not SETS[name][2]:
            continue
        other = header_runs[key[:5] + (1,)][2]
        strip = [e.split(" ->")[0] for e in header_runs[key][2]]
        assert strip == [e.split(" ->")[0] for e in other], (name, key)
        compared += 1
    assert compared > 0


def test_the_one_rank_fused_loop_is_the_only_one_that_uses_a_later_state(header_runs):
    """... and the loop that is not lock-step does enqueue less when it polls late (else the flag would be dead)."""
    differ = 0
    for key, name, K, view in cases():
        if name == "fused" and view == "eager":
            a = [e for e in header_runs[key][2] if e.startswith("L")]
            b = [e for e in header_runs[key[:5] + (1,)][2] if e.startswith("L")]
            assert len(b) <= len(a)
            differ += a != b
    assert differ > 0


def test_no_unit_beyond_the_maximum(header_runs):
    for key, (rc, done, log) in header_runs.items():
        units = [int(e.split()[1]) for e in log if e.startswith("L")]
        assert units == list(range(len(units))) and len(units) <= key[1], (key, log)
        assert not any("X" in e for e in log), (key, log)

