"""Option cauchy_block = K without a GPU: the rule and its two helpers (csrc/bh_cauchy_plan.h, built by the host compiler with the
address and undefined-behaviour sanitizers) against a Python statement of the option's description; the launch structure of
cauchy_block_kernel<K> as a float64 model (tests/block_cases.py) against refresh_cases.carried_search, bit for bit; and the
launch-ahead schedule with the blocked parameters against a scripted device."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import block_cases as bc
import refresh_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")

MA = (0, 1)
COMM = (0, 1)
IMAGE = (0, 1)
FUSED = (0, 1)
REFRESH = (0, 5)
N = (1, 4096, 4097, 20000)
PANEL = (0, 1)
BLOCK = (0, 1, 2, 4, 8, 16)
LENGTHS = range(1, 71)
BATCH = (1, 2, 4)                        # the library runs the blocked search with first = 4, batch = 4
FIRST = 4
MAX_PASS = 70

PROGRAM = r"""
#include "bh_cauchy_plan.h"
#include "bh_launch_ahead.h"
#include <cstdio>
using namespace bh;

// The scripted device: unit 0 is launch 0, block launch b >= 1 takes the decisions up to pass cauchy_block_pass_target(b, K); the
// search is P passes long.  After e units the word holds min(decided, P) passes and done = (decided >= P).
struct Device {
    int K, P; bool drained;
    int enq = 0, seen = 0, bad = 0;
    MirrorWord word(int e) const {
        const int decided = e >= 1 ? cauchy_block_pass_target(e - 1, K) : 0;
        MirrorWord m{};
        m.done = decided >= P ? 1 : 0; m.n_hmul = decided < P ? decided : P; m.iter = m.n_hmul > 0 ? m.n_hmul - 1 : 0;
        return m;
    }
    int launch(int i) { if (i != enq) bad = 1; enq += 1; return 0; }
    int wait(int unit_target, MirrorWord* out) {
        const int nt = cauchy_block_pass_target(unit_target, K);             // what cauchy_impl's wait callable does
        auto ok = [&](const MirrorWord& m) { return m.done != 0 || m.n_hmul >= nt; };
        int e = drained ? enq : seen;
        while (e < enq && !ok(word(e))) ++e;
        if (!ok(word(e))) return 1;                                          // stream drained, target not reached
        seen = e; *out = word(e);
        return 0;
    }
};

int main() {
    const int ns[] = {1, 4096, 4097, 20000}, blocks[] = {0, 1, 2, 4, 8, 16}, Ks[] = {2, 4, 8, 16}, batches[] = {1, 2, 4};
    for (int mA = 0; mA < 2; ++mA) for (int comm = 0; comm < 2; ++comm) for (int image = 0; image < 2; ++image) for (int fused = 0; fused < 2; ++fused)
    for (long long refresh : {0ll, 5ll}) for (int n : ns) for (int panel = 0; panel < 2; ++panel) for (int blk : blocks) {
        CauchySelectIn in{};
        in.mA = mA; in.comm = comm != 0; in.multi_panel = panel != 0; in.last_cauchy_passes = -1;
        in.cauchy_image = image; in.cauchy_image_max_ma = 64; in.cauchy_fused = fused; in.cauchy_image_refresh = refresh;
        in.n = n; in.cauchy_block = blk;
        const CauchySelection s = cauchy_select(in);
        std::printf("R %d %d %d %d\n", (int)s.form, s.fused ? 1 : 0, s.refresh, s.block);
    }
    for (int K : Ks) {
        for (int t = 0; t <= 40; ++t) std::printf("T %d %d %d\n", K, t, cauchy_block_pass_target(t, K));
        for (int p = 1; p <= 70; ++p) std::printf("F %d %d %d\n", K, p, cauchy_block_final_launch(p, K));
    }
    for (long long v = -2; v <= 33; ++v) std::printf("V %lld %d\n", v, cauchy_block_value_ok(v) ? 1 : 0);
    for (int K : Ks) for (int P = 1; P <= 70; ++P) for (int batch : batches) for (int view = 0; view < 2; ++view) {
        LaunchAhead s{};
        s.off = 1; s.first = 3 + s.off; s.batch = batch; s.max_units = 2 + (70 + K - 1) / K;
        s.await_iter = false; s.lock_step = false; s.look_first = false;
        Device dev{K, P, view == 1};
        MirrorWord mw{};
        const int rc = launch_ahead(s, [&](int i) { return dev.launch(i); }, [&](int nt, int, MirrorWord* m) { return dev.wait(nt, m); }, &mw);
        std::printf("S %d %d %d %d %d %d %d %d %d\n", K, P, batch, view, rc, mw.done, mw.n_hmul, dev.enq, dev.bad);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("cauchy_block")
    src, exe = d / "block.cpp", d / "block"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    by = {}
    for ln in out:
        by.setdefault(ln[0], []).append([int(x) for x in ln[2:].split()])
    return by


# ------------------------------------------------------------------------------------------------------------------ 1. the rule
def test_block_follows_the_documented_rule(lines):
    """Fails without the feature (CauchySelectIn has no `cauchy_block`).  Full product of mA, communicator, cauchy_image,
    cauchy_fused, refresh 0 / 5, n = 1 / 4096 / 4097 / 20000, a multi-panel J and every accepted K: `block` = K exactly where the
    description says, 0 elsewhere — and form, fused, refresh are what they are without the option."""
    cases = list(itertools.product(MA, COMM, IMAGE, FUSED, REFRESH, N, PANEL, BLOCK))
    assert len(lines["R"]) == len(cases)
    seen = set()
    for (mA, comm, image, fused, refresh, n, panel, K), (form, one_kernel, interval, block) in zip(cases, lines["R"]):
        exp_form = 0 if not image else (1 if mA == 0 else 2)
        exp_one = int(exp_form == 1 and not comm and fused == 1)
        exp_interval = refresh if (exp_form in (1, 2) and not comm and not (exp_one and panel)) else 0
        assert (form, one_kernel, interval) == (exp_form, exp_one, exp_interval)
        assert block == bc.expected_block(form, one_kernel, comm, interval, n, K), (mA, comm, image, fused, refresh, n, panel, K, block)
        seen.add(block)
    assert seen == {0, 2, 4, 8, 16}


def test_helpers_and_accepted_values(lines):
    for K, t, got in lines["T"]:
        assert got == bc.pass_target(t, K)
    for K, p, got in lines["F"]:
        assert got == bc.final_launch(p, K)
        # the launch that takes decision p - 1 is the first whose target reaches p
        assert bc.pass_target(got, K) >= p and (got == 1 or bc.pass_target(got - 1, K) < p)
    assert {v for v, ok in lines["V"] if ok} == {0, 1, 2, 4, 8, 16}


def test_library_plumbs_the_option():
    api = open(os.path.join(CSRC, "bh_api.hip")).read()
    options = open(os.path.join(CSRC, "bh_options.h")).read()       # the key and its environment variable: one row of the option table
    assert '"cauchy_block"' in options and '"BH_CAUCHY_BLOCK"' in options and '#include "bh_options.h"' in api
    assert "cauchy_pass_rowspace_block" in api
    assert "cauchy_block_pass_target(" in api and "cauchy_block_final_launch(" in api
    assert '"cauchy_block"' in open(os.path.join(ROOT, "include", "benlsip_hip.h")).read()
    hdr = open(os.path.join(CSRC, "bh_cauchy_plan.h")).read()
    assert "hip" not in "".join(ln for ln in hdr.splitlines() if ln.lstrip().startswith("#include"))


# ------------------------------------------------------------------------------------------------------------------ 2. the model
def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def _check(inst, K, passes_expected=None):
    s_ref, fix_ref, passes = rc.carried_search(*inst, refresh=0)
    if passes_expected is not None:
        assert passes == passes_expected
    log = {}
    s, fix, p, err = bc.blocked_search(*inst, K, log=log)
    assert err == 0 and p == passes, (K, p, passes)
    assert np.array_equal(_bits(s), _bits(s_ref)), (K, passes)
    assert np.array_equal(fix, fix_ref), (K, passes)                      # no speculative mark in the active set
    assert log["launches"] == bc.final_launch(passes, K) and log["buffer"] == log["launches"] % 3
    return log


@pytest.mark.parametrize("K", bc.KS)
@pytest.mark.parametrize("npass", bc.NPASS)
def test_model_equals_the_carried_search_on_exact_instances(npass, K):
    log = _check(bc.exact(40, 48, 3, npass), K, npass)
    # (a search that ends inside a block threw its run-ahead away: at most K - 1 advances, once)
    assert 0 <= log["wasted"] <= K - 1


def test_every_ending_offset_is_reached():
    """The lengths above end at every offset inside a block for K = 2 and 4, at the first, last and a middle one for 8 and 16."""
    for K, need in ((2, {0, 1}), (4, {0, 1, 2, 3}), (8, {0, 3, 7}), (16, {0, 7, 15})):
        offs = {(p - 1) % K for p in bc.NPASS if p > 1}
        assert need <= offs, (K, offs)


@pytest.mark.parametrize("K", bc.KS)
@pytest.mark.parametrize("name,inst", list(bc.named_cases()), ids=[n for n, _ in bc.named_cases()])
def test_model_equals_the_carried_search_on_the_edges(name, inst, K):
    log = _check(inst, K)
    s_ref, fix_ref, passes = rc.carried_search(*inst, refresh=0)
    n = inst[0].shape[1]
    if name == "bad_instance_d300":
        assert passes == 121
    if name.startswith("all_fixed"):
        assert passes == n + 1 and fix_ref.all()
    if name == "stationary_at_pass_0":
        assert passes == 1 and not fix_ref.any() and log["launches"] == 1
    if name == "tie_in_block":
        seq = bc.sequential_search(*inst)
        assert seq[2] == passes == 9


@pytest.mark.parametrize("K", bc.KS)
def test_tie_takes_the_smaller_index_first(K):
    """Two variables with the same theta at pass 2: a model that broke the tie the other way would fix the same set but pass through
    another order — seen in fixpass; here through the step: the second of the pair advances with theta = 0."""
    inst = bc.tie_in_block()
    J, C, mu, x, g, xlow, xupp, delta = inst
    hit = np.flatnonzero(xupp < 1024.0)
    ratios = np.sort(xupp[hit] / -g[hit])
    assert ratios[2] == ratios[3]
    _check(inst, K, 9)


@pytest.mark.parametrize("K", bc.KS)
def test_no_breakpoint_left_raises_the_error_flag_at_pass_0(K):
    inst = bc.no_breakpoint()
    s_seq, fix_seq, p_seq, err_seq = bc.sequential_search(*inst)
    s, fix, p, err = bc.blocked_search(*inst, K)
    assert (p, err) == (p_seq, err_seq) == (1, 1)
    assert np.array_equal(_bits(s), _bits(s_seq)) and np.array_equal(fix, fix_seq) and not fix.any()


def test_sequential_restatement_is_the_carried_search():
    """sequential_search (the reference for the error path) gives carried_search's bits wherever that one runs."""
    for inst in [bc.exact(40, 48, 3, 9)] + [i for _, i in bc.named_cases()]:
        a = rc.carried_search(*inst, refresh=0)
        b = bc.sequential_search(*inst)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2] and b[3] == 0


# ------------------------------------------------------------------------------------------------------------------ 3. the schedule
def test_blocked_schedule_ends_every_search(lines):
    """launch_ahead with off = 1, first = 4, batch <= first, lock_step = false, max_units = 2 + ceil(max_pass / K) and the wait callable translating
    unit targets with cauchy_block_pass_target: every search length 1 .. 70 ends, for both views of the device; the units enqueued
    stay below units needed + first + batch (the host looks two batches behind what it has enqueued: 2 batch - 1 units past the end at
    the most); the final word carries the true pass count."""
    assert len(lines["S"]) == len(bc.KS) * len(LENGTHS) * len(BATCH) * 2
    for K, P, batch, view, rcode, done, n_hmul, enq, bad in lines["S"]:
        needed = 1 + bc.final_launch(P, K)
        assert rcode == 0 and done == 1 and n_hmul == P and bad == 0, (K, P, batch, view)
        assert needed <= enq <= needed + FIRST + batch - 1, (K, P, batch, view, enq, needed)
        assert enq <= 2 + -(-MAX_PASS // K)
