"""CPU tests of the policy behind the compact image of the free columns (option free_image): csrc/bh_free_image_plan.h (no HIP in
it) built into a stand-alone program by the host compiler, with the address and undefined-behaviour sanitizers, and driven over
generated call sequences — active sets that grow by a few variables, now and then lose one, under each value of the option.  The
program keeps a model of the image (one row whose entries are the column numbers) and applies the planned moves the way
free_image_move_kernel does; the properties are checked here, from its log."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")

# "K build launch column min_bytes", then per sequence "Q option rows n" and per call
# "C nfix present k_new k_freed credit last_n_hmul action n_hmul | present nfree ldf image_ok"
PROGRAM = r"""
#include "bh_free_image_plan.h"
#include <cstdio>
using namespace bh;
static unsigned long long rng_state = 88172645463325252ull;
static unsigned long long rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
int main() {
    std::printf("K %.17g %.17g %.17g %.17g\n", kFreeImageBuildSweeps, kFreeImageMoveLaunchSweeps, kFreeImageMoveColumnSweeps, kFreeImageMinSavedBytes);
    const long long ns[] = {7, 64, 65, 301, 4096}, rowss[] = {64, 65536};
    for (int option = 0; option <= 2; ++option) for (long long n : ns) for (long long rows : rowss) for (int rep = 0; rep < 3; ++rep) {
        std::printf("Q %d %lld %lld\n", option, rows, n);
        const long long nwords = (n + 63) / 64;
        std::vector<uint64_t> want((size_t)nwords, 0ull);
        FreeImageBook b;
        std::vector<int32_t> img;                        // the model image: entry = original column, -1 = zero padding
        long long last_n_hmul = 0;
        for (int call = 0; call < 40; ++call) {
            // the active set of this call: a few variables more (sometimes none, sometimes many), now and then one less
            const int what = (int)(rnd() % 8);
            long long add = what == 0 ? 0 : what == 1 ? (long long)(rnd() % (n / 4 + 1)) : what < 6 ? (long long)(rnd() % 3) : 1;
            if (call == 0) add = n / 8;
            for (long long a = 0; a < add; ++a) { const long long i = (long long)(rnd() % n); want[(size_t)(i >> 6)] |= 1ull << (i & 63); }
            if (what == 7 && call > 3) {
                for (long long i = (long long)(rnd() % n), tries = 0; tries < n; ++tries, i = (i + 1) % n)
                    if (free_image_bit(want.data(), i)) { want[(size_t)(i >> 6)] &= ~(1ull << (i & 63)); break; }
            }
            const long long nfix = free_image_count(want.data(), n);
            const long long n_hmul = 1 + (long long)(rnd() % 30);
            int64_t k_new = 0, k_freed = 0;
            if (b.present) free_image_diff(b, want.data(), &k_new, &k_freed);
            const bool present = b.present;
            const double credit = b.credit;
            const FreeImageAction act = free_image_decide(option, b.present, rows, n, nfix, k_new, k_freed, b.credit, last_n_hmul);
            if (act == FI_BUILD) {
                free_image_book_build(b, want.data(), n);
                img.assign(b.map.begin(), b.map.end());
            } else if (act == FI_MOVE) {
                std::vector<int32_t> ops;
                const long long old_nfree = b.nfree;
                free_image_book_move(b, want.data(), ops);
                const long long k = (long long)ops.size();
                if (old_nfree - k != b.nfree) { std::printf("X width\n"); return 1; }
                for (long long t = 0; t < k; ++t) {      // as free_image_move_kernel: one thread per t, no slot read and written
                    const int32_t x = img[(size_t)(b.nfree + t)];
                    if (ops[(size_t)t] >= 0) {
                        if (ops[(size_t)t] >= b.nfree) { std::printf("X dst\n"); return 1; }
                        img[(size_t)ops[(size_t)t]] = x;
                    }
                    img[(size_t)(b.nfree + t)] = -1;
                }
            } else if (act == FI_FULL && option == 1 && nfix < n && !(b.present && k_freed == 0) && free_image_worthwhile(rows, nfix, last_n_hmul)) {
                b.credit += free_image_saving(n_hmul, nfix, n);
            }
            int ok = 1;
            if (act != FI_FULL) {
                // the image holds exactly the free variables, each once, in the slots the map says; the rest is padding
                std::vector<int> seen((size_t)n, 0);
                if ((long long)img.size() != b.ldf || b.ldf % 16 != 0 || b.nfree != n - nfix) ok = 0;
                for (long long s = 0; ok && s < b.ldf; ++s) {
                    if (img[(size_t)s] != b.map[(size_t)s]) ok = 0;
                    else if (s >= b.nfree) ok = img[(size_t)s] == -1;
                    else if (img[(size_t)s] < 0 || free_image_bit(want.data(), img[(size_t)s]) || seen[(size_t)img[(size_t)s]]++ || b.slot[(size_t)img[(size_t)s]] != s) ok = 0;
                }
                for (long long i = 0; ok && i < n; ++i)
                    if (free_image_bit(want.data(), i) && b.slot[(size_t)i] != -1) ok = 0;
                if (free_image_state(b, want.data()) != FI_STATE_VALID) ok = 0;
            }
            std::printf("C %lld %d %lld %lld %.17g %lld %d %lld | %d %lld %lld %d\n", nfix, present ? 1 : 0, (long long)k_new, (long long)k_freed, credit,
                        last_n_hmul, (int)act, n_hmul, b.present ? 1 : 0, (long long)b.nfree, (long long)b.ldf, ok);
            last_n_hmul = n_hmul;
        }
    }
    return 0;
}
"""

FULL, USE, BUILD, MOVE = 0, 1, 2, 3


@pytest.fixture(scope="module")
def log(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("free_image_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    consts = [float(x) for x in out[0].split()[1:]]
    seqs, cur = [], None
    for line in out[1:]:
        v = line.replace("|", " ").split()
        if v[0] == "Q":
            cur = dict(option=int(v[1]), rows=int(v[2]), n=int(v[3]), calls=[])
            seqs.append(cur)
        else:
            assert v[0] == "C", line
            keys = ("nfix", "present", "k_new", "k_freed", "credit", "last", "action", "n_hmul", "present_after", "nfree", "ldf", "ok")
            cur["calls"].append({k: (float(x) if k == "credit" else int(x)) for k, x in zip(keys, v[1:])})
    assert len(seqs) == 3 * 5 * 2 * 3 and all(len(s["calls"]) == 40 for s in seqs)
    return dict(build=consts[0], launch=consts[1], column=consts[2], min_bytes=consts[3]), seqs


def _worth(K, s, c):
    return 8.0 * s["rows"] * c["nfix"] * max(c["last"], 1) >= K["min_bytes"]


def test_the_sequences_exercise_every_action(log):
    K, seqs = log
    seen = {(s["option"], c["action"]) for s in seqs for c in s["calls"]}
    assert {(1, FULL), (1, USE), (1, BUILD), (1, MOVE), (2, USE), (2, BUILD), (2, MOVE), (0, FULL)} <= seen
    assert any(c["k_freed"] > 0 and c["present"] for s in seqs for c in s["calls"]), "no sequence ever freed a variable under an image"
    assert any(c["action"] == FULL and c["present"] and c["k_new"] > 0 and c["k_freed"] == 0 for s in seqs if s["option"] == 1 for c in s["calls"]), \
        "no call ever declined its moves"


def test_no_build_before_the_credit_reaches_the_cost(log):
    K, seqs = log
    for s in (s for s in seqs if s["option"] == 1):
        credit = 0.0
        for c in s["calls"]:
            assert c["credit"] == credit, (s["option"], s["n"], c)                   # the book carries what the calls earned, nothing else
            if c["action"] == BUILD:
                assert c["credit"] >= K["build"] and _worth(K, s, c) and 0 < c["nfix"] < s["n"], c
                credit = 0.0
            elif c["action"] == FULL and not (c["present"] and c["k_freed"] == 0) and _worth(K, s, c) and 0 < c["nfix"] < s["n"]:
                # ... and a call that could have built does so as soon as the credit is there
                assert c["credit"] < K["build"], c
                credit += c["n_hmul"] * c["nfix"] / s["n"]
        # small problems never build: the sweeps they would save are worth less than the launch the compact loop adds
        if 8.0 * s["rows"] * s["n"] * 30 < K["min_bytes"]:
            assert all(c["action"] == FULL for c in s["calls"])


def test_moves_only_when_they_pay(log):
    K, seqs = log
    for s in seqs:
        for c in s["calls"]:
            cost = K["launch"] + K["column"] * c["k_new"]
            saving = c["last"] * c["nfix"] / s["n"]
            if c["action"] == MOVE:
                assert c["present"] and c["k_freed"] == 0 and c["k_new"] > 0
                assert s["option"] == 2 or (cost <= saving and _worth(K, s, c)), (s["option"], c)
            elif s["option"] == 1 and c["present"] and c["k_freed"] == 0 and c["k_new"] > 0 and _worth(K, s, c) and c["nfix"] < s["n"]:
                assert c["action"] == FULL and cost > saving, c                      # declined: this call streams the full image


def test_a_stale_image_is_never_used(log):
    K, seqs = log
    for s in seqs:
        for c in s["calls"]:
            if c["action"] in (USE, MOVE):
                assert c["present"] and c["k_freed"] == 0, c
            if c["action"] == USE:
                assert c["k_new"] == 0, c
            if c["action"] != FULL:
                # what the loop then streams is exactly the free columns of THIS call's active set
                assert c["ok"] == 1 and c["present_after"] == 1 and c["nfree"] == s["n"] - c["nfix"] and c["nfree"] <= c["ldf"], c
            if c["present"] and c["k_freed"] > 0:
                assert c["action"] in (FULL, BUILD), c                               # it never grows


def test_option_0_never_builds_and_option_2_builds_at_the_first_eligible_call(log):
    K, seqs = log
    for s in seqs:
        if s["option"] == 0:
            assert all(c["action"] == FULL and not c["present_after"] for c in s["calls"])
        if s["option"] == 2:
            first = True
            for c in s["calls"]:
                eligible = 0 < c["nfix"] < s["n"]
                assert (c["action"] != FULL) == eligible, c
                if eligible and first:
                    assert c["action"] == BUILD, c
                    first = False
                if eligible and c["present"] and c["k_freed"] > 0:
                    assert c["action"] == BUILD, c                                   # rebuilt at once


def test_option_is_accepted_and_documented():
    import benlsip_jl_amd as bh
    lib = bh.load()
    try:
        for v in (0, 2, 1):
            assert lib.bh_set_option(b"free_image", v) == 0, lib.bh_last_error_detail()
        assert lib.bh_set_option(b"free_image", 3) == bh._lib.BH_ERR_INVALID_ARG
        assert lib.bh_set_option(b"free_image", -1) == bh._lib.BH_ERR_INVALID_ARG
    finally:
        assert lib.bh_set_option(b"free_image", 1) == 0
    hdr = open(os.path.join(ROOT, "include", "benlsip_hip.h")).read()
    i = hdr.index("int32_t bh_set_option(")
    assert re.search(r'^ \*   "free_image"\s+\[1\]', hdr[hdr.rindex("/*", 0, i):i], flags=re.M)
    assert "bh_hess_free_image_info" in hdr and "bh_hess_free_image_read" in hdr
    assert "free_image" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_library_follows_the_plan():
    """bh_api.hip takes every decision, the map and the moves from the header; the header has no HIP; every constant cites its file."""
    api = open(os.path.join(CSRC, "bh_api.hip")).read()
    assert '#include "bh_free_image_plan.h"' in api
    for name in ("free_image_decide(", "free_image_book_build(", "free_image_book_move(", "free_image_diff(", "free_image_saving("):
        assert name in api, name
    hdr = open(os.path.join(CSRC, "bh_free_image_plan.h")).read()
    assert "hip" not in "".join(ln for ln in hdr.splitlines() if ln.lstrip().startswith("#include"))
    for name in re.findall(r"profiles/(r\d+_[a-z0-9_]+\.(?:txt|csv|json))", hdr):
        assert os.path.exists(os.path.join(ROOT, "profiles", name)), name
