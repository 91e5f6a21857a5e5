"""CPU tests of the Gram build that runs during the asynchronous upload of J (option gram_ingest): the schedule
(csrc/bh_gram_ingest_plan.h, no HIP in it) built into a stand-alone program by the host compiler, with the address and undefined-
behaviour sanitizers, and checked over a sweep of leading dimensions and chunk widths; the option is accepted and documented."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")

LD = (16, 64, 80, 208, 304, 1472, 4096, 16384)
CHUNK_COLS = (32, 96, 128, 160, 4096)
NROWS = (1, 705, 65536)                  # one slab; slabs capped by the 256-row minimum; slabs set by the CU count
N_CU = 256

# One line per (ld, chunk_cols, nrows): "P ld cc nchunks nrows nb part_doubles", then one line per chunk:
# "S k row_lo row_hi block_lo nblocks nslabs slab_rows part_doubles".  n = ld - 3 (> ld - 16): the last chunk also writes padding.
PROGRAM = r"""
#include "bh_gram_ingest_plan.h"
#include <cstdio>
int main() {
    const long long lds[] = {16, 64, 80, 208, 304, 1472, 4096, 16384}, ccs[] = {32, 96, 128, 160, 4096}, rows[] = {1, 705, 65536};
    for (long long ld : lds) for (long long cc0 : ccs) for (long long nrows : rows) {
        const long long n = ld - 3;
        const long long cc = cc0 < (n + 31) / 32 * 32 ? cc0 : (n + 31) / 32 * 32;      // as bh_hess_create_async clamps it
        const long long nchunks = (n + cc - 1) / cc;
        const bh::GramIngestPlan p = bh::gram_ingest_plan(ld, cc, nchunks, nrows, 256);
        std::printf("P %lld %lld %lld %lld %lld %lld\n", ld, cc, nchunks, nrows, (long long)p.nb, (long long)p.part_doubles);
        for (long long k = 0; k < nchunks; ++k) {
            const bh::GramIngestStep s = bh::gram_ingest_step(p, k);
            std::printf("S %lld %lld %lld %lld %lld %lld %lld %lld\n", k, (long long)s.row_lo, (long long)s.row_hi, (long long)s.block_lo,
                        (long long)s.nblocks, (long long)s.nslabs, (long long)s.slab_rows, (long long)s.part_doubles);
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("gram_ingest_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    plans, cur = [], None
    for line in out:
        tag, *v = line.split()
        v = [int(x) for x in v]
        if tag == "P":
            cur = dict(zip(("ld", "cc", "nchunks", "nrows", "nb", "part"), v), steps=[])
            plans.append(cur)
        else:
            cur["steps"].append(dict(zip(("k", "lo", "hi", "block_lo", "nblocks", "nslabs", "slab_rows", "part"), v)))
    assert len(plans) == len(LD) * len(CHUNK_COLS) * len(NROWS)
    assert {(p["ld"], p["nrows"]) for p in plans} == {(ld, r) for ld in LD for r in NROWS}
    return plans


def test_block_rows_are_partitioned_and_never_early(plans):
    for p in plans:
        ld, cc, nchunks, nb = p["ld"], p["cc"], p["nchunks"], p["nb"]
        n = ld - 3
        assert nb == -(-ld // 64) and len(p["steps"]) == nchunks
        nxt = 0
        for s in p["steps"]:
            k = s["k"]
            assert s["lo"] == nxt <= s["hi"], (p, s)                   # contiguous, in order: a partition of [0, nb)
            nxt = s["hi"]
            # columns in the image once chunk k is transposed: the last chunk writes everything up to ld
            landed = ld if k == nchunks - 1 else min((k + 1) * cc, n)
            for b in range(s["lo"], s["hi"]):
                assert min((b + 1) * 64, ld) <= landed, ("block row scheduled before its last column", p["ld"], cc, k, b)
            # ... and not later than necessary: the next block row is still incomplete
            if s["hi"] < nb:
                assert min((s["hi"] + 1) * 64, ld) > landed, ("a complete block row was left waiting", p["ld"], cc, k)
            # the packed lower blocks of these rows: every block exactly once
            assert s["block_lo"] == s["lo"] * (s["lo"] + 1) // 2
            assert s["nblocks"] == sum(b + 1 for b in range(s["lo"], s["hi"]))
        assert nxt == nb, "the last chunk schedules everything left"
        assert sum(s["nblocks"] for s in p["steps"]) == nb * (nb + 1) // 2


def test_step_geometry(plans):
    for p in plans:
        nrows = p["nrows"]
        for s in p["steps"]:
            assert s["nslabs"] >= 1 and s["slab_rows"] >= 1 and s["slab_rows"] % 16 == 0
            if s["nblocks"] == 0:
                assert s["part"] == 0
                continue
            # the slabs cover the rows and none is empty; their number is at most ceil(nrows / 256) (the one-shot build's rule), so
            # one of several has more than 128 rows
            assert s["nslabs"] * s["slab_rows"] >= nrows > (s["nslabs"] - 1) * s["slab_rows"]
            assert s["nslabs"] <= max(1, -(-nrows // 256))
            if s["nslabs"] > 1:
                assert s["slab_rows"] > 128
                assert s["nblocks"] < N_CU                              # blocks that outnumber the CUs take one slab
                # about two workgroups per CU, no more than one slab above it
                assert s["nblocks"] * (s["nslabs"] - 1) < 2 * N_CU
                assert s["part"] == s["nslabs"] * s["nblocks"] * 64 * 64
            else:
                assert s["part"] == 0
            assert s["part"] <= p["part"], "the compact buffer covers every step"
        assert p["part"] == max([s["part"] for s in p["steps"]], default=0)
        assert p["part"] < 3 * N_CU * 64 * 64                            # compact: slabs x blocks x 64 x 64, never slabs x ld x ld


def test_documented_examples(plans):
    """The shapes DESIGN.md and the header comment speak of."""
    by = {(p["ld"], p["cc"], p["nrows"]): p for p in plans}
    p = by[(4096, 128, 65536)]                                           # config 3 with 64 MiB chunks: two block rows per chunk
    assert p["nchunks"] == 32
    assert [s["nblocks"] for s in p["steps"]] == [4 * k + 3 for k in range(32)]
    p = by[(4096, 32, 65536)]                                            # half a block per chunk: every second chunk completes a row
    assert [s["hi"] - s["lo"] for s in p["steps"]][:6] == [0, 1, 0, 1, 0, 1]
    p = by[(304, 160, 705)]                                              # chunks that straddle blocks; n = 301: the last block is partial
    assert [(s["lo"], s["hi"]) for s in p["steps"]] == [(0, 2), (2, 5)]
    p = by[(80, 96, 705)]                                                # one chunk: everything at once
    assert [(s["lo"], s["hi"]) for s in p["steps"]] == [(0, 2)]


def test_option_is_accepted_and_documented():
    import benlsip_jl_amd as bh
    lib = bh.load()
    try:
        assert lib.bh_set_option(b"gram_ingest", 1) == 0, lib.bh_last_error_detail()
        assert lib.bh_set_option(b"gram_ingest", 2) == bh._lib.BH_ERR_INVALID_ARG
        assert lib.bh_set_option(b"gram_ingest", -1) == bh._lib.BH_ERR_INVALID_ARG
    finally:
        assert lib.bh_set_option(b"gram_ingest", 0) == 0
    hdr = open(os.path.join(ROOT, "include", "benlsip_hip.h")).read()
    i = hdr.index("int32_t bh_set_option(")
    assert re.search(r'^ \*   "gram_ingest"\s+\[0\]', hdr[hdr.rindex("/*", 0, i):i], flags=re.M)
    j = hdr.index("int32_t bh_hess_create_async(")
    assert '"gram_ingest"' in hdr[hdr.rindex("/*", 0, j):j]
    assert "gram_ingest" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_library_follows_the_schedule():
    """bh_api.hip includes the header and takes every step and the size of the compact buffer from it; the header has no HIP."""
    api = open(os.path.join(CSRC, "bh_api.hip")).read()
    assert '#include "bh_gram_ingest_plan.h"' in api and "gram_ingest_step(u.gram_plan, k)" in api and "u->gram_plan.part_doubles" in api
    hdr = open(os.path.join(CSRC, "bh_gram_ingest_plan.h")).read()
    assert "hip" not in "".join(ln for ln in hdr.splitlines() if ln.lstrip().startswith("#include"))
