"""The rule that picks the iteration shape of a projected_cg call (csrc/bh_pcg_plan.h: pcg_select, no HIP in it) against the rule as
the option descriptions of include/benlsip_hip.h (cg_fused, gram_cg_fused, linv_refine, fold_init, free_image, stats.cg_kernels) and
DESIGN.md §4 / §7 state it: a stand-alone program built by the host compiler (address and undefined-behaviour sanitizers on) packs
the selection over the whole cross product of its inputs into 16-bit words; every word is compared with `expected` below, which
is written from the documents as a case tree, not from the C++."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")

MA = (0, 1, 2, 64, 65)                   # box | one equality (no refinement) | refinement from two on | the last fused count | past it
CG_FUSED = (0, 1, 2)
BITS = ("gram", "gram_cg_fused", "linv_refine", "fold_init", "comm", "peer_path", "reduced", "tpart", "W", "M_valid", "lda_is_ld",
        "rs_cfg_ok", "cgp3_ok", "peer_blocks_fit", "iterates", "g_padded", "vectors_in_regs", "hw_wanted", "atol_f2b_positive",
        "allow_free_image")
SEPARATE, FUSED, RCCL_BOX = 0, 1, 2

PROGRAM = r"""
#include "bh_pcg_plan.h"
#include <cstdio>
#include <vector>
int main() {
    const long long mAs[] = {0, 1, 2, 64, 65};
    std::vector<unsigned short> out;
    out.reserve(15u << 20);
    for (long long mA : mAs) for (long long cg_fused = 0; cg_fused < 3; ++cg_fused) for (unsigned b = 0; b < (1u << 20); ++b) {
        auto bit = [&](int i) { return ((b >> i) & 1u) != 0; };
        bh::PcgSelectIn in{};
        in.mA = mA; in.cg_fused = cg_fused;
        in.gram_handle = bit(0); in.gram_cg_fused = bit(1); in.linv_refine = bit(2); in.fold_init = bit(3);
        in.comm = bit(4); in.peer_path = bit(5); in.reduced = bit(6); in.tpart = bit(7); in.W = bit(8); in.M_valid = bit(9);
        in.lda_is_ld = bit(10); in.rs_cfg_ok = bit(11); in.cgp3_ok = bit(12); in.peer_blocks_fit = bit(13); in.iterates = bit(14);
        in.g_padded = bit(15); in.vectors_in_regs = bit(16); in.hw_wanted = bit(17); in.atol_f2b_positive = bit(18);
        in.allow_free_image = bit(19);
        const bh::PcgSelection s = bh::pcg_select(in);
        out.push_back((unsigned short)((int)s.shape | s.fuse_gen << 2 | s.gen_linv << 3 | s.linv_refine << 4 | s.peer_fused << 5 |
                                       s.rccl_gen << 6 | s.free_image_eligible << 7 | s.fold_init << 8 | s.cg_kernels << 9));
    }
    return std::fwrite(out.data(), sizeof(unsigned short), out.size(), stdout) == out.size() ? 0 : 1;
}
"""


def expected(mA, cg_fused, v):
    """The packed selection for one (mA, cg_fused) over all 2^20 settings of the flags `v` (name -> bool array).

    By the documents.  "cg_fused" = 1: box constraints in two kernels (one rank; over the peer buffers, the exchange inside the update
    kernel; over RCCL two kernels + the collective, the update in the prologue of the next H*p — the CGP = 3 variant of a
    register-resident geometry), linear equalities (reduced form, mA <= 64) in three kernels through the explicit inverse of the
    factor; 2: equalities in four kernels, box as 1; 0: the separate-kernel shapes.  A handle in the Gram form ignores "cg_fused": with
    "gram_cg_fused" on (one rank) two kernels with box constraints, three with up to 64 equalities in the reduced form, else the
    separate shape.  stats.cg_kernels: 2 / 3 / 4, one more with equalities over RCCL, 0 in the separate shapes.  Every fused shape
    needs J's rows register-resident (n <= 16384), something free (max_iter >= 1) and g readable to the padded length; with
    equalities also the buffers the kernels work on (partials of A_free r; the image of A with the handle's leading dimension;
    the explicit inverse for three kernels, and on a Gram handle always).  "linv_refine": the three-kernel iteration, from two
    equalities on, with a valid Gram matrix of A_free.  "free_image": box, one rank, implicit form, the two-kernel iteration, no H*w
    wanted (bh_minor_iterate), atol_f2b > 0; a call the compact loop handed back is not considered again.  "fold_init": box
    constraints in the separate-kernel shape, register-resident vectors."""
    one_rank = ~v["comm"]
    peers = v["comm"] & v["peer_path"]
    rccl = v["comm"] & ~v["peer_path"]
    # the option that governs the handle
    level = np.where(v["gram"], np.where(v["gram_cg_fused"] & one_rank, 1, 0), cg_fused)
    streams = v["rs_cfg_ok"] & v["iterates"] & v["g_padded"]
    transport = one_rank | (peers & v["peer_blocks_fit"])          # the fused kernels carry the exchange themselves, or need none
    zero = np.zeros_like(level)
    shape, kernels = zero.copy(), zero.copy()
    if mA == 0:
        fused = (level != 0) & streams & transport
        rccl_box = (level != 0) & streams & rccl & v["cgp3_ok"] & ~v["gram"]
        shape = np.where(fused, FUSED, np.where(rccl_box, RCCL_BOX, SEPARATE))
        kernels = np.where(fused | rccl_box, 2, 0)
        three = four = rccl_eq = np.zeros_like(fused)
    else:
        buffers = v["reduced"] & v["tpart"] & v["lda_is_ld"] & (mA <= 64)
        three = (level == 1) & buffers & v["W"]
        four = (level >= 1) & buffers & ~three & ~(v["gram"] & ~v["W"])
        fused = (three | four) & streams & (transport | rccl)
        three, four = three & fused, four & fused
        rccl_eq = fused & rccl
        shape = np.where(fused, FUSED, SEPARATE)
        kernels = np.where(three, 3, np.where(four, 4, 0)) + rccl_eq
    is_fused = shape == FUSED
    refine = three & v["linv_refine"] & v["M_valid"] & (mA >= 2)
    free_image = is_fused & (mA == 0) & one_rank & ~v["gram"] & ~v["hw_wanted"] & v["atol_f2b_positive"] & v["allow_free_image"]
    fold = (shape == SEPARATE) & (mA == 0) & v["fold_init"] & streams & v["vectors_in_regs"]
    return (shape | (is_fused & (mA > 0)) << 2 | three << 3 | refine << 4 | (is_fused & peers) << 5 | rccl_eq << 6 | free_image << 7 |
            fold << 8 | kernels << 9).astype(np.uint16)


@pytest.fixture(scope="module")
def selections(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("pcg_plan")
    src, exe = d / "select.cpp", d / "select"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    raw = subprocess.run([str(exe)], check=True, capture_output=True).stdout
    out = np.frombuffer(raw, dtype=np.uint16)
    assert out.size == len(MA) * len(CG_FUSED) << 20
    return out.reshape(len(MA), len(CG_FUSED), 1 << 20)


def test_selection_rule_matches_the_documented_rule(selections):
    b = np.arange(1 << 20, dtype=np.uint32)
    v = {name: ((b >> i) & 1).astype(bool) for i, name in enumerate(BITS)}
    shapes, kernels = set(), set()
    for i, mA in enumerate(MA):
        for j, cg_fused in enumerate(CG_FUSED):
            got, want = selections[i, j], expected(mA, cg_fused, v)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (mA, cg_fused, {n: int(v[n][bad[0]]) for n in BITS}, int(got[bad[0]]), int(want[bad[0]]))
            shapes |= set(np.unique(got & 3).tolist())
            kernels |= set(np.unique(got >> 9).tolist())
    assert shapes == {SEPARATE, FUSED, RCCL_BOX}
    assert kernels == {0, 2, 3, 4, 5}


def test_library_takes_the_shape_from_the_rule():
    """bh_api.hip includes both plain headers, fills the plan from pcg_select and schedules both drivers with launch_ahead; neither
    header includes anything of HIP."""
    api = open(os.path.join(CSRC, "bh_api.hip")).read()
    assert '#include "bh_pcg_plan.h"' in api and '#include "bh_launch_ahead.h"' in api
    assert "p.sel = pcg_select(in);" in api and "H->stats.cg_kernels = sel.cg_kernels;" in api
    assert api.count("launch_ahead(") == 2                          # pcg_run and cauchy_impl
    assert "struct MirrorWord" not in api
    for name in ("bh_pcg_plan.h", "bh_launch_ahead.h"):
        hdr = open(os.path.join(CSRC, name)).read()
        includes = [ln for ln in hdr.splitlines() if ln.lstrip().startswith("#include")]
        assert includes and all("hip" not in ln and '"' not in ln for ln in includes), includes
