"""Option free_image_eq on the CPU: the decision rule (csrc/bh_pcg_plan.h: pcg_select) over the whole cross product of its inputs and
the stamp rule of the compact lineq image Af (csrc/bh_free_image_plan.h: free_image_af_valid), both built into stand-alone programs
by the host compiler alone (address and undefined-behaviour sanitizers on), as tests/test_pcg_plan_cpu.py builds the selection rule.

* Option off: free_image_eligible is today's expression for every input, and the new input changes no other field of the selection
  whatever its value.
* Option on: exactly the rule of DESIGN.md §4 — today's box rule, or: the three-kernel shape (cg_fused = 1, reduced form, 1 <= mA <= 64,
  W and tpart present, the lineq image with the handle's leading dimension, a register-resident geometry, something to iterate on, g
  padded), one rank, the implicit form, atol_f2b > 0, the call not handed back, and no H*w wanted — whatever hw_free_part_ok says."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")

MA = (0, 1, 2, 64, 65)
CG_FUSED = (0, 1, 2)
BITS = ("gram", "gram_cg_fused", "linv_refine", "fold_init", "comm", "peer_path", "reduced", "tpart", "W", "M_valid", "lda_is_ld",
        "rs_cfg_ok", "cgp3_ok", "peer_blocks_fit", "iterates", "g_padded", "vectors_in_regs", "hw_wanted", "atol_f2b_positive",
        "allow_free_image", "hw_free_part_ok", "free_image_eq")
NB = len(BITS)

# One byte per input: bit 0 free_image_eligible, bit 1 shape == PCG_FUSED, bit 2 gen_linv, bit 3 "every field but free_image_eligible
# equals the selection of the same input with the option off", bit 4 "free_image_eligible with the option off equals today's
# expression", written out next to pcg_select as the parent commit had it.
PROGRAM = r"""
#include "bh_pcg_plan.h"
#include <cstdio>
#include <vector>
int main() {
    const long long mAs[] = {0, 1, 2, 64, 65};
    std::vector<unsigned char> out;
    out.reserve(15u << %(nb)d);
    for (long long mA : mAs) for (long long cg_fused = 0; cg_fused < 3; ++cg_fused) for (unsigned b = 0; b < (1u << %(nb)d); ++b) {
        auto bit = [&](int i) { return ((b >> i) & 1u) != 0; };
        bh::PcgSelectIn in{};
        in.mA = mA; in.cg_fused = cg_fused;
        in.gram_handle = bit(0); in.gram_cg_fused = bit(1); in.linv_refine = bit(2); in.fold_init = bit(3);
        in.comm = bit(4); in.peer_path = bit(5); in.reduced = bit(6); in.tpart = bit(7); in.W = bit(8); in.M_valid = bit(9);
        in.lda_is_ld = bit(10); in.rs_cfg_ok = bit(11); in.cgp3_ok = bit(12); in.peer_blocks_fit = bit(13); in.iterates = bit(14);
        in.g_padded = bit(15); in.vectors_in_regs = bit(16); in.hw_wanted = bit(17); in.atol_f2b_positive = bit(18);
        in.allow_free_image = bit(19); in.hw_free_part_ok = bit(20); in.free_image_eq = bit(21) ? 1 : 0;
        const bh::PcgSelection s = bh::pcg_select(in);
        bh::PcgSelectIn off = in;
        off.free_image_eq = 0;
        const bh::PcgSelection t = bh::pcg_select(off);
        const bool rest = s.shape == t.shape && s.fuse_gen == t.fuse_gen && s.gen_linv == t.gen_linv && s.linv_refine == t.linv_refine &&
                          s.peer_fused == t.peer_fused && s.rccl_gen == t.rccl_gen && s.fold_init == t.fold_init && s.cg_kernels == t.cg_kernels;
        const bool today = t.shape == bh::PCG_FUSED && in.allow_free_image && mA == 0 && !in.gram_handle && !in.comm &&
                           (!in.hw_wanted || in.hw_free_part_ok) && in.atol_f2b_positive;
        out.push_back((unsigned char)(s.free_image_eligible | (s.shape == bh::PCG_FUSED) << 1 | s.gen_linv << 2 | rest << 3 |
                                      (t.free_image_eligible == today) << 4));
    }
    return std::fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 1;
}
""" % {"nb": NB}

# The stamp rule as plain values: (af_epoch, fi_epoch, mask_epoch) -> serves?
STAMPS = [((0, 0, 0), False),          # nothing anywhere
          ((0, 5, 5), False),          # Jf describes the caller's set, no Af yet
          ((5, 5, 5), True),           # formed for exactly this pair of constraint handle and active set
          ((4, 5, 5), False),          # Jf moved on (a move, a rebuild, another constraint handle): rebuild
          ((5, 5, 6), False),          # the caller's set is another than Jf's (the driver moves or rebuilds Jf first)
          ((5, 0, 5), False),          # Jf released
          ((6, 5, 6), False),
          ((2 ** 40 + 1, 2 ** 40 + 1, 2 ** 40 + 1), True)]
STAMP_PROGRAM = r"""
#include "bh_free_image_plan.h"
#include <cstdio>
int main() {
    unsigned long long a, f, m;
    while (std::scanf("%llu %llu %llu", &a, &f, &m) == 3) std::printf("%d\n", bh::free_image_af_valid(a, f, m) ? 1 : 0);
    return 0;
}
"""


def _build(tmp_path_factory, name, program):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp(name)
    src, exe = d / (name + ".cpp"), d / name
    src.write_text(program)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.fixture(scope="module")
def selections(tmp_path_factory):
    raw = subprocess.run([_build(tmp_path_factory, "select_eq", PROGRAM)], check=True, capture_output=True).stdout
    out = np.frombuffer(raw, dtype=np.uint8)
    assert out.size == len(MA) * len(CG_FUSED) << NB
    return out.reshape(len(MA), len(CG_FUSED), 1 << NB)


def expected_eligible(mA, cg_fused, v):
    """By DESIGN.md §4 and the option's description in include/benlsip_hip.h, as a case tree of its own."""
    one_rank, implicit = ~v["comm"], ~v["gram"]
    streams = v["rs_cfg_ok"] & v["iterates"] & v["g_padded"]
    common = one_rank & implicit & v["atol_f2b_positive"] & v["allow_free_image"]
    if mA == 0:
        # the box rule: the two-kernel iteration, no H*w wanted or only its free part — the new option does not enter
        return common & (cg_fused != 0) & streams & (~v["hw_wanted"] | v["hw_free_part_ok"])
    if mA > 64 or cg_fused != 1:
        return np.zeros_like(common)                             # the four- and the seven-kernel shape, mA > 64: never
    three_kernel = v["reduced"] & v["tpart"] & v["W"] & v["lda_is_ld"] & streams
    return common & v["free_image_eq"] & three_kernel & ~v["hw_wanted"]


def test_the_rule_of_the_option_over_all_inputs(selections):
    b = np.arange(1 << NB, dtype=np.uint32)
    v = {name: ((b >> i) & 1).astype(bool) for i, name in enumerate(BITS)}
    seen_eq = 0
    for i, mA in enumerate(MA):
        for j, cg_fused in enumerate(CG_FUSED):
            got = selections[i, j]
            assert np.all(got & 8), (mA, cg_fused, "the option changes another field of the selection")
            assert np.all(got & 16), (mA, cg_fused, "option off: free_image_eligible is not today's expression")
            eligible, fused, three = (got & 1).astype(bool), (got & 2).astype(bool), (got & 4).astype(bool)
            want = expected_eligible(mA, cg_fused, v)
            bad = np.flatnonzero(eligible != want)
            assert bad.size == 0, (mA, cg_fused, {n: int(v[n][bad[0]]) for n in BITS}, bool(eligible[bad[0]]), bool(want[bad[0]]))
            assert not np.any(eligible & ~fused)
            if mA > 0:
                assert not np.any(eligible & ~three) and not np.any(eligible & ~v["free_image_eq"]) and not np.any(eligible & v["hw_wanted"])
                seen_eq += int(np.count_nonzero(eligible))
            else:
                # box constraints: the option is not looked at
                off = eligible[~v["free_image_eq"]]
                assert np.array_equal(off, eligible[v["free_image_eq"]])
    assert seen_eq > 0


def test_the_stamp_rule_of_the_compact_lineq_image(tmp_path_factory):
    exe = _build(tmp_path_factory, "stamp", STAMP_PROGRAM)
    text = "".join("%d %d %d\n" % s for s, _ in STAMPS)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
    assert [x == "1" for x in out] == [w for _, w in STAMPS], out


def test_the_library_follows_the_rule_and_the_stamp():
    """bh_api.hip hands the option to pcg_select, asks free_image_af_valid before it reuses Af, stamps Af with the epoch of Jf, releases
    it wherever Jf is released, and reads BH_FREE_IMAGE_EQ where it reads BH_FREE_IMAGE."""
    api = open(os.path.join(CSRC, "bh_api.hip")).read()
    assert "in.free_image_eq = g_ctx.opt_free_image_eq;" in api
    assert "free_image_af_valid(H->af_epoch, H->fi_epoch, P->mask_epoch)" in api and "H->af_epoch = H->fi_epoch;" in api
    release = api[api.index("static void free_image_release(bh_hess* H) {"):]
    release = release[:release.index("\n}\n")]
    assert "dev_free(H->Af)" in release and "H->af_epoch = 0" in release
    # both variables are environment rows of the option table, which bh_init reads (what each does: tests/test_options_cpu.py)
    options = re.sub(r"\s+", " ", open(os.path.join(CSRC, "bh_options.h")).read())
    assert re.search(r'\{"free_image", &Options::opt_free_image, [^{}]*"BH_FREE_IMAGE", OPT_\w+\}', options)
    assert re.search(r'\{"free_image_eq", &Options::opt_free_image_eq, [^{}]*"BH_FREE_IMAGE_EQ", OPT_\w+\}', options)
    init = api[api.index("int32_t bh_init(int32_t device, int32_t flags) {"):api.index("int32_t bh_shutdown(void) {")]
    assert "options_from_env(g_ctx, getenv, kMaxBlocksPerCu);" in init
    hdr = open(os.path.join(CSRC, "bh_pcg_plan.h")).read()
    fields = hdr[hdr.index("struct PcgSelectIn {"):hdr.index("struct PcgSelection {")]
    assert fields.rstrip().rstrip("};").rstrip().splitlines()[-1].lstrip().startswith("int64_t free_image_eq;")     # appended at the end
