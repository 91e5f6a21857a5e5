"""CPU tests of the Cauchy search with linear equalities on a Gram-form handle (option cauchy_gram_eq): the option exists and checks its
value, the header documents it, the kernel's header is part of the translation unit (no compute without a GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cauchy_gram_eq_option_is_accepted_and_checked():
    import benlsip_jl_amd as bh
    lib = bh.load()
    try:
        assert lib.bh_set_option(b"cauchy_gram_eq", 1) == 0
        assert lib.bh_set_option(b"cauchy_gram_eq", 2) != 0
        assert lib.bh_set_option(b"cauchy_gram_eq", -1) != 0
    finally:
        assert lib.bh_set_option(b"cauchy_gram_eq", 0) == 0


def test_header_documents_the_option_and_form_4():
    hdr = open(os.path.join(ROOT, "include", "benlsip_hip.h")).read()
    assert re.search(r'"cauchy_gram_eq"\s*\[0\]', hdr)
    info = hdr[hdr.index("Form and launch count of the last bh_cauchy_step"):hdr.index("int32_t bh_cauchy_info(")]
    assert re.search(r"form 4 = from G with linear equalities", info)
    form_doc = hdr[:hdr.index("#define BH_HESS_IMPLICIT")]
    assert '"cauchy_gram_eq" = 1' in form_doc and "form 4" in form_doc


def test_kernel_header_is_part_of_the_translation_unit_and_the_interval_is_named():
    csrc = os.path.join(ROOT, "benlsip.jl_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "bh_cauchygrameq.hip.h"))
    assert '#include "bh_cauchygrameq.hip.h"' in open(os.path.join(csrc, "bh_kernels.hip.h")).read()
    src = open(os.path.join(csrc, "bh_api.hip")).read()
    m = re.search(r"constexpr int kCauchyGramEqRefresh = (\d+);", src)
    assert m and int(m.group(1)) >= 2 and (int(m.group(1)) & (int(m.group(1)) - 1)) == 0        # a power of two
    assert re.search(r"hipLaunchKernelGGL\(cauchy_gram_eq_kernel, dim3\(rblocks \+ dblocks \+ mA\)", src)
