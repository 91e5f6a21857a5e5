"""CPU tests of the fused Gram-form CG iteration: the option is documented and declared where the library dispatches it, and
switching it on without a device fails like every other product-path call (no compute without a GPU)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_documents_gram_cg_fused():
    hdr = open(os.path.join(ROOT, "include", "benlsip_hip.h")).read()
    i = hdr.index("int32_t bh_set_option(")
    options = hdr[hdr.rindex("/*", 0, i):i]
    assert re.search(r'^ \*   "gram_cg_fused"\s+\[0\]', options, flags=re.M)
    # ... and next to the Gram-form paragraph, with what stats.cg_kernels reports for such a handle
    j = hdr.index("int32_t bh_hess_set_form(")
    assert '"gram_cg_fused"' in hdr[hdr.rindex("/*", 0, j):j]
    k = hdr.index("int64_t cg_kernels;")
    assert "gram_cg_fused" in hdr[hdr.rindex("/*", 0, k):k]


def test_gram_cg_fused_needs_an_initialised_device():
    import benlsip_jl_amd as bh
    lib = bh.load()
    if lib.bh_synchronize() == -2:                      # BH_ERR_NOT_INIT: no bh_init in this process (always the case without a GPU)
        assert lib.bh_set_option(b"gram_cg_fused", 1) == -2 and b"bh_init" in lib.bh_last_error_detail()
        import torch
        if not torch.cuda.is_available():
            with pytest.raises(bh.BenlsipHipError):
                bh.set_option("gram_cg_fused", 1)
    else:
        try:
            bh.set_option("gram_cg_fused", 1)
        finally:
            bh.set_option("gram_cg_fused", 0)
    assert lib.bh_set_option(b"gram_cg_fused", 0) == 0                  # switching it off never needs a device
    assert lib.bh_set_option(b"gram_cg_fused", 2) != 0


def test_gram_cg_kernel_is_dispatched_for_every_geometry_from_a_function_of_its_own():
    api = open(os.path.join(ROOT, "benlsip.jl_amd", "csrc", "bh_api.hip")).read()
    assert '#include "bh_gramcg.hip.h"' in open(os.path.join(ROOT, "benlsip.jl_amd", "csrc", "bh_kernels.hip.h")).read()
    # launch_gram_cg goes through the one geometry dispatcher and launches both prologue variants in the geometry it is handed;
    # gram_cg_kernel is launched nowhere else
    m = re.search(r"void\s+launch_gram_cg\s*\(\s*int\s+cfg\s*,[^{]*\{(.*?)\n\}", api, flags=re.S)
    assert m, "launch_gram_cg not found"
    body = m.group(1)
    assert "with_rs_geom(cfg," in body and "using G = decltype(geom);" in body
    inst = re.findall(r"gram_cg_kernel<G::T, G::CPT, G::R, (\d)>\), dim3\(grid\), dim3\(G::T\), 0, s, a\)", body)
    assert inst == ["1", "0"]
    assert api.count("gram_cg_kernel<") == 2
    # with_rs_geom hands out every entry of the geometry list
    geoms = re.search(r"using\s+RsGeoms\s*=\s*std::tuple<(.*?)\n\s*>;", api, flags=re.S).group(1)
    n = len(re.findall(r"RsGeom<\s*\d+\s*,\s*\d+\s*,\s*\d+\s*,\s*\d+\s*>", geoms))
    assert n == 7 and len(re.findall(r"f\(std::tuple_element_t<\d+, RsGeoms>\{\}\)", api)) == n
