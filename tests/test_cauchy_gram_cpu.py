"""CPU tests of the one-launch Gram-form Cauchy search: the option and the export exist (no compute without a GPU)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cauchy_gram_option_is_accepted():
    import benlsip_jl_amd as bh
    lib = bh.load()
    try:
        assert lib.bh_set_option(b"cauchy_gram", 1) == 0
    finally:
        assert lib.bh_set_option(b"cauchy_gram", 0) == 0


def test_cauchy_info_is_exported_and_declared():
    import benlsip_jl_amd as bh
    lib = bh.load()
    assert hasattr(lib, "bh_cauchy_info")
    assert "bh_cauchy_info" in bh._lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "benlsip_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int32_t\s+bh_cauchy_info\s*\(\s*const\s+bh_proj\s*\*\s*P\s*,\s*int32_t\s*\*\s*form\s*,\s*int32_t\s*\*\s*n_launches\s*\)", hdr)


def test_cauchy_gram_kernel_is_one_workgroup_launch_in_the_search_path():
    """The search kernel exists in its own header, is included in the translation unit, and the host launches it with a grid of one."""
    src = open(os.path.join(ROOT, "benlsip.jl_amd", "csrc", "bh_api.hip")).read()
    assert os.path.exists(os.path.join(ROOT, "benlsip.jl_amd", "csrc", "bh_cauchygram.hip.h"))
    assert '#include "bh_cauchygram.hip.h"' in open(os.path.join(ROOT, "benlsip.jl_amd", "csrc", "bh_kernels.hip.h")).read()
    launches = re.findall(r"hipLaunchKernelGGL\(cauchy_gram_kernel<\w+>, dim3\((\w+)\)", src)
    assert launches and all(g == "1" for g in launches), launches
