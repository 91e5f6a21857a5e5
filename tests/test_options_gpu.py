"""bh_init takes the initial value of an option from the environment (options_from_env, csrc/bh_options.h): that line runs only with a
device.  Each case is a fresh child process — the variables are read once, by the first bh_init of a process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# One box-constrained projected_cg at d = 64, n = 32 with every eighth variable fixed; argv: the expected stats.cg_kernels, the expected
# state of the compact image, then key=value pairs for set_option.
CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import benlsip_jl_amd as bh
import benlsip_ref as R
want_kernels, want_image = int(sys.argv[1]), sys.argv[2]
bh.init(0)
for kv in sys.argv[3:]:
    bh.set_option(kv.split("=")[0], int(kv.split("=")[1]))
d, n = 64, 32
J = R.synthetic_J(d, n, seed=1)
inst = R.synthetic_box_vectors(d, n, fix_every=8)
assert int(np.count_nonzero(inst.fixvars)) == n // 8
A = np.zeros((0, n))
cons_o = R.make_mixed_constraints(A, R.chol_lower(A @ A.T), inst.fixvars, l=inst.x_l, u=inst.x_u)
g = J.T @ inst.r0
w_l, w_u = R.build_step_bounds(inst.x, cons_o, 0.1 * np.linalg.norm(g))
H = bh.AlHessian(J, None, 10.0)
cons = bh.MixedConstraints(A, None, inst.fixvars, l=inst.x_l, u=inst.x_u)
w, status, info = bh.projected_cg(g, H, w_l, w_u, cons, 0.1, full_output=True)
kernels, image = H.stats()["cg_kernels"], H.free_image_info(cons)
print("cg_kernels", kernels, "image", image, "status", int(status), "iters", info["iters"], flush=True)
assert info["iters"] >= 1 and not w[inst.fixvars].any()
assert kernels == want_kernels, (kernels, want_kernels)
assert image["state"] == want_image and (image["builds"] > 0) == (want_image != "none"), image
H.close()
cons.close()
""" % (ROOT, os.path.join(ROOT, "oracle"))

NAMES = ("BH_HOST_COPY_KERNELS", "BH_BLOCKS_PER_CU", "BH_PCG_BATCH", "BH_PROJ_FORM", "BH_CG_FUSED", "BH_FINAL_SYNC", "BH_FREE_IMAGE",
         "BH_FREE_IMAGE_EQ", "BH_CAUCHY_BLOCK")


def _child(env_add, *args):
    env = {k: v for k, v in os.environ.items() if k not in NAMES}
    env.update(env_add)
    r = subprocess.run([sys.executable, "-c", CHILD] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    return r.stdout


def test_bh_init_reads_the_environment_rows_of_the_option_table():
    # BH_CG_FUSED=0: the separate-kernel shape (stats.cg_kernels == 0); BH_FREE_IMAGE=0: no compact image
    _child({"BH_CG_FUSED": "0", "BH_FREE_IMAGE": "0"}, 0, "none")
    # nothing set, free_image = 2 through bh_set_option: the two-kernel iteration on an image built at this first eligible call
    _child({}, 2, "valid", "free_image=2")
