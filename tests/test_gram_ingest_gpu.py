"""GPU tests of option gram_ingest: bh_hess_create_async builds G = J'J + mu C'C during the upload of J (panel steps behind the
transposes, csrc/bh_gram_ingest_plan.h, gn_gram_panel_kernel), so the handle is in the Gram form with a valid G when bh_hess_wait
returns.  G is read through bh_hmul on unit vectors (the columns of G; a product with one non-zero is exact).

Exact instances: small integer J, C and mu a power of two — every entry of G is an integer below 2^53, independent of the
summation order — against numpy's integer result, bit for bit.  Rounded instances: against a handle made by bh_hess_create +
bh_hess_set_form.  A panel step partitions the rows by the one-shot build's rule applied to the blocks of the step; where both end
at the same slab boundaries (BIT_EQUAL below) the two G are bit-equal, elsewhere every entry lies within
2 gamma_k (|J|' W |J|)_ij, gamma_k = k u / (1 - k u), k = d + q, u = 2^-53: either build sums k products in some order with one
rounding per addition (fused multiply-adds; mu = 1/2 scales exactly), so each is within gamma_k of the exact entry."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")

# (d, n, q, upload_chunk_mb)
SHAPES = [
    (4099, 200, 0, 1),     # 32-column chunks, half a block each, odd d
    (700, 300, 5, 1),      # 160-column chunks straddling blocks, C rows, ld = 304
    (300, 70, 0, 64),      # one chunk, two block rows, the second partial
    (64, 64, 0, 64),       # one block
    (2048, 1472, 3, 1),    # 23 block rows of 64-column chunks, 276 lower blocks > 256 CUs: the one-shot build uses a single slab
    (0, 48, 4, 64),        # no rows: G from C alone, through the ordinary lazy build
]
# Slab boundaries of the ingest steps against the one-shot build's (256 CUs).  Up to 15 lower blocks in all: both take
# min(ceil(512 / blocks), ceil((d + q) / 256)) slabs, and the second term is the smaller one for the step and for the whole matrix
# alike (17, 3, 2, 1 slabs): same boundaries, bit-equal.  (2048, 1472, 3): the one-shot build has 276 blocks >= 256 and takes one slab,
# a step has at most 23 blocks and takes 9 slabs of 240 rows: rounded differently, the derived bound applies.  d = 0: the same build.
BIT_EQUAL = {(4099, 200, 0, 1): True, (700, 300, 5, 1): True, (300, 70, 0, 64): True, (64, 64, 0, 64): True, (2048, 1472, 3, 1): False,
             (0, 48, 4, 64): True}
MU = 4.0               # exact instances
MU_ROUNDED = 0.5


@pytest.fixture
def ingest(bh):
    """Option gram_ingest = 1 for the duration of one test; upload_chunk_mb back at its default afterwards."""
    bh.set_option("gram_ingest", 1)
    try:
        yield bh
    finally:
        bh.set_option("gram_ingest", 0)
        bh.set_option("upload_chunk_mb", 64)


def integer_instance(d, n, q, seed=0):
    rng = np.random.default_rng(1000 * seed + d + n)
    return rng.integers(-3, 4, (d, n)).astype(np.float64), rng.integers(-2, 3, (q, n)).astype(np.float64)


def float_instance(d, n, q):
    rng = np.random.default_rng(77 + d + n)
    return rng.standard_normal((d, n)), rng.standard_normal((q, n))


def exact_gram(J, C, mu):
    """Integer entries, every partial sum an integer below 2^53: the float64 products are the integer result in any order."""
    return J.T @ J + mu * (C.T @ C)


def columns_of_G(H):
    e = np.zeros(H.n)
    G = np.empty((H.n, H.n))
    for j in range(H.n):
        e[j] = 1.0
        G[:, j] = H * e
        e[j] = 0.0
    return G


def ingest_handle(bh, J, C, mu, chunk_mb):
    bh.set_option("upload_chunk_mb", chunk_mb)
    H = bh.AlHessian.create_async(J, C, mu)
    H.wait()
    return H


# ------------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("d,n,q,chunk_mb", SHAPES)
def test_exact_instances(ingest, d, n, q, chunk_mb):
    bh = ingest
    J, C = integer_instance(d, n, q)
    H = ingest_handle(bh, J, C, MU, chunk_mb)
    assert H.form == "gram"
    assert H.gram_builds == (1 if d > 0 else 0)             # d = 0: no upload thread, the ordinary lazy build at the first product
    G = columns_of_G(H)
    assert H.gram_builds == 1                               # the first product launched no build
    ref = exact_gram(J, C, MU)
    assert np.abs(ref).max() < 2.0 ** 53
    assert np.array_equal(G, ref), (d, n, q, int(np.count_nonzero(G != ref)))
    assert np.array_equal(G, G.T)
    # integer vectors: exact products
    v = np.random.default_rng(5).integers(-4, 5, n).astype(np.float64)
    assert np.array_equal(H * v, ref @ v)
    H.close()


# ----------------------------------------------------------------------------------------------------------------- rounded
@pytest.mark.parametrize("d,n,q,chunk_mb", SHAPES)
def test_rounded_instances_against_the_one_shot_build(ingest, d, n, q, chunk_mb):
    bh = ingest
    J, C = float_instance(d, n, q)
    H = ingest_handle(bh, J, C, MU_ROUNDED, chunk_mb)
    assert H.form == "gram"
    G = columns_of_G(H)
    H.close()
    bh.set_option("gram_ingest", 0)
    P = bh.AlHessian(J, C, MU_ROUNDED)                       # the sequence without the option: synchronous create + set_form
    P.set_form("gram")
    Gp = columns_of_G(P)
    assert P.gram_builds == 1
    P.close()
    assert np.array_equal(G, G.T)
    k = d + q
    u = 2.0 ** -53
    gamma = k * u / (1.0 - k * u)
    bound = 2.0 * gamma * (np.abs(J).T @ np.abs(J) + MU_ROUNDED * (np.abs(C).T @ np.abs(C)))
    excess = np.abs(G - Gp) - bound
    print("gram_ingest rounded d=%d n=%d q=%d: max |G - G_oneshot| = %.3e, max bound = %.3e, entries differing: %d"
          % (d, n, q, np.abs(G - Gp).max(), bound.max(), np.count_nonzero(G != Gp)))
    assert np.all(excess <= 0.0), (d, n, q, float(excess.max()))
    if BIT_EQUAL[(d, n, q, chunk_mb)]:
        assert np.array_equal(G, Gp), (d, n, q, int(np.count_nonzero(G != Gp)))


# --------------------------------------------------------------------------------------------------------------- lifecycle
def test_build_count_and_new_mu(ingest):
    bh = ingest
    d, n, q = 700, 300, 5
    J, C = integer_instance(d, n, q, seed=1)
    H = ingest_handle(bh, J, C, MU, 1)
    assert H.form == "gram" and H.gram_builds == 1
    v = np.random.default_rng(6).integers(-4, 5, n).astype(np.float64)
    assert np.array_equal(H * v, exact_gram(J, C, MU) @ v)
    assert H.gram_builds == 1
    H.mu = 8.0
    assert H.gram_builds == 1                               # stale: rebuilt by the next product only
    assert np.array_equal(H * v, exact_gram(J, C, 8.0) @ v)
    H * v
    assert H.gram_builds == 2
    H.close()


def test_new_mu_while_the_upload_is_in_flight(ingest):
    """G of the upload belongs to the mu of the create call: a bh_hess_set_mu before the wait leaves it stale, as on any Gram handle."""
    bh = ingest
    d, n, q = 4099, 200, 3
    J, C = integer_instance(d, n, q, seed=2)
    bh.set_option("upload_chunk_mb", 1)
    H = bh.AlHessian.create_async(J, C, MU)
    H.mu = 2.0
    v = np.random.default_rng(7).integers(-4, 5, n).astype(np.float64)
    assert np.array_equal(H * v, exact_gram(J, C, 2.0) @ v)
    assert H.form == "gram" and H.gram_builds == 2
    H.close()


def test_destroy_and_leave_the_form_while_the_upload_is_in_flight(ingest):
    bh = ingest
    lib = bh._lib.lib()
    d, n, q = 4099, 200, 0
    J, C = integer_instance(d, n, q, seed=3)
    v = np.random.default_rng(8).integers(-4, 5, n).astype(np.float64)
    bh.set_option("upload_chunk_mb", 1)
    H = bh.AlHessian.create_async(J, C, MU)
    assert lib.bh_hess_destroy(H.handle) == bh._lib.BH_OK   # joins the worker and drains its Gram launches first
    H._h = type(H._h)()
    H = bh.AlHessian.create_async(J, C, MU)
    assert lib.bh_hess_set_form(H.handle, bh._lib.BH_HESS_IMPLICIT) == bh._lib.BH_OK
    assert H.form == "implicit"
    assert np.array_equal(H * v, J.T @ (J @ v))             # integers: the implicit product is exact too
    H.close()
    J2, C2 = integer_instance(d, n, q, seed=4)              # another J into the recycled image: no block may have read stale columns
    H = ingest_handle(bh, J2, C2, MU, 1)
    assert H.gram_builds == 1
    assert np.array_equal(H * v, exact_gram(J2, C2, MU) @ v)
    assert np.array_equal(columns_of_G(H), exact_gram(J2, C2, MU))
    H.close()
    bh.set_option("gram_ingest", 0)
    H = bh.AlHessian(J, C, MU)                              # an ordinary create and product afterwards
    assert H.form == "implicit" and np.array_equal(H * v, J.T @ (J @ v))
    H.close()


def test_two_ingests_in_a_row_are_bit_identical(ingest):
    bh = ingest
    d, n, q = 2048, 1472, 3
    J, C = float_instance(d, n, q)
    V = np.random.default_rng(9).standard_normal((4, n))
    out = []
    for _ in range(2):                                      # the second reuses the streams, the staging buffers and the partial blocks
        H = ingest_handle(bh, J, C, MU_ROUNDED, 1)
        assert H.gram_builds == 1
        out.append(np.stack([H * v for v in V]))
        H.close()
    assert np.array_equal(out[0], out[1])


def test_option_off_and_preconditions(bh):
    rng = np.random.default_rng(10)
    J = rng.standard_normal((300, 70))
    H = bh.AlHessian.create_async(J, None, 1.0)             # option 0: what the call always did
    H.wait()
    assert H.form == "implicit" and H.gram_builds == 0
    H.close()
    lib = bh._lib.lib()
    assert lib.bh_set_option(b"gram_ingest", 2) == bh._lib.BH_ERR_INVALID_ARG
    bh.set_option("gram_ingest", 1)
    try:
        W = bh.AlHessian.create_async(rng.standard_normal((2, 16385)), None, 1.0)     # n > 16384: an implicit handle
        W.wait()
        assert W.form == "implicit" and W.gram_builds == 0
        assert np.isfinite(W * rng.standard_normal(16385)).all()
        W.close()
        S = bh.AlHessian(J, None, 1.0)                      # the synchronous constructor does not read the option
        assert S.form == "implicit"
        S.close()
    finally:
        bh.set_option("gram_ingest", 0)


# -------------------------------------------------------------------------------------------------------------- downstream
def test_pcg_dev_on_a_golden_box_case(ingest):
    """bh_pcg_dev on the golden case box_q (d = 50, n = 20, q = 2: one block, one slab in both builds, G bit-equal) through an
    ingest-built handle and through a set_form-built one: the same status, counts and w, bit for bit."""
    bh = ingest
    c = [c for c in json.load(open(os.path.join(GOLD, "pcg_cases.json")))["cases"] if c["name"] == "box_q"][0]
    flt = lambda xs: np.array([float(x) for x in xs], dtype=np.float64)
    d, n, q = c["d"], c["n"], c["q"]
    J, C = flt(c["J"]).reshape((d, n), order="F"), flt(c["C"]).reshape((q, n), order="F")
    fix = np.array(c["fixvars"], dtype=bool)
    g, wl, wu = flt(c["g"]), flt(c["w_l"]), flt(c["w_u"])

    def run(H):
        cons = bh.MixedConstraints(np.zeros((0, n)), None, fix)
        vec = [bh.DeviceVector(n, x) for x in (g, wl, wu)]
        w = bh.DeviceVector(n)
        res = bh.projected_cg_dev(vec[0], H, vec[1], vec[2], cons, c["kappa2"], w)
        out = w.download()
        cons.close()
        return res, out

    H = ingest_handle(bh, J, C, c["mu"], 64)
    assert H.form == "gram" and H.gram_builds == 1
    res_i, w_i = run(H)
    assert H.gram_builds == 1
    H.close()
    bh.set_option("gram_ingest", 0)
    P = bh.AlHessian(J, C, c["mu"])
    P.set_form("gram")
    res_p, w_p = run(P)
    P.close()
    assert int(res_i[0]) == c["status"] and res_i == res_p
    assert np.array_equal(w_i, w_p)
