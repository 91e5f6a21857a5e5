"""row_stream_kernel and gn_gram_mfma_kernel in their steady-state loop, checked exactly.

The shapes come from tests/rs_cases.py: with the option blocks_per_cu = 1 (grid = number of compute units) every geometry of the
row-streaming kernel — and the column-panel path above n = 16384 — makes two and three passes over its row groups, so register
buffer B, the second LDS slot, the prefetch across the barrier, a partial last group behind full ones and a mu boundary inside a
later group all run (tests/test_rs_cases_cpu.py proves that from the launch geometry in the source).

B1/B2: integer-valued operands.  Every product and sum of these kernels is then exact in fp64 whatever the order, so the
       comparison with an int64 reference is bitwise and a wrong element is pinned to its row / column index.
B3:    badly scaled real operands against a long-double reference, per component, within the classical bound
       |fl(sum of m terms) - sum| <= gamma_m sum |terms|, gamma_m = m u / (1 - m u), u = 2^-53, which holds for any order of
       fma / add (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1 and 4.2).  The bounds are derived in the
       docstrings, none is fitted.
B4:    projected_cg through the multi-pass streams against the oracle.
"""
import ctypes as ct

import numpy as np
import pytest

import benlsip_ref as R
import rs_cases as rc
from _util import assert_w_close, note_tol, w_tolerance
from test_parity_gpu import cg_fused  # noqa: F401  (the fixture that walks the shapes of the CG iteration)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EXACT_LIMIT = 2 ** 52
CASE_IDS = [(p, t) for p in rc.PATHS for t in ("3A", "3a", "2B", "2b", "G", "g", "G1", "g1")
            if not (rc.config_of(p)[2] == 1 and t.islower())]


def _n_cu(bh):
    n = ct.c_int32(0)
    bh._lib.check(bh._lib.lib().bh_device_info(None, 0, ct.byref(n), None, 0), "bh_device_info")
    return int(n.value)


@pytest.fixture(scope="module")
def n_cu(bh):
    """Compute units of the device; pins the row-stream grid to it (blocks_per_cu = 1) for the module."""
    n = _n_cu(bh)
    bh.set_option("blocks_per_cu", 1)
    try:
        yield n
    finally:
        bh.set_option("blocks_per_cu", 0)


def test_case_table(n_cu, capsys):
    """Prints, once per session and past the capture, what every case makes the kernels do (shape, geometry, passes, tail
    rows), so that the log shows the steady-state loop ran for every geometry on this device."""
    lines = ["", "row-stream cases for %d compute units, blocks_per_cu = 1 (tests/rs_cases.py):" % n_cu]
    lines += ["  " + rc.describe(c, n_cu) for c in rc.cases(n_cu)]
    lines += ["Gram-build cases:"] + ["  " + rc.describe_gram(c, n_cu) for c in rc.GRAM_CASES + [rc.GRAM_WIDE_CASE]]
    with capsys.disabled():
        print("\n".join(lines))
    for c in rc.cases(n_cu):
        assert rc.stream_shape(c.path, c.d + c.q, n_cu, 1)["grid"] == n_cu


def _case(n_cu, path, tag):
    hits = [c for c in rc.cases(n_cu) if c.path == path and c.tag == tag]
    assert len(hits) == 1, (path, tag)
    return hits[0]


# --------------------------------------------------------------------------------------------------------------------- B1
class IntProblem:
    """Integer operands and their int64 products.  J is generated column-major (the layout bh_hess_create reads)."""

    def __init__(self, d, n, q, seed):
        rng = np.random.default_rng(seed)
        self.d, self.n, self.q = d, n, q
        self.Ji = rng.integers(-3, 4, size=(n, d), dtype=np.int8).T          # d x n, Fortran order
        self.Ci = rng.integers(-3, 4, size=(n, q), dtype=np.int8).T
        v = rng.integers(-1, 2, size=n)
        v[:min(n, 3)] = np.array([-1, 0, 1])[:min(n, 3)]                      # both signs and a zero, whatever the draw
        self.v = rng.permutation(v).astype(np.int64)
        self.u = rng.integers(-3, 4, size=d).astype(np.int64)
        self.r = rng.integers(-3, 4, size=d).astype(np.int64)
        self.ybar = rng.integers(-3, 4, size=q).astype(np.int64)
        self.g = rng.integers(-3, 4, size=n).astype(np.int64)
        self.J64, self.C64 = self.Ji.astype(np.int64), self.Ci.astype(np.int64)
        self._kept = None
        self._jtu = self._grad = None

    def floats(self):
        return self.Ji.astype(np.float64), self.Ci.astype(np.float64)

    def _images(self, v):
        """(J v, C v, J'(J v), C'(C v)) in int64; kept for the case's own v (asked for at every mu and form)."""
        if v is self.v and self._kept is not None:
            return self._kept
        t, c = self.J64 @ v, self.C64 @ v
        out = (t, c, self.J64.T @ t, self.C64.T @ c)
        if v is self.v:
            self._kept = out
        return out

    def hv2(self, mu, v):
        """2 H v = 2 J'(J v) + (2 mu) C'(C v): integral for mu in {0.5, 2}."""
        m2 = int(round(2 * mu))
        assert m2 == 2 * mu
        t, c, jt, ct_ = self._images(v)
        return 2 * jt + m2 * ct_

    def vthv2(self, mu, v):
        m2 = int(round(2 * mu))
        t, c, _, _ = self._images(v)
        return 2 * int(t @ t) + m2 * int(c @ c)

    def assert_exactly_representable(self, vectors):
        """Condition on the INPUTS: no intermediate of any product, in any summation order, reaches 2^52 (then every fma of the
        kernels is exact).  Bounded through the absolute values: |J||v|, |J|'(W |J||v|), sum W (|J||v|)^2, each doubled for the
        half-integers of mu = 0.5 and taken at the larger mu = 2."""
        Ja, Ca = np.abs(self.J64), np.abs(self.C64)
        worst = 0
        for v in vectors:
            va = np.abs(v)
            t, c = Ja @ va, Ca @ va
            z = 2 * (Ja.T @ t) + 4 * (Ca.T @ c) + 2 * np.abs(self.g)
            worst = max(worst, int(z.max(initial=0)), 2 * int(t @ t) + 4 * int(c @ c))
        ua = np.maximum(np.abs(self.u), np.abs(self.r))
        worst = max(worst, int((Ja.T @ ua + Ca.T @ np.abs(self.ybar)).max(initial=0)))
        assert worst < EXACT_LIMIT, worst
        return worst


def _same(got, want, what):
    """Bitwise equality with the int64 reference (given as numerator / 2), naming the first wrong indices."""
    want = np.asarray(want, dtype=np.float64)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(~(np.asarray(got) == want))
        raise AssertionError("%s: %d of %d entries differ; first at %s: got %s, want %s"
                             % (what, bad.size, want.size, bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), want[bad[:8]].tolist()))


def _hmul_dev(bh, H, v):
    dv, dout = bh.DeviceVector(H.n, v), bh.DeviceVector(H.n)
    bh._lib.check(bh._lib.lib().bh_hmul_dev(H.handle, dv.ptr, dout.ptr), "bh_hmul_dev")
    out = dout.download()
    dv.close()
    dout.close()
    return out


def _check_products(bh, H, P, mu, label, rows_too=True):
    v = P.v
    hv = P.hv2(mu, v) / 2.0
    if rows_too:
        if P._jtu is None:
            P._jtu, P._grad = P.J64.T @ P.u, P.J64.T @ P.r + P.C64.T @ P.ybar
        _same(H.jv(v), P._images(v)[0], label + " jv")
        _same(H.jtv(P.u), P._jtu, label + " jtv")
        _same(bh.gradient(H, P.r, P.ybar), P._grad, label + " bh_grad")
        assert bh.vthv(H, v) == P.vthv2(mu, v) / 2.0, label + " vthv"
    _same(H * v, hv, label + " H*v")
    _same(_hmul_dev(bh, H, v), hv, label + " bh_hmul_dev")
    _same(bh.hmul_add(H, v, P.g), hv + P.g, label + " hmul_add")


def _exact_round_trip(bh, case, seed, n_cu):
    P = IntProblem(case.d, case.n, case.q, seed)
    P.assert_exactly_representable([P.v])
    Jf, Cf = P.floats()
    H = bh.AlHessian(Jf, Cf, 0.5)
    del Jf
    try:
        _check_products(bh, H, P, 0.5, "implicit mu=0.5")
        H.mu = 2.0                                              # changed once, on the live handle
        _check_products(bh, H, P, 2.0, "implicit mu=2")
        if case.n <= 16384:
            H.set_form("gram")
            assert H.form == "gram" and H.gram_builds == 0
            _check_products(bh, H, P, 2.0, "gram mu=2")         # H*v, bh_hmul_dev, hmul_add read G; the others still read J
            assert H.gram_builds == 1
            H.mu = 0.5
            _check_products(bh, H, P, 0.5, "gram mu=0.5", rows_too=False)
            assert H.gram_builds == 2
            H.set_form("implicit")
        else:
            assert bh._lib.lib().bh_hess_set_form(H.handle, bh._lib.BH_HESS_GRAM) == bh._lib.BH_ERR_UNSUPPORTED
            H.mu = 0.5
        # back in the implicit form: a stray write into the image or the slab buffers would show here
        assert H.form == "implicit"
        _check_products(bh, H, P, 0.5, "implicit again mu=0.5")
    finally:
        H.close()


@pytest.mark.parametrize("path,tag", CASE_IDS, ids=["%s-%s" % (p, t) for p, t in CASE_IDS])
def test_products_are_bit_exact_on_integer_operands(bh, n_cu, path, tag):
    """jv, jtv, H*v, bh_hmul_dev, hmul_add, bh_grad and vthv on J, C in [-3, 3], v in {-1, 0, 1}, u, r, ybar, g in [-3, 3],
    mu = 0.5 then 2: equal to the int64 products bit for bit; the same through G after set_form("gram") (one build per mu), and
    again after the return to the implicit form."""
    case = _case(n_cu, path, tag)
    s = rc.stream_shape(path, case.d + case.q, n_cu, 1)
    assert s["grid"] == n_cu
    _exact_round_trip(bh, case, 7000 + 13 * rc.PATHS.index(path) + CASE_IDS.index((path, tag)), n_cu)


@pytest.mark.parametrize("d,n,q", [(4101, 1501, 3), (2053, 6001, 2), (1100, 16400, 1)])
def test_products_are_bit_exact_at_the_shipped_grids(bh, n_cu, d, n, q):
    """The same at the default blocks_per_cu (geometry 3 with 512 workgroups, geometry 5 and the panel path with 256): several
    passes per workgroup there too."""
    bh.set_option("blocks_per_cu", 0)
    try:
        path = rc.path_of(n)
        assert rc.stream_shape(path, d + q, n_cu, 0)["passes"] >= 2
        _exact_round_trip(bh, rc.Case(d, n, q, path, "default"), 7900 + n, n_cu)
    finally:
        bh.set_option("blocks_per_cu", 1)


# --------------------------------------------------------------------------------------------------------------------- B2
def _gram_columns(H, n):
    return np.stack([H * e for e in np.eye(n)], axis=1)


@pytest.mark.parametrize("c", rc.GRAM_CASES, ids=["d%d-n%d-q%d" % (c.d, c.n, c.q) for c in rc.GRAM_CASES])
def test_gram_matrix_is_bit_exact(bh, n_cu, c):
    """G = J'J + mu C'C extracted column by column (H * e_i) equals the int64 Gram matrix exactly, is exactly symmetric, and
    its last valid column carries nothing from the padding (the column of e_{n-1} and a product with a vector supported there
    are exact) — over the slab situations of rs_cases.GRAM_CASES, for mu = 0.5 and after a rebuild for mu = 2."""
    P = IntProblem(c.d, c.n, c.q, 8100 + c.d + c.n)
    P.assert_exactly_representable([P.v, np.ones(c.n, dtype=np.int64)])
    slabs, slab_rows = rc.gram_geometry(c.d + c.q, rc.ld_of(c.n), n_cu)
    Jf, Cf = P.floats()
    H = bh.AlHessian(Jf, Cf, 0.5)
    H.set_form("gram")
    try:
        for k, mu in enumerate((0.5, 2.0)):
            H.mu = mu
            G2 = 2 * (P.J64.T @ P.J64) + int(2 * mu) * (P.C64.T @ P.C64)
            G = _gram_columns(H, c.n)
            assert H.gram_builds == k + 1
            bad = np.argwhere(G != G2 / 2.0)
            assert bad.size == 0, "mu=%g, %d slabs of %d rows: %d entries of G differ, first (row, col) %s" % (
                mu, slabs, slab_rows, len(bad), bad[:6].tolist())
            assert np.array_equal(G, G.T)
            last = np.zeros(c.n, dtype=np.int64)
            last[-1] = 3
            _same(H * last, 3 * G2[:, -1] / 2.0, "G * (3 e_last)")
            _same(bh.hmul_add(H, last, P.g), 3 * G2[:, -1] / 2.0 + P.g, "G * (3 e_last) + g")
            _same(_hmul_dev(bh, H, P.v), P.hv2(mu, P.v) / 2.0, "bh_hmul_dev")
    finally:
        H.close()


def test_gram_matrix_is_bit_exact_for_a_wide_image(bh, n_cu):
    """4096 < n <= 16384 (one slab, geometry 5 or 6 for G v): G probed with integer vectors instead of all columns — unit
    vectors at both ends and inside, their symmetric partners, and dense vectors in {-1, 0, 1}."""
    c = rc.GRAM_WIDE_CASE
    P = IntProblem(c.d, c.n, c.q, 8200)
    rng = np.random.default_rng(8201)
    dense = [P.v] + [rng.integers(-1, 2, size=c.n).astype(np.int64) for _ in range(2)]
    P.assert_exactly_representable(dense)
    Jf, Cf = P.floats()
    H = bh.AlHessian(Jf, Cf, 0.5)
    H.set_form("gram")
    try:
        for v in dense:
            _same(H * v, P.hv2(0.5, v) / 2.0, "G v")
        idx = [0, 1, 63, 64, 4095, 4096, c.n - 2, c.n - 1]
        cols = {}
        for i in idx:
            e = np.zeros(c.n, dtype=np.int64)
            e[i] = 1
            cols[i] = H * e
            _same(cols[i], P.hv2(0.5, e) / 2.0, "G e_%d" % i)
        for i in idx:
            for j in idx:
                assert cols[i][j] == cols[j][i], (i, j)
        assert H.gram_builds == 1
    finally:
        H.close()


# --------------------------------------------------------------------------------------------------------------------- B3
def _scaled(rng, rows, n):
    """D_r N D_c with N standard normal and D_r, D_c powers of two from 2^-30 to 2^30.  Exponents are dealt out with strides
    coprime to 61, so consecutive rows (one row group) and the two columns of a 16-byte chunk (one lane) differ by up to 2^60."""
    er = (np.arange(rows) * 37) % 61 - 30
    ec = (np.arange(n) * 23) % 61 - 30
    N = rng.standard_normal((n, rows)).T                          # Fortran order
    return N * np.ldexp(1.0, er)[:, None] * np.ldexp(1.0, ec)[None, :]


def _ratio(label, got, ref_l, bound_l, detail):
    """Worst |got - ref| / bound over the components (a zero bound demands a zero error); recorded for the tolerance table."""
    err = np.abs(got.astype(np.longdouble) - ref_l)
    assert np.all(err[bound_l == 0] == 0), (label, detail)
    m = bound_l > 0
    ratio = float(np.max(err[m] / bound_l[m])) if m.any() else 0.0
    note_tol(label, ratio, 1.0, detail)
    i = int(np.argmax(np.where(m, err / np.where(m, bound_l, 1), 0))) if m.any() else -1
    assert ratio <= 1.0, "%s %s: component %d off by %.3e, bound %.3e" % (label, detail, i, float(err[i]), float(bound_l[i]))


@pytest.mark.parametrize("path,tag", [(p, t) for p in rc.PATHS for t in ("2B", "3A")],
                         ids=["%s-%s" % (p, t) for p in rc.PATHS for t in ("2B", "3A")])
def test_products_meet_the_componentwise_rounding_bound(bh, n_cu, path, tag):
    """Badly scaled J = D_r N D_c and C (entries over 2^-60 ... 2^60 relative to N), v, u, g standard normal, mu = 0.7, at one odd
    inside n (tag 2B) and the edge n (tag 3A) of every path, multi-pass row counts.  Reference: the same products in long double.

    With u = 2^-53 and gamma_m = m u / (1 - m u) <= 1.001 m u for the m used here, per component:

      jv      t_i = sum_j J_ij v_j has ld terms (fma chains per lane, a fixed tree over the lanes, waves and — wide images —
              panels): |t^_i - t_i| <= gamma_ld (|J||v|)_i.                                  Asserted with m = ld + 8.
      jtv     z_j = sum_i J_ij u_i has `rows` terms (one chain per workgroup, a fixed tree over the workgroups):
              |z^_j - z_j| <= gamma_rows (|J|'|u|)_j.                                        Asserted with m = rows + 8.
      H*v     z_j = sum_i J_ij w_i t_i, w_i in {1, mu}: the computed coefficient is w_i t_i (1 + e_i), |e_i| <= gamma_(ld+1)
              (the sum above, one rounding for mu t_i), then `rows` terms: to first order gamma_(ld+rows+1) (|J|'W|J||v|)_j, with
              the higher-order terms (1 + gamma_a)(1 + gamma_b) - 1 <= gamma_(a+b).          Asserted with m = 2 (ld + rows + 8).
      hmul_add  one more rounding of z_j + g_j:  m u (|J|'W|J||v| + |g|)_j with the same m.
      Gram    G^_jk = sum_i J_ij (w_i J_ik): one rounding for w_i J_ik, `rows` terms in the order of the matrix cores, waves and
              slabs: |G^ - G| <= gamma_(rows+1) |J|'W|J|; then (G^ v)_j over ld terms: |G^v^ - G v| <= (gamma_ld + gamma_(rows+1)
              (1 + gamma_ld)) |J|'W|J||v| <= gamma_(ld+rows+1) (|J|'W|J|)|v|, and (|J|'W|J|)|v| = |J|'W(|J||v|), the bar of the
              implicit form.  Forming G first costs the rounding of the ld-term sum ON TOP of already rounded entries instead of
              inside one nest; it is granted as one more gamma_ld:                            m = 2 (ld + rows + 8) + ld.
    The asserted m leave a factor of about two over the first-order constants; nothing is fitted to what the kernels reach.
    The long-double reference (u_l = 2^-64) carries the same sums with gamma^l_m = m 2^-64 <= 2^-11 of the bound: ignored."""
    case = _case(n_cu, path, tag)
    d, n, q = case.d, case.n, max(case.q, 1)
    rows, ld = d + q, rc.ld_of(n)
    rng = np.random.default_rng(9000 + 17 * rc.PATHS.index(path) + len(tag) + d)
    J, C, mu = _scaled(rng, d, n), _scaled(rng, q, n), 0.7
    v, u, g = rng.standard_normal(n), rng.standard_normal(d), rng.standard_normal(n) * 2.0 ** 40
    detail = "path %s d=%d n=%d q=%d" % (path, d, n, q)
    L = np.longdouble
    Jl, Cl, vl = J.astype(L), C.astype(L), v.astype(L)
    Ja, Ca, va = np.abs(Jl), np.abs(Cl), np.abs(vl)
    t_ref, t_bar = Jl @ vl, Ja @ va
    c_ref, c_bar = Cl @ vl, Ca @ va
    z_ref = Jl.T @ t_ref + Cl.T @ (L(mu) * c_ref)
    z_bar = Ja.T @ t_bar + Ca.T @ (L(mu) * c_bar)
    H = bh.AlHessian(J, C, mu)
    try:
        _ratio("row-stream J v: componentwise error / gamma_(ld+8) |J||v|", H.jv(v), t_ref, (ld + 8) * L(U) * t_bar, detail)
        _ratio("row-stream J'u: componentwise error / gamma_(rows+8) |J|'|u|", H.jtv(u), Jl.T @ u.astype(L), (d + 8) * L(U) * (Ja.T @ np.abs(u).astype(L)), detail)
        m = 2 * (ld + rows + 8)
        _ratio("row-stream H*v: componentwise error / gamma_2(ld+rows+8) |J|'W|J||v|", H * v, z_ref, m * L(U) * z_bar, detail)
        _ratio("row-stream hmul_add: componentwise error / gamma_2(ld+rows+8) (|J|'W|J||v| + |g|)", bh.hmul_add(H, v, g), z_ref + g.astype(L),
               m * L(U) * (z_bar + np.abs(g).astype(L)), detail)
        if n <= 16384:
            H.set_form("gram")
            mg = m + ld
            _ratio("Gram form H*v: componentwise error / gamma_(2(ld+rows+8)+ld) (|J|'W|J|)|v|", H * v, z_ref, mg * L(U) * z_bar, detail)
            _ratio("Gram form hmul_add: componentwise error / gamma_(2(ld+rows+8)+ld) ((|J|'W|J|)|v| + |g|)", bh.hmul_add(H, v, g),
                   z_ref + g.astype(L), mg * L(U) * (z_bar + np.abs(g).astype(L)), detail)
    finally:
        H.close()


# --------------------------------------------------------------------------------------------------------------------- B4
_PCG_ORACLE = {}


def _pcg_instance(path, n, nfix, kappa2, n_cu):
    """Instance and oracle answer, computed once for the three shapes of the CG iteration."""
    key = (path, n_cu)
    if key not in _PCG_ORACLE:
        Rr = rc.config_of(path)[2]
        d = max((n + 7) // 8, 2 * n_cu * Rr + 37)                # >= 3 passes at blocks_per_cu = 1, d >= n / 8
        rng = np.random.default_rng(n + d)
        J = rng.standard_normal((d, n)) / np.sqrt(d)
        fix = np.zeros(n, dtype=bool)
        fix[rng.choice(n, nfix, replace=False)] = True
        A = np.zeros((0, n))
        cons_o = R.make_mixed_constraints(A, R.chol_lower(A @ A.T), fix, l=-np.ones(n), u=np.ones(n))
        g = J.T @ rng.standard_normal(d) + 1e-3 * rng.standard_normal(n)
        w_l, w_u = R.build_step_bounds(np.where(fix, 1.0, 0.0), cons_o, 0.5 * np.linalg.norm(g))
        Ho = R.AlHessian(J, np.zeros((0, n)), 2.0)
        tr = R.CGTrace()
        w_ref, s_ref, it_ref = R.projected_cg(g, Ho, w_l, w_u, cons_o, kappa2, trace=tr)
        tol = w_tolerance(g, Ho, w_l, w_u, cons_o, kappa2, w_ref)
        _PCG_ORACLE[key] = dict(d=d, J=J, fix=fix, A=A, g=g, w_l=w_l, w_u=w_u, tr=tr, w_ref=w_ref, s_ref=s_ref, it_ref=it_ref, tol=tol)
    return _PCG_ORACLE[key]


@pytest.mark.parametrize("path,n,nfix,kappa2", [(3, 1100, 200, 0.01), (5, 6001, 300, 0.1), (6, 9001, 700, 0.1), (rc.PANEL, 16400, 500, 0.3)],
                         ids=["geometry3", "geometry5", "geometry6", "panels"])
def test_pcg_through_the_multi_pass_streams(bh, n_cu, cg_fused, path, n, nfix, kappa2):
    """projected_cg with box constraints where every H*p launch makes three passes (the CG prologue ahead of a multi-pass
    stream; the column-panel pair of sweeps above n = 16384), d >= n / 8, a few hundred fixed variables: status, iteration
    count, n_hmul, w and the scalar trace against the oracle, and a second call — launch schedule from the hint, the launch
    expected to stop on its own symbol — bit-identical to the first."""
    assert rc.path_of(n) == path
    I = _pcg_instance(path, n, nfix, kappa2, n_cu)
    assert rc.stream_shape(path, I["d"], n_cu, 1)["passes"] >= 3 and 8 * I["d"] >= n
    tr = I["tr"]
    H = bh.AlHessian(I["J"], None, 2.0)
    cons = bh.MixedConstraints(I["A"], None, I["fix"])
    try:
        w, status, info = bh.projected_cg(I["g"], H, I["w_l"], I["w_u"], cons, kappa2, trace_cap=32, full_output=True)
        assert int(status) == int(I["s_ref"]) and info["iters"] == I["it_ref"] and info["n_hmul"] == tr.n_hmul, (
            status, info["iters"], info["n_hmul"], I["s_ref"], I["it_ref"], tr.n_hmul)
        assert_w_close(w, I["w_ref"], I["tol"], "projected_cg: w vs oracle (tolerance max(1e-9, 20 x oracle sensitivity))",
                       "multi-pass path %s cg_fused=%d" % (path, cg_fused))
        k = min(len(tr.rows), 32)
        ref_rows = np.array(tr.rows[:k])
        m = np.isfinite(ref_rows)
        np.testing.assert_allclose(info["trace"][:k][m], ref_rows[m], rtol=1e-6, atol=1e-12)
        w2, status2, info2 = bh.projected_cg(I["g"], H, I["w_l"], I["w_u"], cons, kappa2, full_output=True)
        assert np.array_equal(w, w2) and int(status2) == int(status) and info2["iters"] == info["iters"] and info2["n_hmul"] == info["n_hmul"]
    finally:
        H.close()
        cons.close()
