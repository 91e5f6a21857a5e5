"""The resident inner-step chain on the compact image of the free columns (option free_image_chain).

With free_image_chain = 1 a bh_minor_iterate_dev made under step_from_cg = 1 is considered for the compact image like one made under
free_image_minor = 1 with step_from_cg = 0; its line search also keeps the free part of H*w scaled with w, and the
bh_step_accumulate_dev behind it adds that to g_minor on the free variables only (free_image_step_accumulate_kernel) while the model
value q(s) = g.s + s'Hs / 2 is carried on the device, so that bh_model_reduction_dev needs no sweep either.

What is compared with what:
  * the minor iterate itself against the SAME call under (free_image_minor = 1, step_from_cg = 0) on the same operands: the two run
    the same loop and the same line search arithmetic (the chain's kernel only stores one more word per slot), so w, status, iters,
    n_hmul and alpha are demanded equal as uint64;
  * the accumulate against the oracle's H (s0 + w) + g on the free variables with the 1e-12 rule of
    test_parity_gpu.py::test_step_accumulate_takes_hw_from_the_cg_loop, and against the uploaded g_minor, bit for bit, on the fixed ones;
  * the model value against g.s + s'Hs / 2 of the oracle with that test's 1e-10 (|g||s| + s'Hs) rule;
  * on dyadic data (exact in any order) against the exact values and against the two chains the library already had, bit for bit.

The exact chain.  With J'J = 16 I alone the chain degenerates: projected CG is exact after one product, so g_minor is zero on every free
variable after the first step, and with nested active sets every later minor iterate sees mask(g_minor) = 0 (alpha = Inf * 0).  The
instance below keeps free_image_cases.exact_jacobian and doubles a set B of its columns (J'J = diag(16, 64), still orthogonal columns
and integer entries): with sum_A gm^2 = 2 sum_B gm^2 over the free variables the first CG step is 1/32, the loop is stopped after it by
a large kappa2, the line search gives alpha = 1, and g_minor becomes gm / 2 on A and -gm on B — non-zero, and again dyadic.  The three
nested free sets are chosen so that the same relation holds for each step's g_minor (see _exact_chain).

The negative-curvature iterate.  A step along negative curvature goes to the boundary (:727-729), and minor_iterate gives +-Inf bounds to
every free variable: with mu < 0 the closed-form case of _util.closed_form_cases yields w = +-Inf, which no chain can be checked on.
The instance here takes the other branch of :725-727 — p'Hp = 0 exactly — at the SECOND direction, so that the loop stops with status
negative_curvature holding the w of its first step, which then stays unscaled: J'J = diag(16 on A, 0 on B), sum_A gm^2 = sum_B gm^2 over
the free variables: the first step is 1/8, beta = 1, p_2 = (0, -2 gm_B), J p_2 = 0.
"""
import ctypes as ct

import numpy as np
import pytest

import benlsip_ref as R
import free_image_cases as F
from _util import note_tol, relnorm
from test_free_image_exact_gpu import INNER
from test_free_image_gpu import _bits

pytestmark = pytest.mark.gpu

DELTA = 1.0                # only the fixed variables get finite step bounds from it, and the box loop never reads those
ACC_LABEL = "bh_step_accumulate_dev: g_minor vs the oracle's H*(s+w)+g (1e-12 of the operands' scale)"
MR_LABEL = "bh_model_reduction_dev vs oracle (1e-10 of |g||s| + s'Hs)"
OPTIONS = {"free_image": 1, "free_image_minor": 0, "free_image_chain": 0, "ls_from_cg": 1, "step_from_cg": 0}


@pytest.fixture(scope="module")
def n_cu(bh):
    n = ct.c_int32(0)
    bh._lib.check(bh._lib.lib().bh_device_info(None, 0, ct.byref(n), None, 0), "bh_device_info")
    bh.set_option("blocks_per_cu", 1)
    try:
        yield int(n.value)
    finally:
        _restore(bh)
        bh.set_option("blocks_per_cu", 0)


def _restore(bh):
    lib = bh._lib.lib()
    for key, value in OPTIONS.items():
        lib.bh_set_option(key.encode(), value)      # (free_image_chain does not exist on the parent: no check here)


def _mode(bh, chain, minor, sfc, free_image=2):
    bh.set_option("free_image", free_image)
    bh.set_option("free_image_minor", minor)
    bh.set_option("free_image_chain", chain)
    bh.set_option("step_from_cg", sfc)


def _box(n):
    return -F.XB * np.ones(n), F.XB * np.ones(n)


def _constraints(bh, n, fix):
    lo, up = _box(n)
    return bh.MixedConstraints(np.zeros((0, n)), None, fix, l=lo, u=up)


class Chain:
    """The resident vectors of one chain (x = 0) and the calls on them."""

    def __init__(self, bh, H, n, s0, g, gm0=None):
        self.bh, self.H, self.n = bh, H, n
        self.lib, self.chk = bh._lib.lib(), bh._lib.check
        lo, up = _box(n)
        self.v = {k: bh.DeviceVector(n, a) for k, a in (("x", np.zeros(n)), ("s", s0), ("g", g), ("lo", lo), ("up", up),
                                                        ("w", np.full(n, 7.25)), ("gm", np.zeros(n) if gm0 is None else gm0))}
        if gm0 is None:                                  # the library writes g_minor = H s + g itself, as inner_step does (:412)
            self.chk(self.lib.bh_hmul_add_dev(H.handle, self.v["s"].ptr, self.v["g"].ptr, self.v["gm"].ptr), "bh_hmul_add_dev")

    def minor(self, P, kappa2=F.KAPPA2, w=None):
        P._sync()
        v = self.v
        status, iters, n_hmul, alpha = ct.c_int32(-1), ct.c_int32(0), ct.c_int32(0), ct.c_double(0.0)
        wv = v["w"] if w is None else w
        self.chk(self.lib.bh_minor_iterate_dev(self.H.handle, P.handle, v["x"].ptr, v["s"].ptr, v["gm"].ptr, v["lo"].ptr, v["up"].ptr, DELTA,
                                               float(kappa2), self.bh.operators.SQRT_EPS, 1e-10, wv.ptr, ct.byref(status), ct.byref(iters),
                                               ct.byref(n_hmul), ct.byref(alpha)), "bh_minor_iterate_dev")
        return wv.download(), status.value, iters.value, n_hmul.value, alpha.value

    def accumulate(self, w=None):
        """-> (growth of n_hmul, growth of n_jv)."""
        v = self.v
        before = self.H.stats()
        self.chk(self.lib.bh_step_accumulate_dev(self.H.handle, v["s"].ptr, (v["w"] if w is None else w).ptr, v["g"].ptr, v["gm"].ptr),
                 "bh_step_accumulate_dev")
        after = self.H.stats()
        return after["n_hmul"] - before["n_hmul"], after["n_jv"] - before["n_jv"]

    def model(self):
        """-> (value, growth of n_jv)."""
        mr, j0 = ct.c_double(0.0), self.H.stats()["n_jv"]
        self.chk(self.lib.bh_model_reduction_dev(self.H.handle, self.v["g"].ptr, self.v["s"].ptr, ct.byref(mr)), "bh_model_reduction_dev")
        return mr.value, self.H.stats()["n_jv"] - j0

    def get(self, key):
        return self.v[key].download()

    def close(self):
        for a in self.v.values():
            a.close()


def _same_call(a, b, what):
    """Two minor iterates: w, status, iters, n_hmul, alpha as uint64."""
    assert a[1:4] == b[1:4], (what, a[1:4], b[1:4])
    assert _bits(a[4]).tolist() == _bits(b[4]).tolist(), (what, "alpha", a[4], b[4])
    bad = np.flatnonzero(_bits(a[0]) != _bits(b[0]))
    assert bad.size == 0, (what, "w differs at", bad[:8], a[0][bad[:8]], b[0][bad[:8]])


def _assert_model(value, g, s, Ho, what):
    """The 1e-10 rule of test_parity_gpu.py::test_step_accumulate_takes_hw_from_the_cg_loop."""
    shs = R.vthv(Ho, s)
    ref = float(g @ s) + 0.5 * shs
    bound = 1e-10 * (np.linalg.norm(g) * np.linalg.norm(s) + shs)
    print("[%s] model reduction %r, explicit %r: |difference| %.3e, bound %.3e" % (what, value, ref, abs(value - ref), bound))
    note_tol(MR_LABEL, abs(value - ref), bound, what)
    assert abs(value - ref) <= bound, (what, value, ref, bound)


def _assert_free_part(gm1, s1, w, s0, g, I, fix, what):
    """The 1e-12 rule of the same test, on the free variables."""
    Jabs = np.abs(I["J"])
    scale = np.linalg.norm(Jabs.T @ (Jabs @ np.abs(s0))) + np.linalg.norm(g) + 1e-300
    ref = R.hmul(I["Ho"], s1) + g
    err = np.linalg.norm((gm1 - ref)[~fix]) / (scale + np.linalg.norm(Jabs.T @ (Jabs @ np.abs(w))))
    print("[%s] g_minor on the free variables vs oracle: %.3e of the operands' scale (bound 1e-12)" % (what, err))
    note_tol(ACC_LABEL, err, 1e-12, what)
    assert err <= 1e-12, (what, err)


# ---------------------------------------------------------------------------------------------------------------- 1. the key
def test_the_option_exists_defaults_to_zero_and_rejects_other_values(bh, n_cu):
    lib = bh._lib.lib()
    I = F.instance("S3", n_cu)
    st = F.states("S3")[0]
    n = I["n"]
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = _constraints(bh, n, st.fix.copy())
    ch = Chain(bh, H, n, np.zeros(n), I["g"])
    try:
        for bad in (2, -1):
            assert lib.bh_set_option(b"free_image_chain", bad) == bh._lib.BH_ERR_INVALID_ARG
        # the default (every test of this module restores 0): the chain's minor iterate stays on the full image
        bh.set_option("free_image", 2)
        bh.set_option("step_from_cg", 1)
        ch.minor(P)
        assert H.free_image_info(None)["calls_served"] == 0 and H.free_image_info(None)["builds"] == 0
        assert lib.bh_set_option(b"free_image_chain", 1) == 0                # fails where the option does not exist
        ch.minor(P)
        assert H.free_image_info(P)["calls_served"] == 1
        assert lib.bh_set_option(b"free_image_chain", 2) == bh._lib.BH_ERR_INVALID_ARG      # a rejected value leaves it as it was
        ch.minor(P)
        assert H.free_image_info(P)["calls_served"] == 2
        assert lib.bh_set_option(b"free_image_chain", 0) == 0
        ch.minor(P)
        assert H.free_image_info(P)["calls_served"] == 2
    finally:
        _restore(bh)
        ch.close()
        H.close()
        P.close()


# ------------------------------------------------------------------- 2. the minor iterate, 3. the accumulate behind it, S1 ... S5
@pytest.mark.parametrize("name", list(F.SEQS))
def test_minor_iterate_and_accumulate_in_the_chain_through_the_sequences(bh, n_cu, name):
    I = F.instance(name, n_cu)
    n, g, Ho = I["n"], I["g"], I["Ho"]
    sts = F.states(name)
    rng = np.random.default_rng(77)
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    cons = {}
    try:
        for k, st in enumerate(sts):
            what = "%s state %d (width %d, %s %d)" % (name, k, st.width, st.action, st.k)
            if st.who not in cons:
                cons[st.who] = _constraints(bh, n, st.fix.copy())
            elif not np.array_equal(cons[st.who].fixvars, st.fix):
                cons[st.who].fixvars = st.fix.copy()
            P = cons[st.who]
            s0 = 0.01 * rng.standard_normal(n)                      # non-zero on the fixed variables too
            gm0 = R.hmul(Ho, s0) + g                                # from the oracle: not the library's own g_minor
            ch = Chain(bh, H, n, s0, g, gm0=gm0)
            try:
                served = H.free_image_info(None)["calls_served"]
                _mode(bh, chain=0, minor=1, sfc=0)
                ref = ch.minor(P)
                assert H.free_image_info(P)["calls_served"] == served + 1, what
                _mode(bh, chain=1, minor=0, sfc=1)
                got = ch.minor(P)                                   # this fails on the parent: no such option, the call is not served
                assert H.free_image_info(P)["calls_served"] == served + 2, what
                _same_call(got, ref, what)
                assert got[1] == int(R.CGStatus.solved) and not _bits(got[0][st.fix]).any(), (what, got[1:])
                # 3. the accumulate right behind it
                w = got[0]
                d_hmul, d_jv = ch.accumulate()
                assert (d_hmul, d_jv) == (0, 0), (what, d_hmul, d_jv)
                s1, gm1 = ch.get("s"), ch.get("gm")
                assert np.array_equal(_bits(s1), _bits(s0 + w)), what
                _assert_free_part(gm1, s1, w, s0, g, I, st.fix, what)
                assert np.array_equal(_bits(gm1[st.fix]), _bits(gm0[st.fix])), (what, "g_minor has moved on a fixed variable")
                # g_minor was not the library's own: no q could be carried, and a stale g_minor is not used — the J v sweep
                value, d_jv = ch.model()
                assert d_jv == 1, what
                _assert_model(value, g, s1, Ho, what)
            finally:
                _restore(bh)
                ch.close()
    finally:
        _restore(bh)
        H.close()
        for P in cons.values():
            P.close()


# ----------------------------------------------------------------------------------------------- 4. three exact steps (integers)
def _exact_chain():
    """n, J (J'J = diag(16 on A, 64 on B)), h = diag(H), the three nested active sets, g and s0 (dyadic, s0 non-zero everywhere) such that
    G = H s0 + g has: on free_3: 10 A entries +-4 and 5 B entries +-1 (160 = 32 * 5); on free_2 \\ free_3: 10 A entries +-4 and 35 B entries
    +-1 (320 = 8 * 40); on free_1 \\ free_2: 10 A entries +-2 and 140 B entries +-1 (360 = 2 * 180).  Step k multiplies g_minor by 1/2 on A
    and by -1 on B, so before step k: sum_A gm^2 = 2 sum_B gm^2 over free_k — the first CG step is exactly 1/32 each time."""
    n = F.EXACT_N
    rng = np.random.default_rng(F.EXACT_SEED + 4)
    order = rng.permutation(n)
    take = lambda k: [order[:k], order[k:]]
    groups = {}
    for key, k in (("a3", 10), ("b3", 5), ("a2", 10), ("b2", 35), ("a1", 10), ("b1", 140)):
        groups[key], order = take(k)
    rest = order                                                     # 91 variables fixed throughout
    is_b = np.zeros(n, dtype=bool)
    for key in ("b3", "b2", "b1"):
        is_b[groups[key]] = True
    is_b[rest[::2]] = True
    J = F.exact_jacobian(n, n + 3)
    J[:, is_b] *= 2.0
    h = np.where(is_b, 64.0, 16.0)
    assert np.array_equal(J.T @ J, np.diag(h))
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    G = sign * rng.integers(1, 8, n)
    for key, mag in (("a3", 4.0), ("a2", 4.0), ("a1", 2.0), ("b3", 1.0), ("b2", 1.0), ("b1", 1.0)):
        G[groups[key]] = sign[groups[key]] * mag
    s0 = rng.integers(1, 9, n) / 16.0 * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = G - h * s0
    sets = []
    for keys in (("a3", "b3", "a2", "b2", "a1", "b1"), ("a3", "b3", "a2", "b2"), ("a3", "b3")):
        fix = np.ones(n, dtype=bool)
        for key in keys:
            fix[groups[key]] = False
        sets.append(fix)
    return n, J, h, sets, g, s0, is_b


def test_three_exact_steps_with_a_growing_active_set(bh, n_cu):
    n, J, h, sets, g, s0, is_b = _exact_chain()
    # the exact chain, in float64 (every value is a small dyadic rational)
    exact = []
    s, gm = s0.copy(), h * s0 + g
    for fix in sets:
        free = ~fix
        a, b = float(np.sum(gm[free & ~is_b] ** 2)), float(np.sum(gm[free & is_b] ** 2))
        assert a == 2.0 * b and b > 0.0
        w = np.where(free, -gm / 32.0, 0.0)
        s = s + w
        gm = h * s + g
        exact.append((w + 0.0, s.copy(), gm.copy(), float(g @ s) + 0.5 * float(np.sum(h * s * s))))
        assert np.all(gm[free] != 0.0)
    out = {}
    for key, (chain, sfc) in (("compact", (1, 1)), ("full", (0, 1)), ("sweep", (0, 0))):
        H = bh.AlHessian(J, None, F.MU)
        P = None
        ch = Chain(bh, H, n, s0, g)
        log = []
        try:
            _mode(bh, chain=chain, minor=0, sfc=sfc)
            assert np.array_equal(_bits(ch.get("gm")), _bits(h * s0 + g))
            for step, fix in enumerate(sets):
                if P is None:
                    P = _constraints(bh, n, fix.copy())
                else:
                    P.fixvars = fix.copy()
                got = ch.minor(P, kappa2=1.0e3)                       # (the loop stops after its first step: |r.v| < kappa2 |v_0|)
                assert got[1:4] == (int(R.CGStatus.solved), 2, 1) and got[4] == 1.0, (key, step, got[1:])
                d_hmul, d_jv = ch.accumulate()
                assert (d_hmul, d_jv) == ((1, 0) if key == "sweep" else (0, 0)), (key, step, d_hmul, d_jv)
                value, d_jv = ch.model()
                assert d_jv == (1 if key == "sweep" else 0), (key, step, d_jv)
                log.append((got[0], ch.get("s"), ch.get("gm"), value))
            info = H.free_image_info(None)
            assert info["calls_served"] == (3 if key == "compact" else 0) and info["builds"] == (1 if key == "compact" else 0), (key, info)
            out[key] = log
        finally:
            _restore(bh)
            ch.close()
            H.close()
            if P is not None:
                P.close()
    for key, log in out.items():
        for step, (fix, got, want) in enumerate(zip(sets, log, exact)):
            what = (key, "step", step + 1)
            assert np.array_equal(_bits(got[0]), _bits(want[0])), (what, "w")
            assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "s")
            assert np.array_equal(_bits(got[2][~fix]), _bits(want[2][~fix])), (what, "g_minor on the free variables")
            assert _bits(got[3]).tolist() == _bits(want[3]).tolist(), (what, "model reduction", got[3], want[3])
    # the compact chain's g_minor on the fixed variables is the one it had when they were last free (or H s0 + g)
    gm_start = h * s0 + g
    assert np.array_equal(_bits(out["compact"][2][2][sets[0]]), _bits(gm_start[sets[0]]))


# ------------------------------------------------------------------------------------------------------------- 5. bh.inner_step
def test_inner_step_under_the_option(bh, n_cu):
    d, n = INNER["d"], INNER["n"]
    J = R.synthetic_J(d, n, seed=INNER["seed"])
    inst = R.synthetic_box_vectors(d, n, fix_every=8)
    A = np.zeros((0, n))
    L0 = R.chol_lower(A @ A.T)
    g = J.T @ inst.r0
    delta = R.initial_tr(g)
    Ho = R.AlHessian(J, np.zeros((0, n)), 10.0)
    cons_o = R.make_mixed_constraints(A, L0, l=inst.x_l, u=inst.x_u)
    s_ref, pred_ref = R.inner_step(inst.x, g, Ho, L0, cons_o, delta, INNER["minor_steps"], INNER["kappa2"], INNER["kappa3"])
    out = {}
    try:
        for opt in (0, 1):
            _mode(bh, chain=opt, minor=0, sfc=0)                  # (inner_step switches step_from_cg on around its loop itself)
            H = bh.AlHessian(J, None, 10.0)
            P = bh.MixedConstraints(A, None, None, l=inst.x_l, u=inst.x_u)
            try:
                s, pred, info = bh.inner_step(inst.x, g, H, P, delta, INNER["minor_steps"], INNER["kappa2"], INNER["kappa3"], full_output=True)
                out[opt] = (s, pred, [(int(a), int(b), int(c)) for a, b, c, _ in info["minor"]], H.free_image_info(None), H.stats()["n_jv"],
                            P.fixvars.copy())
            finally:
                H.close()
                P.close()
        assert len(out[0][2]) == INNER["minor_steps"] and out[0][2] == out[1][2], (out[0][2], out[1][2])
        assert out[0][3]["calls_served"] == 0 and out[1][3]["calls_served"] >= 1, (out[0][3], out[1][3])
        assert out[0][4] == out[1][4], ("J v sweeps inside the chain", out[0][4], out[1][4])
        assert np.array_equal(out[0][5], out[1][5]) and np.array_equal(out[1][5], cons_o.fixvars)
        print("[inner_step free_image_chain=1] %s; minor iterates (status, iters, fixed): %s" % (out[1][3], out[1][2]))
        for opt in (0, 1):
            s, pred = out[opt][:2]
            assert relnorm(s, s_ref) <= 1e-6, (opt, relnorm(s, s_ref))
            _assert_model(pred, g, s, Ho, "inner_step, free_image_chain = %d, the explicit value at its own s" % opt)
            bound = 1e-10 * (np.linalg.norm(g) * np.linalg.norm(s_ref) + R.vthv(Ho, s_ref))
            print("[inner_step free_image_chain=%d] model reduction %r, R.inner_step %r: |difference| %.3e, bound %.3e" % (
                opt, pred, pred_ref, abs(pred - pred_ref), bound))
            note_tol(MR_LABEL, abs(pred - pred_ref), bound, "inner_step vs R.inner_step, free_image_chain = %d" % opt)
            assert abs(pred - pred_ref) <= bound, (opt, pred, pred_ref, bound)
    finally:
        _restore(bh)


# ---------------------------------------------------------------------------------------------------------- 6. a mixed chain
def test_a_mixed_chain_full_compact_full_carries_the_model_value(bh, n_cu):
    I = F.instance("S1", n_cu)
    n, g, Ho = I["n"], I["g"], I["Ho"]
    sts = F.states("S1")[3:6]                                       # widths 127, 113, 112: the active set grows between the iterates
    s0 = 0.01 * np.random.default_rng(5).standard_normal(n)
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    P = _constraints(bh, n, sts[0].fix.copy())
    ch = Chain(bh, H, n, s0, g)
    try:
        s_prev = s0
        for step, (st, fi) in enumerate(zip(sts, (0, 2, 0))):
            what = "mixed chain, iterate %d (free_image = %d, width %d)" % (step + 1, fi, st.width)
            if step > 0:
                P.fixvars = st.fix.copy()
            _mode(bh, chain=1, minor=0, sfc=1, free_image=fi)
            served = H.free_image_info(None)["calls_served"]
            got = ch.minor(P)
            assert H.free_image_info(None)["calls_served"] - served == (1 if fi == 2 else 0), what
            assert got[1] == int(R.CGStatus.solved) and np.any(got[0] != 0.0), (what, got[1:])
            assert ch.accumulate() == (0, 0), what
            s = ch.get("s")
            assert np.array_equal(_bits(s), _bits(s_prev + got[0])), what
            value, d_jv = ch.model()
            assert d_jv == 0, what
            _assert_model(value, g, s, Ho, what)
            _assert_free_part(ch.get("gm"), s, got[0], s_prev, g, I, st.fix, what)
            s_prev = s
    finally:
        _restore(bh)
        ch.close()
        H.close()
        P.close()


# ------------------------------------------------------------------------------------------------- 7. zero curvature in the chain
def _flat_direction_instance():
    """n, J (J'J = diag(16 on A, 0 on B)), h, the active set, g, s0: over the free variables G = H s0 + g has 24 A entries and 24 B
    entries, all +-1."""
    n = F.EXACT_N
    rng = np.random.default_rng(F.EXACT_SEED + 7)
    order = rng.permutation(n)
    fa, fb, rest = order[:24], order[24:48], order[48:]
    is_b = np.zeros(n, dtype=bool)
    is_b[fb] = True
    is_b[rest[::3]] = True
    J = F.exact_jacobian(n, n + 3)
    J[:, is_b] = 0.0
    h = np.where(is_b, 0.0, 16.0)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    G = sign * rng.integers(1, 8, n)
    G[fa], G[fb] = sign[fa], sign[fb]
    s0 = rng.integers(1, 9, n) / 16.0 * sign[::-1]
    fix = np.ones(n, dtype=bool)
    fix[fa] = fix[fb] = False
    return n, J, h, fix, G - h * s0, s0, is_b


def test_a_zero_curvature_iterate_in_the_chain_leaves_w_unscaled(bh, n_cu):
    n, J, h, fix, g, s0, is_b = _flat_direction_instance()
    gm0 = h * s0 + g
    w_exact = np.where(fix, 0.0, -gm0 / 8.0) + 0.0                   # the first CG step, 1/8; no line search follows
    s_exact = s0 + w_exact
    gm_exact = h * s_exact + g
    q_exact = float(g @ s_exact) + 0.5 * float(np.sum(h * s_exact * s_exact))
    Ho = R.AlHessian(J, np.zeros((0, n)), F.MU)
    out = {}
    for key, chain in (("compact", 1), ("full", 0)):
        H = bh.AlHessian(J, None, F.MU)
        P = _constraints(bh, n, fix.copy())
        ch = Chain(bh, H, n, s0, g)
        try:
            _mode(bh, chain=chain, minor=0, sfc=1)
            got = ch.minor(P)
            assert got[1:4] == (int(R.CGStatus.negative_curvature), 2, 2) and np.isnan(got[4]), (key, got[1:])
            assert H.free_image_info(None)["calls_served"] == chain
            assert np.array_equal(_bits(got[0]), _bits(w_exact)), (key, "w is not the unscaled first step")
            assert ch.accumulate() == (0, 0), key
            s1, gm1 = ch.get("s"), ch.get("gm")
            value, d_jv = ch.model()
            assert d_jv == 0, key
            out[key] = (s1, gm1, value)
            assert np.array_equal(_bits(s1), _bits(s_exact)), key
            assert np.array_equal(_bits(gm1[~fix]), _bits(gm_exact[~fix])), key
            assert np.array_equal(_bits(gm1[fix]), _bits(gm0[fix])), key            # (J'J is diagonal: stale or not, the same numbers)
            assert _bits(value).tolist() == _bits(q_exact).tolist(), (key, value, q_exact)
            _assert_model(value, g, s1, Ho, "zero curvature, %s" % key)
        finally:
            _restore(bh)
            ch.close()
            H.close()
            P.close()


# ------------------------------------------------------------------------------------------------------------------ 8. hygiene
def _disturbed_accumulate(bh, n_cu, disturbance, compact):
    """compact: the chain under test runs on the compact image (free_image_chain = 1) against the compact step_from_cg = 0 chain
    (free_image_minor = 1); otherwise both run on the full image (free_image_chain = 0, free_image_minor = 0)."""
    I = F.instance("S3", n_cu)                                      # n == ld: bh_pcg_dev takes device vectors in place
    st = F.states("S3")[0]
    n, g, Ho = I["n"], I["g"], I["Ho"]
    s0 = 0.01 * np.random.default_rng(41).standard_normal(n)
    steps = 2 if disturbance == "second_accumulate" else 1
    out = {}
    # reference: the step_from_cg = 0 chain on the same image
    for key, (chain, minor, sfc) in (("reference", (0, int(compact), 0)), ("disturbed", (int(compact), 0, 1))):
        H = bh.AlHessian(I["J"], I["C"], F.MU)
        P = _constraints(bh, n, st.fix.copy())
        ch = Chain(bh, H, n, s0, g)
        extra = []
        try:
            _mode(bh, chain=chain, minor=minor, sfc=sfc)
            got = ch.minor(P)
            assert H.free_image_info(None)["calls_served"] == int(compact)
            w_arg = None
            if key == "disturbed" and disturbance == "pcg":
                big = 1e6 * np.ones(n)
                extra = [bh.DeviceVector(n, a) for a in (g, -big, big, np.zeros(n))]
                bh.projected_cg_dev(extra[0], H, extra[1], extra[2], P, 0.1, extra[3])
            elif key == "disturbed" and disturbance == "other_handle":
                I5 = F.instance("S5", n_cu)
                H2 = bh.AlHessian(I5["J"], I5["C"], F.MU)
                P2 = _constraints(bh, I5["n"], F.states("S5")[1].fix.copy())
                ch2 = Chain(bh, H2, I5["n"], np.zeros(I5["n"]), I5["g"])
                try:
                    ch2.minor(P2)
                finally:
                    ch2.close()
                    H2.close()
                    P2.close()
            elif key == "disturbed" and disturbance == "other_w":
                extra = [bh.DeviceVector(n, got[0])]
                w_arg = extra[0]
            elif key == "disturbed" and disturbance == "set_mu":
                H.mu = 2 * F.MU                                     # cg.hw, cg.hwc, g_minor and the carried q are of another operator now ...
                H.mu = F.MU                                         # ... and the library does not look whether it comes back
            sweeps = [ch.accumulate(w_arg) for _ in range(steps)]
            if key == "reference":
                assert sweeps == [(1, 0)] * steps
            elif disturbance == "second_accumulate":
                assert sweeps == [(0, 0), (1, 0)], sweeps          # the first one is the chain's, the second another step
            else:
                assert sweeps == [(1, 0)], sweeps
            s1, gm1 = ch.get("s"), ch.get("gm")
            value, d_jv = ch.model()
            assert d_jv == (0 if sfc else 1)                       # after a sweep g_minor is whole again: s.(g_minor - g) will do
            _assert_model(value, g, s1, Ho, "%s, %s" % (disturbance, key))
            out[key] = (got, s1, gm1)
        finally:
            _restore(bh)
            ch.close()
            for a in extra:
                a.close()
            H.close()
            P.close()
    _same_call(out["disturbed"][0], out["reference"][0], disturbance)
    assert np.array_equal(_bits(out["disturbed"][1]), _bits(out["reference"][1])), (disturbance, "s")
    assert np.array_equal(_bits(out["disturbed"][2]), _bits(out["reference"][2])), (disturbance, "g_minor")


@pytest.mark.parametrize("disturbance", ["pcg", "other_handle", "other_w", "second_accumulate", "set_mu"])
def test_anything_between_the_minor_iterate_and_the_accumulate_sends_it_down_the_sweep(bh, n_cu, disturbance):
    _disturbed_accumulate(bh, n_cu, disturbance, compact=True)


def test_a_changed_mu_sends_the_full_image_chain_down_the_sweep_too(bh, n_cu):
    """free_image_chain = 0, free_image_minor = 0, step_from_cg = 1: cg.hw is H*w of the old mu as much as cg.hwc is.  (A library that
    clears the compact note alone takes the two vector launches here: [(0, 0)].)"""
    _disturbed_accumulate(bh, n_cu, "set_mu", compact=False)


def test_a_changed_mu_sends_the_model_value_back_to_the_sweep(bh, n_cu):
    """bh_hmul_add_dev notes g_minor = H*s + g; with another mu that g_minor is no longer of this H, and s.(g_minor - g) no longer s'Hs."""
    I = F.instance("S3", n_cu)
    n, g = I["n"], I["g"]
    s0 = 0.01 * np.random.default_rng(43).standard_normal(n)
    H = bh.AlHessian(I["J"], I["C"], F.MU)
    ch = Chain(bh, H, n, s0, g)                                     # (bh_hmul_add_dev(H, s, g, gm))
    try:
        _mode(bh, chain=0, minor=0, sfc=1)
        H.mu = 2 * F.MU
        value, d_jv = ch.model()
        assert d_jv == 1
        _assert_model(value, g, s0, R.AlHessian(I["J"], I["C"], 2 * F.MU), "model value after set_mu(2 mu)")
    finally:
        _restore(bh)
        ch.close()
        H.close()
