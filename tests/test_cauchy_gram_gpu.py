"""GPU tests of the one-launch Cauchy search on a Gram-form handle (option cauchy_gram, cauchy_gram_kernel):
the whole box-constrained search of src/basic_tralcnlss.jl:574-639 from G = J'J + mu C'C — Hd downdated by one row of G per breakpoint,
the loop on the device — against hand-derived answers, the oracle, and the device's own other forms."""
import numpy as np
import pytest

import benlsip_ref as R
from _util import closed_form_cauchy_cases, note_tol, relnorm
from hip_ops import HipOpsResident

pytestmark = pytest.mark.gpu

FORM_HD, FORM_ROWSPACE, FORM_ROWSPACE_EQ, FORM_GRAM = 0, 1, 2, 3


def _gram(bh, J, C=None, mu=0.0):
    H = bh.AlHessian(J, C, mu)
    H.set_form("gram")
    return H


def _instance(d, n, q, nact, delta_factor, seed, jscale=1.0, colscale=None):
    """The generator of test_cauchy_step_in_the_row_space_of_j (same order of draws); delta = delta_factor * ||g||."""
    rng = np.random.default_rng(seed)
    J = jscale * rng.standard_normal((d, n)) / np.sqrt(d)
    C = rng.standard_normal((q, n))
    xlow, xupp = -np.ones(n), np.ones(n)
    x = np.clip(0.5 * rng.standard_normal(n), -0.95, 0.95)
    act = rng.choice(n, nact, replace=False)
    x[act] = np.where(rng.random(nact) < 0.5, -1.0, 1.0)
    g = rng.standard_normal(n)
    if colscale is not None:
        J = J * colscale[None, :]
    return J, C, xlow, xupp, x, g, delta_factor * float(np.linalg.norm(g))


def _oracle(J, C, mu, xlow, xupp, x, g, delta, A=None):
    n = x.shape[0]
    A = np.zeros((0, n)) if A is None else A
    L0 = R.chol_lower(A @ A.T)
    Ho = R.AlHessian(J, C, mu)
    cons_o = R.make_mixed_constraints(A, L0, l=xlow, u=xupp)
    calls = [0]

    class Ops(R.NumpyOps):
        def hmul(self, H, v):
            calls[0] += 1
            return R.hmul(H, v)
    s_ref = R.cauchy_step(x, g, Ho, L0, cons_o, delta, Ops())
    return s_ref, np.asarray(cons_o.fixvars, dtype=bool).copy(), calls[0]


def _search(bh, H, A, xlow, xupp, x, g, delta, gram):
    """One search on a fresh constraint handle with cauchy_gram = `gram`; the option is back at 0 afterwards."""
    bh.set_option("cauchy_gram", gram)
    try:
        cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
        s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
        fix = np.asarray(cons.fixvars, dtype=bool).copy()
        cons.close()
    finally:
        bh.set_option("cauchy_gram", 0)
    return s, fix, info


# ------------------------------------------------------------------------------------------------------------ 1. hand-derived
def test_closed_form_cases_from_g(bh):
    """closed_form_cauchy_cases (H = I in two variables, dyadic data): step bit for bit, active set, number of passes."""
    Z = np.zeros((0, 2))
    for case in closed_form_cauchy_cases():
        H = _gram(bh, np.eye(2), None, 0.0)
        s, fix, info = _search(bh, H, Z, -np.ones(2), np.ones(2), np.zeros(2), case["g"], case["delta"], 1)
        assert info["form"] == FORM_GRAM, (case["name"], info)
        assert np.array_equal(s, case["s"]), (case["name"], s, case["s"])
        assert np.array_equal(fix, case["fix"]), (case["name"], fix)
        assert info["n_hmul"] == case["n_hmul"], (case["name"], info)
        H.close()


# ------------------------------------------------------------------------------------------------------------ 2. the oracle
# d, n, q, nact, delta / ||g||, seed, scale of J, column scaling over three decades
ORACLE_CASES = [(90, 33, 2, 3, 0.1, 11, 1.0, False), (700, 257, 1, 20, 0.3, 12, 1.0, False), (3000, 1024, 0, 100, 1.0, 13, 1.0, False),
                (257, 4100, 3, 50, 0.1, 14, 1.0, False), (5, 3, 1, 0, 0.5, 15, 1.0, False),
                (1, 1, 0, 0, 0.1, 16, 1.0, False), (37, 5, 2, 1, 0.1, 17, 1.0, False), (2000, 512, 0, 40, 0.2, 5, 1.0, False),
                (400, 150, 1, 10, 0.3, 18, 1.0, True),
                (300, 8200, 2, 100, 0.005, 21, 3.0, False)]


@pytest.mark.parametrize("d,n,q,nact,dfac,seed,jscale,scaled", ORACLE_CASES)
def test_against_the_oracle(bh, d, n, q, nact, dfac, seed, jscale, scaled):
    """Same final active set, passes = the oracle's H*d products, step within 1e-9, feasible, form 3, ONE product
    (the G d at the start) and one build of G."""
    colscale = np.logspace(0.0, -3.0, n) if scaled else None
    J, C, xlow, xupp, x, g, delta = _instance(d, n, q, nact, dfac, seed, jscale, colscale)
    mu = 2.5
    s_ref, fix_ref, n_hd = _oracle(J, C, mu, xlow, xupp, x, g, delta)
    H = _gram(bh, J, C, mu)
    n0 = H.stats()["n_hmul"]
    s, fix, info = _search(bh, H, np.zeros((0, n)), xlow, xupp, x, g, delta, 1)
    assert info["form"] == FORM_GRAM, info
    assert np.array_equal(fix, fix_ref), (np.flatnonzero(fix), np.flatnonzero(fix_ref))
    assert info["n_hmul"] == n_hd, (info, n_hd)
    rel = relnorm(s, s_ref)
    note_tol("cauchy_step from G in one launch: step vs oracle, 1e-9", rel, 1e-9, "d=%d n=%d q=%d, %d breakpoints" % (d, n, q, info["n_breakpoints"]))
    assert rel <= 1e-9, rel
    assert np.all(x + s <= xupp + 1e-12) and np.all(x + s >= xlow - 1e-12) and np.max(np.abs(s)) <= delta * (1 + 1e-12)
    assert H.stats()["n_hmul"] - n0 == 1
    assert H.gram_builds == 1
    H.close()


def test_wide_instance_has_the_expected_length(bh):
    """The n = 8200 instance (the streamed shape of the kernel, n > 4096) takes 178 breakpoints, as in the oracle."""
    d, n, q, nact, dfac, seed, jscale, _ = ORACLE_CASES[-1]
    J, C, xlow, xupp, x, g, delta = _instance(d, n, q, nact, dfac, seed, jscale)
    H = _gram(bh, J, C, 2.5)
    _, _, info = _search(bh, H, np.zeros((0, n)), xlow, xupp, x, g, delta, 1)
    assert info["n_breakpoints"] == 178, info
    H.close()


# ------------------------------------------------------------------------------------------------------------ 3. launch count
def test_launch_count_does_not_depend_on_the_search_length(bh):
    J, C, xlow, xupp, x, g, _ = _instance(3000, 1024, 0, 100, 1.0, 13)
    Z = np.zeros((0, 1024))
    H = _gram(bh, J, C, 2.5)
    gn = float(np.linalg.norm(g))
    _search(bh, H, Z, xlow, xupp, x, g, 0.1 * gn, 1)                 # the build of G is behind us
    on = [_search(bh, H, Z, xlow, xupp, x, g, f * gn, 1)[2] for f in (0.005, 1.0)]
    off = [_search(bh, H, Z, xlow, xupp, x, g, f * gn, 0)[2] for f in (0.005, 1.0)]
    assert abs(on[0]["n_breakpoints"] - on[1]["n_breakpoints"]) > 10, on
    assert on[0]["form"] == on[1]["form"] == FORM_GRAM
    assert on[0]["n_launches"] == on[1]["n_launches"] < 16, on
    for a, b in zip(on, off):
        assert b["form"] == FORM_ROWSPACE and b["n_breakpoints"] == a["n_breakpoints"], (a, b)
        assert b["n_launches"] > b["n_breakpoints"], b
    H.close()


# ------------------------------------------------------------------------------------------------------------ 4. the forms agree
@pytest.mark.parametrize("case", [2, 3])
def test_forms_agree_on_one_gram_handle_and_the_search_is_reproducible(bh, case):
    d, n, q, nact, dfac, seed, jscale, _ = ORACLE_CASES[case]
    J, C, xlow, xupp, x, g, delta = _instance(d, n, q, nact, dfac, seed, jscale)
    Z = np.zeros((0, n))
    H = _gram(bh, J, C, 2.5)
    s1, f1, i1 = _search(bh, H, Z, xlow, xupp, x, g, delta, 1)
    s0, f0, i0 = _search(bh, H, Z, xlow, xupp, x, g, delta, 0)
    s2, f2, i2 = _search(bh, H, Z, xlow, xupp, x, g, delta, 1)
    assert (i1["form"], i0["form"]) == (FORM_GRAM, FORM_ROWSPACE)
    assert (i1["n_breakpoints"], i1["n_hmul"]) == (i0["n_breakpoints"], i0["n_hmul"]) and np.array_equal(f1, f0), (i1, i0)
    rel = relnorm(s1, s0)
    note_tol("cauchy_step from G vs row space of J on one handle, 1e-9", rel, 1e-9, "n=%d, %d breakpoints" % (n, i1["n_breakpoints"]))
    assert rel <= 1e-9, rel
    assert np.array_equal(s2, s1) and np.array_equal(f2, f1) and i2["n_hmul"] == i1["n_hmul"]
    H.close()


# ------------------------------------------------------------------------------------------------------------ 5. fall-backs
@pytest.mark.parametrize("gram_handle,mA,form", [(False, 0, FORM_ROWSPACE), (True, 3, FORM_ROWSPACE_EQ), (True, 96, FORM_HD)])
def test_fall_backs_are_silent_and_exact(bh, gram_handle, mA, form):
    """Implicit handle, or linear equalities: the option changes nothing — same form as without it, step and active set bit for bit."""
    n = 200
    J, C, xlow, xupp, x, g, delta = _instance(500, n, 1, 10, 0.3, 31 + mA)
    A = np.random.default_rng(7).standard_normal((mA, n))
    if mA:
        x = x - A.T @ np.linalg.solve(A @ A.T, A @ x)
        x = np.clip(x, -0.95, 0.95)
    H = _gram(bh, J, C, 2.5) if gram_handle else bh.AlHessian(J, C, 2.5)
    s0, f0, i0 = _search(bh, H, A, xlow, xupp, x, g, delta, 0)
    s1, f1, i1 = _search(bh, H, A, xlow, xupp, x, g, delta, 1)
    assert i0["form"] == form and i1["form"] == form, (i0, i1)
    assert np.array_equal(s1, s0) and np.array_equal(f1, f0)
    assert (i1["n_breakpoints"], i1["n_hmul"]) == (i0["n_breakpoints"], i0["n_hmul"])
    H.close()


# ------------------------------------------------------------------------------------------------------------ 6. stale G
@pytest.mark.parametrize("asynchronous", [False, True])
def test_stale_g_is_rebuilt_before_the_search(bh, asynchronous):
    d, n, q = 700, 257, 1
    J, C, xlow, xupp, x, g, delta = _instance(d, n, q, 20, 0.3, 12)
    Z = np.zeros((0, n))
    if asynchronous:
        H = bh.AlHessian.create_async(J, C, 2.5)                  # no wait: the build of G is ordered behind the upload
        H.set_form("gram")
    else:
        H = _gram(bh, J, C, 2.5)
    s, fix, info = _search(bh, H, Z, xlow, xupp, x, g, delta, 1)
    s_ref, fix_ref, n_hd = _oracle(J, C, 2.5, xlow, xupp, x, g, delta)
    assert info["form"] == FORM_GRAM and H.gram_builds == 1
    assert np.array_equal(fix, fix_ref) and info["n_hmul"] == n_hd
    note_tol("cauchy_step from G in one launch: step vs oracle, 1e-9", relnorm(s, s_ref), 1e-9, "first mu%s" % (", async ingest" if asynchronous else ""))
    assert relnorm(s, s_ref) <= 1e-9
    H.mu = 40.0
    s, fix, info = _search(bh, H, Z, xlow, xupp, x, g, delta, 1)
    s_ref, fix_ref, n_hd = _oracle(J, C, 40.0, xlow, xupp, x, g, delta)
    assert info["form"] == FORM_GRAM and H.gram_builds == 2
    assert np.array_equal(fix, fix_ref) and info["n_hmul"] == n_hd
    note_tol("cauchy_step from G in one launch: step vs oracle, 1e-9", relnorm(s, s_ref), 1e-9, "new mu%s" % (", async ingest" if asynchronous else ""))
    assert relnorm(s, s_ref) <= 1e-9
    H.close()


# ------------------------------------------------------------------------------------------------------------ 7. resident chain
class _GramResident(HipOpsResident):
    def new_hessian(self, J, C, mu):
        H = self.bh.AlHessian(J, C, mu)
        H.set_form("gram")
        return H


def test_resident_inner_step_takes_the_one_launch_search(bh):
    """bh.inner_step (box constraints) on a Gram-form handle with the option on against the oracle's inner_step, under the rule of
    test_inner_step_device_chain_against_oracle; the PCIe bytes of the loop are those of the option-off run."""
    d, n = 4096, 512
    J = R.synthetic_J(d, n, seed=1)
    inst = R.synthetic_box_vectors(d, n, fix_every=8)
    A = np.zeros((0, n))
    L0 = R.chol_lower(A @ A.T)
    x = np.clip(inst.x, inst.x_l, inst.x_u)
    g = J.T @ inst.r0
    delta = R.initial_tr(g)

    def run(ops):
        cons = R.make_mixed_constraints(A, L0, l=inst.x_l, u=inst.x_u)
        H = ops.new_hessian(J, np.zeros((0, n)), 10.0)
        log = []
        if hasattr(ops, "inner_step"):
            s, pred = ops.inner_step(x, g, H, L0, cons, delta, 50, 0.1, 0.1, log)
            form = bh.cauchy_info(cons._dev)[0]
        else:
            s, pred = R.inner_step(x, g, H, L0, cons, delta, 50, 0.1, 0.1, ops=ops, log=log)
            form = None
        return s, pred, log, cons.fixvars.copy(), form

    s_ref, pred_ref, log_ref, fix_ref, _ = run(R.NumpyOps())
    off = _GramResident(bh)
    s_off, pred_off, log_off, fix_off, form_off = run(off)
    on = _GramResident(bh)
    bh.set_option("cauchy_gram", 1)
    try:
        s_on, pred_on, log_on, fix_on, form_on = run(on)
    finally:
        bh.set_option("cauchy_gram", 0)
    assert (form_off, form_on) == (FORM_ROWSPACE, FORM_GRAM)
    assert [e[1] for e in log_on] == [e[1] for e in log_ref]
    assert [e[2] for e in log_on] == [e[2] for e in log_ref]
    assert np.array_equal(fix_on, fix_ref)
    note_tol("inner_step with the one-launch Cauchy search: s vs oracle, 1e-6", relnorm(s_on, s_ref), 1e-6)
    assert relnorm(s_on, s_ref) <= 1e-6, relnorm(s_on, s_ref)
    assert pred_on == pytest.approx(pred_ref, rel=1e-8)
    assert on.loop_minor == off.loop_minor and on.loop_bytes == off.loop_bytes, (on.loop_bytes, off.loop_bytes)


# ------------------------------------------------------------------------------------------------------------ 8. error path
def test_no_breakpoint_left_returns_the_same_code_in_both_forms(bh):
    """One NaN in g (n = 6): the search runs out of breakpoints.  Device against device: the same return code with the option on and
    off — and the call returns (the device loop is bounded by n + 1 passes)."""
    n = 6
    rng = np.random.default_rng(3)
    J = rng.standard_normal((20, n)) / np.sqrt(20.0)
    g = rng.standard_normal(n)
    g[2] = np.nan
    x, xlow, xupp = np.zeros(n), -np.ones(n), np.ones(n)
    H = _gram(bh, J, None, 0.0)
    codes = []
    for gram in (0, 1):
        try:
            _search(bh, H, np.zeros((0, n)), xlow, xupp, x, g, 10.0, gram)
            codes.append(0)
        except bh.BenlsipHipError as e:
            codes.append(e.code)
    assert codes[0] == codes[1], codes
    H.close()


# ------------------------------------------------------------------------------------------------------------ 9. config-3 scale
def test_config3_scale_against_the_sweeping_form(bh, capsys):
    """Synthetic 65536 x 4096, the three radii of tools/cauchy_gram_timing.py: the one-launch search against the sweeping form
    (cauchy_image = 0: one H*d per breakpoint) on the same Gram-form handle."""
    syn = bh.synthetic
    d, n = 65536, 4096
    H = bh.AlHessian.synthetic(d, n, seed=1, mu=10.0)
    x, x_l, x_u, fix = syn.box_vectors(n, fix_every=8)
    g = H.jtv(syn.residual_rows(0, d))
    H.set_form("gram")
    Z = np.zeros((0, n))
    for dscale in (0.1, 1.0, 10.0):
        delta = dscale * syn.initial_tr(g)
        s1, f1, i1 = _search(bh, H, Z, x_l, x_u, x, g, delta, 1)
        bh.set_option("cauchy_image", 0)
        try:
            s0, f0, i0 = _search(bh, H, Z, x_l, x_u, x, g, delta, 0)
        finally:
            bh.set_option("cauchy_image", 1)
        with capsys.disabled():
            print("[Cauchy search from G at config-3 scale, delta = %.3g] %d breakpoints, %d passes, %d active bounds, %d launches (sweeping form: %d)"
                  % (delta, i1["n_breakpoints"], i1["n_hmul"], int(f1.sum()), i1["n_launches"], i0["n_launches"]))
        assert (i1["form"], i0["form"]) == (FORM_GRAM, FORM_HD)
        assert i0["n_breakpoints"] > 1000
        assert (i1["n_breakpoints"], i1["n_hmul"]) == (i0["n_breakpoints"], i0["n_hmul"]) and np.array_equal(f1, f0), (i1, i0, int((f1 != f0).sum()))
        rel = relnorm(s1, s0)
        note_tol("cauchy_step from G at config-3 scale vs the sweeping form, 1e-9", rel, 1e-9, "delta=%.3g, %d breakpoints" % (delta, i1["n_breakpoints"]))
        assert rel <= 1e-9, rel
        model = float(g @ s1 + 0.5 * (s1 @ (H * s1)))
        assert model < 0.0
    H.close()
