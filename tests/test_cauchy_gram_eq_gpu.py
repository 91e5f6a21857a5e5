"""GPU tests of the Cauchy search with linear equalities on a Gram-form handle (option cauchy_gram_eq, cauchy_gram_eq_kernel,
bh_cauchy_info form 4): the search of src/basic_tralcnlss.jl:574-639 with Hd = G d = -a - B y kept in the column
space of G = J'J + mu C'C (a = G D g, B = G D A', one row of G per breakpoint, formed again every kCauchyGramEqRefresh-th pass) —
against the oracle and against the device's own other forms.  Tolerances: SURVEY §8c, test_cauchy_step_parity."""
import functools
import os
import re

import numpy as np
import pytest

import benlsip_ref as R
from _util import note_tol, relnorm
from hip_ops import HipOpsResident

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_HD, FORM_ROWSPACE, FORM_ROWSPACE_EQ, FORM_GRAM, FORM_GRAM_EQ = 0, 1, 2, 3, 4
MU = 2.5


def _refresh_interval():
    src = open(os.path.join(ROOT, "benlsip.jl_amd", "csrc", "bh_api.hip")).read()
    return int(re.search(r"constexpr int kCauchyGramEqRefresh = (\d+);", src).group(1))


INTERVAL = _refresh_interval()


def _gram(bh, J, C=None, mu=0.0):
    H = bh.AlHessian(J, C, mu)
    H.set_form("gram")
    return H


def _instance(d, n, q, mA, nact, f, seed, scaled):
    """J, C, A, bounds +-1, x with nact active bounds, g, delta = f ||g|| (this order of draws)."""
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((d, n)) / np.sqrt(d)
    C = rng.standard_normal((q, n))
    A = rng.standard_normal((mA, n))
    xlow, xupp = -np.ones(n), np.ones(n)
    x = np.clip(0.5 * rng.standard_normal(n), -0.95, 0.95)
    act = rng.choice(n, nact, replace=False)
    x[act] = np.where(rng.random(nact) < 0.5, -1.0, 1.0)
    g = rng.standard_normal(n)
    if scaled:
        J = J * np.logspace(0.0, -3.0, n)[None, :]
    return J, C, A, xlow, xupp, x, g, f * float(np.linalg.norm(g))


def _oracle(J, C, A, mu, xlow, xupp, x, g, delta):
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


@functools.lru_cache(maxsize=None)
def _case(case):
    """Instance and oracle answer of one row of ORACLE_CASES, computed once per session (read-only for every test)."""
    inst = _instance(*case)
    J, C, A, xlow, xupp, x, g, delta = inst
    ref = _oracle(J, C, A, MU, xlow, xupp, x, g, delta)
    for arr in inst[:-1] + ref[:2]:
        arr.setflags(write=False)
    return inst, ref


def _search(bh, H, A, xlow, xupp, x, g, delta, eq, gram=0):
    """One search on a fresh constraint handle with cauchy_gram_eq = `eq` (and cauchy_gram = `gram`); both options are back at 0
    afterwards."""
    bh.set_option("cauchy_gram_eq", eq)
    bh.set_option("cauchy_gram", gram)
    try:
        cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
        s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
        fix = np.asarray(cons.fixvars, dtype=bool).copy()
        cons.close()
    finally:
        bh.set_option("cauchy_gram", 0)
        bh.set_option("cauchy_gram_eq", 0)
    return s, fix, info


def _gv_launches(passes):
    """G v launches of a form-4 search: the set-up and one per formation of a, B every INTERVAL-th pass."""
    return 1 + (passes - 1) // INTERVAL


# ------------------------------------------------------------------------------------------------------------ 1. the oracle
# d, n, q, mA, nact, delta / ||g||, seed, three decades of column scaling        -> passes of the oracle
ORACLE_CASES = [(90, 33, 2, 1, 3, 0.3, 41, False),          # 5: mA = 1, n below one tile, q > 0
                (300, 120, 0, 3, 10, 0.3, 42, False),       # 44
                (600, 270, 0, 16, 12, 0.5, 44, False),      # 89: mA = 16, n just above a padding boundary
                (900, 300, 0, 64, 12, 0.5, 46, False),      # 96: mA = 64
                (400, 1030, 1, 33, 30, 0.1, 47, False),     # 196: n > d (singular J'J), odd mA, crosses the re-formation interval
                (400, 150, 1, 4, 10, 0.3, 49, True),        # 67: three decades of column scaling
                (800, 400, 0, 8, 20, 0.3, 50, True),        # 346: scaled, hundreds of updates
                (70, 66, 0, 64, 0, 0.5, 51, False),         # 1: n - mA = 2, the loop ends at once
                (600, 260, 0, 8, 12, 0.5, 43, False),       # 78: mA = 8, one column per column group
                (500, 200, 0, 17, 10, 0.5, 45, False),      # 56: mA = 17, the first size with two columns per column group
                (300, 4100, 10, 5, 50, 0.3, 48, False)]     # 21: n > 4096
ORACLE_PASSES = [5, 44, 89, 96, 196, 67, 346, 1, 78, 56, 21]
CASE_N1030, CASE_N400 = ORACLE_CASES[4], ORACLE_CASES[6]


@pytest.mark.parametrize("case,passes", list(zip(ORACLE_CASES, ORACLE_PASSES)))
def test_against_the_oracle(bh, case, passes):
    """Same final active set, passes = the oracle's H*d products, step within 1e-9, box and trust region to 1e-12,
    ||A s|| <= 1e-10 ||A|| ||s||; form 4; the handle counts the G v launches (not the passes), no J v, one build of G."""
    (J, C, A, xlow, xupp, x, g, delta), (s_ref, fix_ref, n_hd) = _case(case)
    d, n, q, mA = case[:4]
    assert n_hd == passes, (n_hd, passes)                      # the instance is the one the table describes
    H = _gram(bh, J, C, MU)
    st0 = H.stats()
    s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, 1)
    st1 = H.stats()
    assert info["form"] == FORM_GRAM_EQ, info
    assert np.array_equal(fix, fix_ref), (np.flatnonzero(fix), np.flatnonzero(fix_ref))
    assert info["n_hmul"] == n_hd, (info, n_hd)
    rel = relnorm(s, s_ref)
    note_tol("cauchy_step from G with equalities: step vs oracle, 1e-9", rel, 1e-9, "d=%d n=%d q=%d mA=%d, %d passes" % (d, n, q, mA, n_hd))
    assert rel <= 1e-9, rel
    assert np.all(x + s <= xupp + 1e-12) and np.all(x + s >= xlow - 1e-12) and np.max(np.abs(s)) <= delta * (1 + 1e-12)
    feas = float(np.linalg.norm(A @ s))
    note_tol("cauchy_step from G with equalities: ||A s||, 1e-10 ||A|| ||s||", feas, 1e-10 * np.linalg.norm(A) * max(np.linalg.norm(s), 1e-300),
             "n=%d mA=%d" % (n, mA))
    assert feas <= 1e-10 * np.linalg.norm(A) * max(np.linalg.norm(s), 1e-300)
    assert st1["n_hmul"] - st0["n_hmul"] == _gv_launches(n_hd), (st0, st1)
    assert st1["n_jv"] == st0["n_jv"]
    assert H.gram_builds == 1
    H.close()


# ------------------------------------------------------------------------------------------------------------ 2. re-formation
@pytest.mark.parametrize("case", [CASE_N1030, CASE_N400])
def test_a_and_b_are_formed_again_inside_a_long_search(bh, case):
    """196 and 346 passes: a, B are formed once at the start and once per INTERVAL passes — the handle counts those G v launches
    (and G is built once, also when the search is repeated)."""
    (J, C, A, xlow, xupp, x, g, delta), (s_ref, fix_ref, n_hd) = _case(case)
    assert n_hd > INTERVAL, "the instance no longer crosses the re-formation interval: add a longer one"
    H = _gram(bh, J, C, MU)
    for rep in range(2):
        n0 = H.stats()["n_hmul"]
        s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, 1)
        assert info["form"] == FORM_GRAM_EQ and info["n_hmul"] == n_hd
        assert H.stats()["n_hmul"] - n0 == 1 + (n_hd - 1) // INTERVAL >= 2
        assert np.array_equal(fix, fix_ref) and relnorm(s, s_ref) <= 1e-9
    assert H.gram_builds == 1
    H.close()


# ------------------------------------------------------------------------------------------------------------ 3. the forms agree
@pytest.mark.parametrize("case", [ORACLE_CASES[1], ORACLE_CASES[2], CASE_N1030])
def test_forms_agree_on_one_gram_handle_and_the_search_is_reproducible(bh, case):
    (J, C, A, xlow, xupp, x, g, delta), _ = _case(case)
    n, mA = case[1], case[3]
    H = _gram(bh, J, C, MU)
    s4, f4, i4 = _search(bh, H, A, xlow, xupp, x, g, delta, 1)
    s2, f2, i2 = _search(bh, H, A, xlow, xupp, x, g, delta, 0)
    bh.set_option("cauchy_image", 0)
    try:
        s0, f0, i0 = _search(bh, H, A, xlow, xupp, x, g, delta, 0)
    finally:
        bh.set_option("cauchy_image", 1)
    s4b, f4b, i4b = _search(bh, H, A, xlow, xupp, x, g, delta, 1)
    assert (i4["form"], i2["form"], i0["form"], i4b["form"]) == (FORM_GRAM_EQ, FORM_ROWSPACE_EQ, FORM_HD, FORM_GRAM_EQ)
    for name, so, fo, io in (("row space of J", s2, f2, i2), ("one H*d per breakpoint", s0, f0, i0)):
        assert (i4["n_breakpoints"], i4["n_hmul"]) == (io["n_breakpoints"], io["n_hmul"]) and np.array_equal(f4, fo), (name, i4, io)
        rel = relnorm(s4, so)
        note_tol("cauchy_step from G with equalities vs the device's other forms, 1e-9", rel, 1e-9, "%s, n=%d mA=%d" % (name, n, mA))
        assert rel <= 1e-9, (name, rel)
    assert np.array_equal(s4b, s4) and np.array_equal(f4b, f4) and (i4b["n_breakpoints"], i4b["n_hmul"]) == (i4["n_breakpoints"], i4["n_hmul"])
    H.close()


# ------------------------------------------------------------------------------------------------------------ 4. fall-backs
@pytest.mark.parametrize("gram_handle,mA,gram,form", [(False, 3, 0, FORM_ROWSPACE_EQ), (True, 0, 0, FORM_ROWSPACE), (True, 65, 0, FORM_HD),
                                                      (True, 96, 0, FORM_HD), (True, 0, 1, FORM_GRAM)])
def test_fall_backs_are_silent_and_exact(bh, gram_handle, mA, gram, form):
    """Implicit handle, no equalities, more than 64 of them, cauchy_gram = 1 without equalities: the option changes nothing — same
    form as without it, step and active set bit for bit, the same counts."""
    n = 200
    J, C, _, xlow, xupp, x, g, delta = _instance(500, n, 1, 0, 10, 0.3, 31 + mA, False)
    A = np.random.default_rng(7).standard_normal((mA, n))
    H = _gram(bh, J, C, MU) if gram_handle else bh.AlHessian(J, C, MU)
    s0, f0, i0 = _search(bh, H, A, xlow, xupp, x, g, delta, 0, gram)
    s1, f1, i1 = _search(bh, H, A, xlow, xupp, x, g, delta, 1, gram)
    assert i0["form"] == form and i1["form"] == form, (i0, i1)
    assert np.array_equal(s1, s0) and np.array_equal(f1, f0)
    assert (i1["n_breakpoints"], i1["n_hmul"]) == (i0["n_breakpoints"], i0["n_hmul"])
    H.close()


# ------------------------------------------------------------------------------------------------------------ 5. stale G
@pytest.mark.parametrize("asynchronous", [False, True])
def test_stale_g_is_rebuilt_before_the_search(bh, asynchronous):
    case = ORACLE_CASES[5]                                       # q = 1: G depends on mu
    (J, C, A, xlow, xupp, x, g, delta), (s_ref, fix_ref, n_hd) = _case(case)
    if asynchronous:
        H = bh.AlHessian.create_async(J, C, MU)                  # no wait: the build of G is ordered behind the upload
        H.set_form("gram")
    else:
        H = _gram(bh, J, C, MU)
    s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, 1)
    assert info["form"] == FORM_GRAM_EQ and H.gram_builds == 1
    assert np.array_equal(fix, fix_ref) and info["n_hmul"] == n_hd
    note_tol("cauchy_step from G with equalities: step vs oracle, 1e-9", relnorm(s, s_ref), 1e-9, "first mu%s" % (", async ingest" if asynchronous else ""))
    assert relnorm(s, s_ref) <= 1e-9
    H.mu = 40.0
    s, fix, info = _search(bh, H, A, xlow, xupp, x, g, delta, 1)
    s_ref, fix_ref, n_hd = _oracle(J, C, A, 40.0, xlow, xupp, x, g, delta)
    assert info["form"] == FORM_GRAM_EQ and H.gram_builds == 2
    assert np.array_equal(fix, fix_ref) and info["n_hmul"] == n_hd
    note_tol("cauchy_step from G with equalities: step vs oracle, 1e-9", relnorm(s, s_ref), 1e-9, "new mu%s" % (", async ingest" if asynchronous else ""))
    assert relnorm(s, s_ref) <= 1e-9
    H.close()


# ------------------------------------------------------------------------------------------------------------ 6. error path
def test_no_breakpoint_left_returns_the_same_code_in_both_forms(bh):
    """One NaN in g (n = 6, mA = 1).  Device against device: the same return code with the option on and off — and the call
    returns (the loop is bounded by n + 1 passes)."""
    n = 6
    rng = np.random.default_rng(3)
    J = rng.standard_normal((20, n)) / np.sqrt(20.0)
    A = rng.standard_normal((1, n))
    g = rng.standard_normal(n)
    g[2] = np.nan
    x, xlow, xupp = np.zeros(n), -np.ones(n), np.ones(n)
    H = _gram(bh, J, None, 0.0)
    codes, forms = [], []
    for eq in (0, 1):
        bh.set_option("cauchy_gram_eq", eq)
        cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
        try:
            bh.cauchy_step(x, g, H, cons, 10.0)
            codes.append(0)
        except bh.BenlsipHipError as e:
            codes.append(e.code)
        finally:
            bh.set_option("cauchy_gram_eq", 0)
        forms.append(bh.cauchy_info(cons)[0])
        cons.close()
    assert forms == [FORM_ROWSPACE_EQ, FORM_GRAM_EQ], forms
    assert codes[0] == codes[1], codes
    H.close()


# ------------------------------------------------------------------------------------------------------------ 7. resident chain
class _GramResident(HipOpsResident):
    def new_hessian(self, J, C, mu):
        H = self.bh.AlHessian(J, C, mu)
        H.set_form("gram")
        return H


def test_resident_inner_step_takes_the_search_from_g(bh):
    """bh.inner_step with mA = 3 on a Gram-form handle with the option on against the oracle's inner_step, under the rule of
    test_inner_step_device_chain_against_oracle (its shape with equalities); the PCIe bytes of the loop are those of the
    option-off run."""
    d, n, mA = 1500, 300, 3
    J = R.synthetic_J(d, n, seed=1)
    inst = R.synthetic_box_vectors(d, n, fix_every=8)
    A = np.random.default_rng(5).standard_normal((mA, n))
    L0 = R.chol_lower(A @ A.T)
    x = inst.x - A.T @ np.linalg.solve(A @ A.T, A @ inst.x)
    x = np.clip(x, inst.x_l, inst.x_u)
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
    bh.set_option("cauchy_gram_eq", 1)
    try:
        s_on, pred_on, log_on, fix_on, form_on = run(on)
    finally:
        bh.set_option("cauchy_gram_eq", 0)
    assert (form_off, form_on) == (FORM_ROWSPACE_EQ, FORM_GRAM_EQ)
    assert [e[1] for e in log_on] == [e[1] for e in log_ref]
    assert [e[2] for e in log_on] == [e[2] for e in log_ref]
    assert np.array_equal(fix_on, fix_ref)
    note_tol("inner_step with the Cauchy search from G with equalities: s vs oracle, 1e-6", relnorm(s_on, s_ref), 1e-6)
    assert relnorm(s_on, s_ref) <= 1e-6, relnorm(s_on, s_ref)
    assert pred_on == pytest.approx(pred_ref, rel=1e-8)
    assert on.loop_minor == off.loop_minor and on.loop_bytes == off.loop_bytes, (on.loop_bytes, off.loop_bytes)
