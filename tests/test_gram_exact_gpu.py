"""The three device paths of a Gram-form handle on the exact instances of tests/gram_cases.py (proved exact, equal to the oracle
and placed on the edges they name by tests/test_gram_cases_cpu.py):

    gram_cg_kernel<T, CPT, R, NOPF> + cg_reduce_update_kernel   option gram_cg_fused    families C2, C3, every geometry, two grids
    cauchy_gram_kernel<REG>                                     option cauchy_gram      family K: REG = true and the streamed tiles
    cauchy_gram_eq_kernel + image_b_mfma_kernel (J := G)        option cauchy_gram_eq   family E: every cpg, block tails, pass 128

Every assertion is equality of bits (float64 viewed as uint64) or of integers: the instances have one right answer whatever the
grid, the tile or the order of a reduction, so a tie resolved the other way, an element lost at a tile edge, a dropped gamma
partial, a row_p that is not the stored p_j, a wrong column slice or an update applied twice is a different bit.  Every option
touched is back at its default afterwards."""
import ctypes as ct
import functools

import numpy as np
import pytest

import gram_cases as gc
import refresh_cases as rc

pytestmark = pytest.mark.gpu

FORM_ROWSPACE, FORM_ROWSPACE_EQ, FORM_GRAM, FORM_GRAM_EQ = 1, 2, 3, 4
DEFAULTS = {"gram_cg_fused": 0, "blocks_per_cu": 0, "cauchy_gram": 0, "cauchy_gram_eq": 0, "cauchy_gemm": 1}


@pytest.fixture
def options(bh):
    """options(key=value, ...) sets library options; every option this module touches is back at its default afterwards."""
    def set_options(**kw):
        for k, v in kw.items():
            assert k in DEFAULTS
            bh.set_option(k, v)
    try:
        yield set_options
    finally:
        for k, v in DEFAULTS.items():
            bh.set_option(k, v)


@pytest.fixture(scope="module")
def n_cu(bh):
    n = ct.c_int32(0)
    bh._lib.check(bh._lib.lib().bh_device_info(None, 0, ct.byref(n), None, 0), "bh_device_info")
    return int(n.value)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------ the case table
def test_case_table(n_cu, capsys):
    """Prints, once per session and past the capture, what every case makes the kernels do on this device: geometry, grid, passes
    per workgroup and the edge the case places."""
    lines = ["", "Gram-form exact cases for %d compute units (tests/gram_cases.py):" % n_cu]
    for n in gc.CG_SIZES:
        for bpc in gc.cg_grids(n):
            lines += ["  " + line for line in gc.describe_cg(n, n_cu, bpc)]
    for n in gc.K_SIZES:
        for c in gc.k_cases(n):
            hit = np.flatnonzero(c.inst[7] < 1024.0)
            lines.append("  K  n=%-5d REG = %-5s %d tile(s)  %-16s %2d bounded variables  %s" % (n, n <= gc.TILE, -(-n // gc.TILE), c.name, hit.size, c.note))
    lines += ["  K  n=%-5d %-16s %s" % (c.n, c.name, c.note) for c in gc.k_all_fixed() + [gc.k_no_breakpoint(1030), gc.k_no_breakpoint(4097)]]
    lines += ["  " + gc.describe_e(*e) for e in gc.E_CASES]
    with capsys.disabled():
        print("\n".join(lines))
    for n in gc.CG_SIZES:                                  # the placements were designed for this grid (gram_cases.N_CU_DESIGN)
        for bpc in gc.cg_grids(n):
            assert {i for i, _ in gc.cg_placements(n, n_cu, bpc)} <= set(gc.cg_instance("C2", n).deciding)


# ---------------------------------------------------------------------------------------------------------- families C2 and C3
@functools.lru_cache(maxsize=None)
def _cg_ref(family, n, index, kind, side):
    """The oracle's (w, status, iters, trace rows) of a case, computed once and read-only."""
    case = gc.short_case(family, n) if kind == "short" else gc.cg_case(family, n, index, kind, side)
    ref = gc.cg_oracle(case)
    ref[0].setflags(write=False)
    ref[3].setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def cg_handle(bh):
    """cg_handle(family, n): ONE Gram-form handle and one constraint handle per (family, n), shared by every placement and both
    grids of that size (the parametrisation keeps them adjacent; the previous pair is closed when the key changes)."""
    slot = {}

    def close():
        if slot:
            slot["H"].close()
            slot["cons"].close()
            slot.clear()

    def get(family, n):
        if slot.get("key") != (family, n):
            close()
            inst = gc.cg_instance(family, n)
            H = bh.AlHessian(inst.J, inst.C if inst.C.shape[0] else None, inst.mu)
            H.set_form("gram")
            slot.update(key=(family, n), H=H, cons=bh.MixedConstraints(np.zeros((0, n)), None, inst.fix))
        return slot["H"], slot["cons"]
    try:
        yield get
    finally:
        close()


def _pcg(bh, H, cons, case):
    w, st, info = bh.projected_cg(case.g, H, case.w_l, case.w_u, cons, case.kappa2, trace_cap=8, full_output=True)
    return w, int(st), info["iters"], info["n_hmul"], info["trace"]


def _check_cg(out, ref, fix, what):
    w, st, iters, n_hmul, trace = out
    w_ref, st_ref, it_ref, tr_ref = ref
    assert (st, iters, n_hmul) == (st_ref, it_ref, tr_ref.shape[0]), (what, st, iters, n_hmul, st_ref, it_ref, tr_ref.shape[0])
    assert same_bits(trace, tr_ref), (what, trace, tr_ref)
    assert same_bits(w, w_ref), (what, np.flatnonzero(bits(w) != bits(w_ref))[:8])
    assert not np.any(bits(w[fix])), what                                        # fixed components: +0.0


@pytest.mark.parametrize("family,n,bpc", [(f, n, b) for f in ("C2", "C3") for n in gc.CG_SIZES for b in gc.cg_grids(n)])
def test_cg_is_the_oracle_bit_for_bit(bh, options, n_cu, cg_handle, family, n, bpc):
    """Every placement of (family, n) at one grid, all on one handle.  Per case: the fused loop; the identical call again (its stop
    launch is now predicted: the NOPF symbol); a one-iteration call and the case once more (launch 2 is predicted to stop, takes
    the NOPF symbol and must carry on); the separate-kernel loop (option 0)."""
    inst = gc.cg_instance(family, n)
    H, cons = cg_handle(family, n)
    options(blocks_per_cu=bpc)
    short = gc.short_case(family, n)
    short_ref = _cg_ref(family, n, 0, "short", short.side)
    assert (short_ref[1], short_ref[2]) == (1, 1)
    for c in gc.cg_cases(family, n, n_cu, bpc):
        what = "%s n=%d bpc=%d i=%d %s from %s (%s)" % (family, n, bpc, c.index, c.kind, c.side, c.edge)
        ref = _cg_ref(family, n, c.index, c.kind, c.side)
        assert ref[2] >= 2
        options(gram_cg_fused=1)
        _check_cg(_pcg(bh, H, cons, c), ref, inst.fix, what + ": fused")
        assert H.stats()["cg_kernels"] == 2
        _check_cg(_pcg(bh, H, cons, c), ref, inst.fix, what + ": fused, the identical call again")
        _check_cg(_pcg(bh, H, cons, short), short_ref, inst.fix, what + ": the one-iteration call")
        _check_cg(_pcg(bh, H, cons, c), ref, inst.fix, what + ": fused, after a shorter call")
        assert H.stats()["cg_kernels"] == 2
        options(gram_cg_fused=0)
        _check_cg(_pcg(bh, H, cons, c), ref, inst.fix, what + ": gram_cg_fused = 0")
        assert H.stats()["cg_kernels"] == 0
    assert H.gram_builds == 1


# -------------------------------------------------------------------------------------------------------------- families K, E
@functools.lru_cache(maxsize=None)
def _k_cases(n):
    """The cases of family K at width n with the oracle's (step, active set, passes) — computed once, read-only."""
    out = []
    for c in gc.k_cases(n):
        J, C, mu, A, x, g, xlow, xupp, delta = c.inst
        ref = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
        for arr in (J, C, x, g, xlow, xupp) + ref[:2]:
            arr.setflags(write=False)
        out.append((c, ref))
    return out


def _search(bh, H, inst, set_options, **opts):
    """One search on a fresh constraint handle under `opts`: (step, active set, info, growth of the handle's n_hmul, of n_jv)."""
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    set_options(**opts)
    try:
        cons = bh.MixedConstraints(A, None, None, l=xlow, u=xupp)
        st0 = H.stats()
        try:
            s, info = bh.cauchy_step(x, g, H, cons, delta, full_output=True)
            st1 = H.stats()
            fix = np.asarray(cons.fixvars, dtype=bool).copy()
        finally:
            cons.close()
    finally:
        set_options(**{k: DEFAULTS[k] for k in opts})
    return s, fix, info, st1["n_hmul"] - st0["n_hmul"], st1["n_jv"] - st0["n_jv"]


def _check_search(out, ref, form, what):
    s, fix, info, _, _ = out
    s_ref, fix_ref, passes = ref
    assert info["form"] == form, (what, info)
    assert (info["n_hmul"], info["n_breakpoints"]) == (passes, int(fix_ref.sum())), (what, info, passes)
    assert np.array_equal(fix, fix_ref), (what, np.flatnonzero(fix), np.flatnonzero(fix_ref))
    assert same_bits(s, s_ref), (what, np.flatnonzero(bits(s) != bits(s_ref))[:8])


def _gram(bh, inst):
    H = bh.AlHessian(inst[0], inst[1] if inst[1].shape[0] else None, inst[2])
    H.set_form("gram")
    return H


@pytest.mark.parametrize("n", gc.K_SIZES)
def test_cauchy_gram_is_the_oracle_bit_for_bit(bh, options, n):
    """Family K on ONE Gram-form handle per width: every hitting order, tie and ending with cauchy_gram = 1 (form 3: one G d, then
    the whole search in one launch), and the same bits from the row-space form on the same handle with the option off."""
    cases = _k_cases(n)
    H = _gram(bh, cases[0][0].inst)
    wrong = []                                                       # every case is run; the cases that differ are reported together
    try:
        for c, ref in cases:
            what = "K n=%d %s" % (n, c.name)
            try:
                out = _search(bh, H, c.inst, options, cauchy_gram=1)
                _check_search(out, ref, FORM_GRAM, what + ": cauchy_gram = 1")
                assert out[3:] == (1, 0), (what, out[3:])
                off = _search(bh, H, c.inst, options)
                _check_search(off, ref, FORM_ROWSPACE, what + ": cauchy_gram = 0")
                assert off[3] == 0, (what, off[3:])
            except AssertionError as e:
                wrong.append(str(e).splitlines()[0])
        assert H.gram_builds == 1
    finally:
        H.close()
    assert not wrong, "\n".join(wrong)


def test_cauchy_gram_every_variable_fixed(bh, options):
    """block_cases.all_fixed through form 3: n advances, pass n + 1 ends on nfix == nmm."""
    for c in gc.k_all_fixed():
        J, C, mu, A, x, g, xlow, xupp, delta = c.inst
        ref = rc.oracle_step(J, None, mu, None, x, g, xlow, xupp, delta)
        assert ref[2] == c.n + 1 and ref[1].all()
        H = _gram(bh, c.inst)
        try:
            _check_search(_search(bh, H, c.inst, options, cauchy_gram=1), ref, FORM_GRAM, c.name)
            _check_search(_search(bh, H, c.inst, options), ref, FORM_ROWSPACE, c.name + ": cauchy_gram = 0")
        finally:
            H.close()


@pytest.mark.parametrize("n", [1030, 4097])
def test_cauchy_gram_no_breakpoint_left_is_the_same_error(bh, options, n):
    """J = 0, infinite bounds and trust region: pass 0 finds no breakpoint (ind < 0) — the error code of the row-space form, and the
    call returns."""
    c = gc.k_no_breakpoint(n)
    H = _gram(bh, c.inst)
    codes = []
    try:
        for gram in (0, 1):
            try:
                _search(bh, H, c.inst, options, cauchy_gram=gram)
                codes.append(0)
            except bh.BenlsipHipError as e:
                codes.append(e.code)
    finally:
        H.close()
    assert codes[0] == codes[1] != 0, codes


@functools.lru_cache(maxsize=None)
def _e_case(n, mA, npass):
    inst = gc.e_instance(n, mA, npass)
    ref = rc.oracle_step(*inst)
    assert ref[2] == npass
    for arr in inst[:2] + inst[3:8] + ref[:2]:
        arr.setflags(write=False)
    return inst, ref


@pytest.mark.parametrize("n,mA,npass", gc.E_CASES)
def test_cauchy_gram_eq_is_the_oracle_bit_for_bit(bh, options, n, mA, npass):
    """Family E with cauchy_gram_eq = 1 (form 4): the handle's n_hmul grows by the G v launches, 1 + (passes - 1) // 128; the same
    bits from the row-space form (2) on an implicit-form handle — past one 4096-column panel also with cauchy_gemm = 1 named, where
    n_jv + 1 shows that B came from image_b_mfma_kernel (mA sweeps more otherwise): its K-tail against the oracle."""
    inst, ref = _e_case(n, mA, npass)
    what = "E n=%d mA=%d passes=%d" % (n, mA, npass)
    H = _gram(bh, inst)
    try:
        out = _search(bh, H, inst, options, cauchy_gram_eq=1)
        _check_search(out, ref, FORM_GRAM_EQ, what + ": cauchy_gram_eq = 1")
        assert out[3:] == (1 + (npass - 1) // gc.EQ_REFRESH, 0), (what, out[3:])
        assert H.gram_builds == 1
    finally:
        H.close()
    Hi = bh.AlHessian(inst[0], inst[1], inst[2])
    try:
        _check_search(_search(bh, Hi, inst, options), ref, FORM_ROWSPACE_EQ, what + ": implicit form")
        if n > gc.MFMA_PANEL:
            gemm = _search(bh, Hi, inst, options, cauchy_gemm=1)
            _check_search(gemm, ref, FORM_ROWSPACE_EQ, what + ": implicit form, cauchy_gemm = 1")
            assert gemm[3:] == (0, 1), (what, gemm[3:])
    finally:
        Hi.close()
