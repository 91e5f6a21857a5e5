"""The CG loop with linear equalities, its decisions bit for bit at kernel-sized n, on the exact instances of tests/cg_eq_cases.py
(proved exact, equal to the oracle and placed on the edges they name by tests/test_cg_eq_cases_cpu.py):

    shape                                options                                   kernels it pins
    three kernels                        cg_fused = 1, proj_form = 1,              cg_reduce_update_kernel<GEN>, proj_apply_linv_kernel<INIT>
                                         linv_refine 1 | 0                         and <!INIT>, the CGP prologue with equalities
    the identical call again; the short  same                                      the predicted-stop symbol CGP = 2, and CGP = 2 predicted
    case, then the case again                                                      wrongly: it must carry on
    four kernels                         cg_fused = 2                              trsv_small_kernel, proj_left_mul_tr_kernel<true, 4>
    seven kernels                        cg_fused = 0, proj_form 1 | 0; every      the separate step kernels (cg_step_kernel at n = 8200), the
                                         shape at mA = 65                          augmented form, the blocked factor
    compact image                        free_image_eq = 1, free_image = 2         cg_reduce_update_compact_kernel against the oracle (one answer,
                                                                                   no edge placement claimed: tests/test_free_image_eq_gpu.py)
    Gram-form handle                     set_form("gram"), gram_cg_fused = 1       the equality arm of gram_cg_kernel (n = 2050, 4099)
    device pointers                      bh_pcg_dev, n = 4096 | 4099               the caller's buffers in place (n == ld) and staged (odd n)

Every assertion is equality of bits (float64 viewed as uint64) or of integers against the oracle: w, status, iters, n_hmul, every
trace row.  After every call the statistics of the handle must name the shape under test (cg_kernels, the free-image report): a
cell the plan routes elsewhere fails.  The instances have one right answer whatever the grid, the block, the quarter or the lane
order, so a tie resolved the other way, a partial block of A_free r dropped, a y left over from the iteration before or a gamma
partial lost at a run edge is a different bit.  Every option touched is back at its default afterwards."""
import ctypes as ct

import numpy as np
import pytest

import cg_eq_cases as ce
import gram_cases as gc
from test_cg_rows_exact_gpu import _check, _pcg, _pcg_dev, bits

pytestmark = pytest.mark.gpu

DEFAULTS = {"cg_fused": 1, "proj_form": 1, "linv_refine": 1, "free_image": 1, "free_image_eq": 0, "gram_cg_fused": 0, "blocks_per_cu": 0}
DEV_SIZES = (4096, 4099)                 # bh_pcg_dev: n == ld (in place) and an odd n past 4096 (staged)
GRAM_CELLS = ((2050, 17), (4099, 64))
GROUPS = ("placed", "N", "EC2n", "T")
CELLS = [(n, mA, bpc, grp) for n, mA in ce.TABLE for grp in GROUPS for bpc in (gc.cg_grids(n) if grp in ("placed", "EC2n") else (0,))
         if grp != "T" or (n, mA) in ce.T_TABLE]


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


# ------------------------------------------------------------------------------------------------------------ the case table
def test_case_table(n_cu, capsys):
    """Prints, once per session and past the capture, what every case makes the kernels do on this device and FAILS on a device
    whose grids the instances were not designed for."""
    lines = ["", "Equality-loop exact cases for %d compute units (tests/cg_eq_cases.py):" % n_cu]
    for n, mA in ce.TABLE:
        for bpc in gc.cg_grids(n):
            lines += ["  " + line for line in ce.describe_eq(n, mA, n_cu, bpc)]
    lines.append("  each placement: a tie and a half step (w_l and w_u alternate inside / outside the supports); EC2n from both sides")
    for n, mA in ce.TABLE:
        nn = ce.n_cases(n, mA)
        t = ce.t_cases(n, mA) if (n, mA) in ce.T_TABLE else None
        lines.append("  N  n=%-5d mA=%-2d atol = %.17g | its lower neighbour | %.17g%s"
                     % (n, mA, nn[0].atol, nn[2].atol, "" if t is None else "    T  mt=%d kappa2 = %.17g | its upper neighbour" % (ce.instance_of(t[0]).mt, t[0].kappa2)))
    with capsys.disabled():
        print("\n".join(lines))
    for n in ce.SIZES:
        for bpc in gc.cg_grids(n):
            placed = {i for i, _ in ce.eq_placements(n, n_cu, bpc)}
            assert placed <= set(ce.eq_reserved(n)), (n, bpc, sorted(placed - set(ce.eq_reserved(n))))


# ------------------------------------------------------------------------------------------------------------------ plumbing
_REFS = {}


def ref_of(c):
    """The oracle's (w, status, iters, trace rows) of a case, computed once per session and read-only."""
    key = (c.group, c.n, c.mA, c.index, c.kind, c.side)
    if key not in _REFS:
        ref = ce.eq_oracle(c)
        ref[0].setflags(write=False)
        ref[3].setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


@pytest.fixture(scope="module")
def eq_handles(bh):
    """eq_handles(n, mA, kind): ONE implicit handle and one constraint handle (with the reference's augmented factor, read under
    proj_form = 0 only) per (kind, n, mA), shared by every case, grid and shape; the parametrisation keeps the cells of one
    (n, mA) adjacent, and the handles of the previous one are closed when it changes."""
    slot = {}

    def close():
        for H, cons in slot.get("pairs", {}).values():
            H.close()
            cons.close()
        slot.clear()

    def get(n, mA, kind="EC2", gram=False):
        if slot.get("key") != (n, mA):
            close()
            slot.update(key=(n, mA), pairs={})
        if (kind, gram) not in slot["pairs"]:
            inst = ce.eq_instance(n, mA, kind)
            H = bh.AlHessian(ce.dense_J(inst), inst.q.reshape(1, n), ce.mu_of(inst))
            if gram:
                H.set_form("gram")
            assert H.form == ("gram" if gram else "implicit")
            slot["pairs"][(kind, gram)] = (H, bh.MixedConstraints(ce.dense_A(inst), ce.factor_aug(inst), inst.fix))
        return slot["pairs"][(kind, gram)]
    try:
        yield get
    finally:
        close()


def _form(options, cons, form):
    """The projection form is read when the active set is pushed: set the option, then push again."""
    options(proj_form=form)
    cons.mark_dirty()


def _run(bh, H, cons, c, fix, what, kernels, dev=False):
    H.mu = c.mu
    _check((_pcg_dev if dev else _pcg)(bh, H, cons, c), ref_of(c), fix, what)
    assert H.stats()["cg_kernels"] == kernels, (what, H.stats()["cg_kernels"], kernels)


def _every_shape(bh, options, H, cons, cases, short, fix, tag):
    """Every shape of the table on every case, all on one pair of handles."""
    n, mA = cases[0].n, cases[0].mA
    fused = mA <= 64
    _form(options, cons, 1)
    for c in cases:
        what = "%s %s i=%d %s from %s (%s)" % (tag, c.group, c.index, c.kind, c.side, c.edge)
        if fused:
            options(cg_fused=1, linv_refine=1, free_image=0, free_image_eq=0)
            _run(bh, H, cons, c, fix, what + ": three kernels", 3)
            if short is not None:
                _run(bh, H, cons, c, fix, what + ": three kernels, the identical call again", 3)
                _run(bh, H, cons, short, fix, what + ": the one-iteration call", 3)
                _run(bh, H, cons, c, fix, what + ": three kernels, after a shorter call", 3)
            options(linv_refine=0)
            _run(bh, H, cons, c, fix, what + ": three kernels, linv_refine = 0", 3)
            options(linv_refine=1, cg_fused=2)
            _run(bh, H, cons, c, fix, what + ": four kernels", 4)
            options(cg_fused=1, free_image=2, free_image_eq=1)
            served = H.free_image_info(cons)["calls_served"]
            _run(bh, H, cons, c, fix, what + ": compact image", 3)
            info = H.free_image_info(cons)
            assert (info["state"], info["width"], info["calls_served"]) == ("valid", n - int(fix.sum()), served + 1), (what, info)
            options(free_image=0, free_image_eq=0)
            if n in DEV_SIZES:
                _run(bh, H, cons, c, fix, what + ": bh_pcg_dev", 3, dev=True)
        else:
            options(cg_fused=1, free_image=0, free_image_eq=0)
            _run(bh, H, cons, c, fix, what + ": mA = 65 under cg_fused = 1 (the separate shape)", 0)
        options(cg_fused=0)
        _run(bh, H, cons, c, fix, what + ": seven kernels", 0)
    try:
        _form(options, cons, 0)
        options(cg_fused=0, free_image=0, free_image_eq=0)
        for c in cases:
            what = "%s %s i=%d %s from %s (%s)" % (tag, c.group, c.index, c.kind, c.side, c.edge)
            _run(bh, H, cons, c, fix, what + ": seven kernels, augmented form", 0)
    finally:
        _form(options, cons, 1)
        H.mu = ce.mu_of(ce.instance_of(cases[0]))


# --------------------------------------------------------------------------------------------------------------- the implicit handle
@pytest.mark.parametrize("n,mA,bpc,group", CELLS, ids=["n%d-mA%d-bpc%d-%s" % c for c in CELLS])
def test_equality_loop_is_the_oracle_bit_for_bit(bh, options, n_cu, eq_handles, n, mA, bpc, group):
    """placed: every placement of the grid as a tie and as a half step.  N: atol == pHp_2 (negative_curvature, w_1 untouched, gamma
    NaN in the trace), one ulp below (runs on), atol == pHp_1 (w = 0).  EC2n: pHp_2 < 0, a step to the one bound at gamma = 2^-4,
    from w_l and from w_u at every placement.  T: |r.v| == tol_cg goes on (iters 3), one ulp of kappa2 more stops (iters 2)."""
    kind = "T" if group == "T" else "EC2"
    inst = ce.eq_instance(n, mA, kind)
    H, cons = eq_handles(n, mA, kind)
    short = None
    if group == "placed":
        assert {i for i, _ in ce.eq_placements(n, n_cu, bpc)} <= set(inst.inside) | set(inst.outside)
        cases, short = ce.placed_cases(n, mA, n_cu, bpc), ce.short_case(n, mA)
        assert ref_of(short)[1:3] == (1, 1) and all(ref_of(c)[1:3] == ((0, 3) if c.kind == "tie" else (1, 2)) for c in cases)
    elif group == "N":
        at2, below2, at1 = ce.n_cases(n, mA)
        cases = [at2, below2, at1, at2]
        assert [ref_of(c)[1:3] for c in cases[:3]] == [(2, 2), (0, 3), (2, 1)]
        assert np.isnan(ref_of(at2)[3][1, 2]) and not bits(ref_of(at1)[0]).any()
    elif group == "EC2n":
        cases = ce.ec2n_cases(n, mA, n_cu, bpc)
        assert all(ref_of(c)[1:3] == (2, 2) and ref_of(c)[3][1, 0] < 0 and ref_of(c)[3][1, 2] == 2.0 ** -4 for c in cases)
    else:
        tie, above = ce.t_cases(n, mA)
        cases = [tie, above, tie]
        assert ref_of(tie)[1:3] == (0, 3) and ref_of(tie)[3].shape[0] == 2 and ref_of(above)[1:3] == (0, 2) and ref_of(above)[3].shape[0] == 1
    for b in ((bpc,) if group in ("placed", "EC2n") else gc.cg_grids(n)):             # N and T place nothing: both grids in one cell
        options(blocks_per_cu=b)
        _every_shape(bh, options, H, cons, cases, short, inst.fix, "n=%d mA=%d bpc=%d" % (n, mA, b))


# ----------------------------------------------------------------------------------------------------------- the Gram-form handle
@pytest.mark.parametrize("n,mA", GRAM_CELLS)
def test_equality_arm_of_the_gram_form_loop(bh, options, n_cu, eq_handles, n, mA):
    """gram_cg_kernel with equalities (three kernels: G p, the GEN update, proj_apply_linv_kernel) on every placed case, the
    identical call again, after the one-iteration call, on N and on EC2n (G is built again for its mu); gram_cg_fused = 0 takes the
    separate shape."""
    inst = ce.eq_instance(n, mA)
    H, cons = eq_handles(n, mA, gram=True)
    _form(options, cons, 1)
    short = ce.short_case(n, mA)
    try:
        for c in ce.placed_cases(n, mA, n_cu, 0) + ce.n_cases(n, mA) + ce.ec2n_cases(n, mA, n_cu, 0)[:4]:
            what = "gram n=%d mA=%d %s i=%d %s from %s (%s)" % (n, mA, c.group, c.index, c.kind, c.side, c.edge)
            options(gram_cg_fused=1)
            _run(bh, H, cons, c, inst.fix, what + ": fused", 3)
            _run(bh, H, cons, c, inst.fix, what + ": fused, the identical call again", 3)
            if c.group == "EC2":
                _run(bh, H, cons, short, inst.fix, what + ": the one-iteration call", 3)
                _run(bh, H, cons, c, inst.fix, what + ": fused, after a shorter call", 3)
            options(gram_cg_fused=0)
            _run(bh, H, cons, c, inst.fix, what + ": gram_cg_fused = 0", 0)
        assert H.form == "gram" and H.gram_builds == 2                       # mu = 3 lam / mt, then once for mu = -2 lam / mt
    finally:
        H.mu = ce.mu_of(inst)
    # T on its own pair of handles: the exit test of gram_cg_kernel's prologue
    tinst = ce.eq_instance(n, mA, "T")
    H, cons = eq_handles(n, mA, "T", gram=True)
    _form(options, cons, 1)
    tie, above = ce.t_cases(n, mA)
    assert ref_of(tie)[1:3] == (0, 3) and ref_of(above)[1:3] == (0, 2)
    for c in (tie, above, tie):
        options(gram_cg_fused=1)
        _run(bh, H, cons, c, tinst.fix, "gram n=%d mA=%d T %s: fused" % (n, mA, c.kind), 3)
        options(gram_cg_fused=0)
        _run(bh, H, cons, c, tinst.fix, "gram n=%d mA=%d T %s: gram_cg_fused = 0" % (n, mA, c.kind), 0)
