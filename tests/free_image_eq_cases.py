"""Active-set sequences WITH LINEAR EQUALITIES for the bit-for-bit check of the three-kernel equality CG loop on the compact image of the
free columns (option free_image_eq; helper of tests/test_free_image_eq_gpu.py, checked on the CPU by
tests/test_free_image_eq_cases_cpu.py).  Not a test.

The sequences, their active sets and the Book mirror are those of tests/free_image_cases.py (imported, not restated); this module adds
the equality block.  A run is a list of calls on ONE Hessian handle:

    run        sequence  mA      states                       what it exercises
    S1_m2_m1   S1        2, 1    widths 140 .. 15, then the   refinement on from two equalities, off with one; the second pass starts
                                 same states again, mA = 1    with freed variables: a rebuild of Jf and of Af at another row count
    S1_m64     S1        64      widths 140 .. 113            all 16 rows per row group of proj_apply_linv_kernel, two of its workgroups
    S3_m17     S3        17      all                          n == ld: the device's own buffers in place; the 16 rg + k edge
    S2_m64     S2        64      all                          33 partial blocks of A_free r, a 323-column move
    S4_m5      S4        5       all                          three constraint handles with DIFFERENT A taking turns on one image
    S5_m1      S5        1       all                          a rebuild after a freed variable

States with nfree <= mA are left out (max_iter = 2 (nfree - mA) must be positive): that drops S1's widths 2 and 1 and nothing else
(checked on the CPU).  The second pass of S1_m2_m1 visits the states of the first, as the table says.

A is a seeded matrix of integers |a| <= 3 in float64, one per constraint handle.  For n <= 2101 every entry of A_free A_free' and every
partial sum of it, in any order, is an integer below 9 * 2101 < 2^53: the Gram matrix, hence the reduced factor, its explicit inverse W
and the refinement operand M are bit-equal whether the device forms them from the masked full columns (the handle of the sequence) or
from the compacted columns (the fresh handle of the comparison).

Instances: J, C, g as free_image_cases.instance with seeds of their own (EQ_SEED), picked on the CPU so that in every call the ORACLE
alone ends the "wide" cell solved with |r.v| never within MARGIN of the tolerance it is compared with, and the "box" cell on the
boundary after at least two products (the radius rule of free_image_cases.py: the first of BOX_FACTORS x max|w_wide| that does).
"""
from collections import namedtuple

import numpy as np

import free_image_cases as F

Call = namedtuple("Call", "who mA k fix width ldf nch action moved builds moves map")

# run: (sequence, the mA of each pass, the largest mA whose cap selects the states, widths kept beyond the cap or None)
RUNS = {
    "S1_m2_m1": ("S1", (2, 1), None),
    "S1_m64": ("S1", (64,), (140, 139, 128, 127, 113)),
    "S3_m17": ("S3", (17,), None),
    "S2_m64": ("S2", (64,), None),
    "S4_m5": ("S4", (5,), None),
    "S5_m1": ("S5", (1,), None),
}
EQ_SEED = {"S1_m2_m1": 2057, "S1_m64": 2008, "S3_m17": 2002, "S2_m64": 3032, "S4_m5": 2005, "S5_m1": 2002}      # picked on the CPU (seed_is_good)
A_SEED = 4100
COND_MAX = 1.0e6


def kept_states(run):
    """Indices of the states of the run's sequence that every pass visits: nfree > mA for the largest mA of the run, and inside the
    table's width list where it has one."""
    seq, mAs, widths = RUNS[run]
    return [k for k, s in enumerate(F.states(seq)) if s.width > max(mAs) and (widths is None or s.width in widths)]


def dropped_by_the_cap(run):
    seq, mAs, _ = RUNS[run]
    return [(seq, s.width) for s in F.states(seq) if s.width <= max(mAs)]


_CALLS = {}


def calls(run):
    """The calls of a run, with the Book mirror's action, counters and map after each."""
    if run in _CALLS:
        return _CALLS[run]
    seq, mAs, _ = RUNS[run]
    sts = F.states(seq)
    book = F.Book()
    out = []
    for mA in mAs:
        for k in kept_states(run):
            st = sts[k]
            action, moved = book.push(st.fix)
            nch = F.geometry_of(book.nfree)[0]
            out.append(Call("%s/%d" % (st.who, mA), mA, k, st.fix.copy(), book.nfree, book.ldf, nch, action, moved, book.builds, book.moves,
                            book.map.copy()))
    _CALLS[run] = out
    return out


def lineq(run, who):
    """The integer lineq matrix of one constraint handle (who = "<name of the sequence's handle>/<mA>")."""
    seq = RUNS[run][0]
    n = F.SEQS[seq][0]
    mA = int(who.split("/")[1])
    rng = np.random.default_rng([A_SEED, sorted(RUNS).index(run), sum(who.encode())])
    return rng.integers(-3, 4, size=(mA, n)).astype(np.float64)


def expected_af(run, c):
    """Af of call c by the mirror's map: mA x ldf, A[:, map[slot]] on the live slots, +0 beyond."""
    A = lineq(run, c.who)
    Af = np.zeros((c.mA, c.ldf))
    Af[:, :c.width] = A[:, c.map[:c.width]]
    return Af


_INST = {}


def instance(run, n_cu, seed=None):
    """J, C, g and the oracle Hessian of a run (the recipe of free_image_cases.instance, seed EQ_SEED[run])."""
    import benlsip_ref as R
    key = (run, n_cu, seed)
    if key not in _INST:
        seq = RUNS[run][0]
        n = F.SEQS[seq][0]
        rows = F.rows_for(seq, n_cu)
        d = rows - F.Q
        rng = np.random.default_rng(EQ_SEED[run] if seed is None else seed)
        scale = rng.permutation(np.geomspace(1.0, F.SCALE_MAX[seq], n))
        J = rng.standard_normal((d, n)) / np.sqrt(d) * scale
        C = rng.standard_normal((F.Q, n)) * F.C_SCALE
        g = J.T @ rng.standard_normal(d) + 1e-3 * rng.standard_normal(n)
        _INST[key] = dict(n=n, d=d, J=J, C=C, g=g, Ho=R.AlHessian(J, C, F.MU))
    return _INST[key]


def projected_gradient(A, fix, g):
    """v = P(g): zero on the fixed variables, g_f - A_f'(A_f A_f')^{-1} A_f g_f on the free ones."""
    free = ~fix
    Af = A[:, free]
    gf = g[free]
    v = np.zeros_like(g)
    v[free] = gf - Af.T @ np.linalg.solve(Af @ Af.T, Af @ gf)
    return v


_CELLS = {}


def cell(run, n_cu, i, setting, band=True, seed=None):
    """The oracle's view of call i of a run under a bounds setting ("wide" | "box"), as free_image_cases.cell with the handle's A."""
    import benlsip_ref as R
    from _util import oracle_iteration_band
    key = (run, n_cu, i, setting, seed)
    I = instance(run, n_cu, seed)
    c = calls(run)[i]
    if key in _CELLS:
        out = _CELLS[key]
        if band and "band" not in out:
            out["band"] = oracle_iteration_band(I["g"], I["Ho"], out["w_l"], out["w_u"], out["cons_o"], F.KAPPA2, variants=F.BAND)
        return out
    IA = dict(n=I["n"], A=lineq(run, c.who))

    def run_once(delta):
        w_l, w_u, cons_o = F.bounds(IA, c.fix, delta)
        tr = R.CGTrace()
        w, s, it = R.projected_cg(I["g"], I["Ho"], w_l, w_u, cons_o, F.KAPPA2, trace=tr)
        return dict(w_l=w_l, w_u=w_u, cons_o=cons_o, w=w, status=int(s), iters=int(it), n_hmul=tr.n_hmul, delta=delta, rows=tr.rows)

    if setting == "wide":
        out = run_once(None)
        tol_cg = F.KAPPA2 * float(np.linalg.norm(projected_gradient(IA["A"], c.fix, I["g"])))
        out["rtv_over_tol"] = [abs(r[3]) / tol_cg for r in out["rows"]]
    else:
        wide = cell(run, n_cu, i, "wide", band=False, seed=seed)
        out = None
        for f in F.BOX_FACTORS:
            t = run_once(f * float(np.max(np.abs(wide["w"]))))
            if t["status"] == int(R.CGStatus.bound_hit) and t["n_hmul"] >= 2:
                out = t
                break
        assert out is not None, ("no radius ends on the boundary after two products", run, i)
    if band:
        out["band"] = oracle_iteration_band(I["g"], I["Ho"], out["w_l"], out["w_u"], out["cons_o"], F.KAPPA2, variants=F.BAND)
    _CELLS[key] = out
    return out


def seed_is_good(run, n_cu, seed):
    """The rule EQ_SEED was picked by (tests/test_free_image_eq_cases_cpu.py asserts it for the seeds above)."""
    import benlsip_ref as R
    from _util import oracle_iteration_band
    try:
        for i in range(len(calls(run))):
            wide = cell(run, n_cu, i, "wide", band=False, seed=seed)
            if wide["status"] != int(R.CGStatus.solved) or wide["n_hmul"] > 64:
                return False
            if not all(x == 0.0 or max(x, 1.0 / x) >= F.MARGIN for x in wide["rtv_over_tol"]):
                return False
            box = cell(run, n_cu, i, "box", band=False, seed=seed)
            if i in (0, len(calls(run)) - 1):                      # the anchors: the oracle decides its own iteration count
                for c in (wide, box):
                    # ... on any machine's BLAS: under every re-association of its own H*p that tests/_util.py knows, and on
                    # eight copies of the instance whose J carries relative perturbations of 1e-15
                    band = oracle_iteration_band(instance(run, n_cu, seed)["g"], instance(run, n_cu, seed)["Ho"], c["w_l"], c["w_u"], c["cons_o"],
                                                 F.KAPPA2, perturbed=8)
                    if set(band.values()) != {(c["status"], c["iters"])}:
                        return False
    except AssertionError:
        return False
    return True


# ------------------------------------------------------------------------------------------- one exact iteration (dyadic numbers)
EXACT_MA = 16
EXACT_N = 208
EXACT_WIDTHS = (150, 144, 17)         # after a build, after a move to a width = 0 mod 16, the smallest width kept (nfree > mA)
EXACT_SEED = 23


def exact_cases():
    """Three reduced-form cases of proj_cases.py on nested free sets of widths EXACT_WIDTHS (A_free = T Q on each set's own free
    columns: one constraint handle per state), n == ld.  Column n - 1 stays free, as in every case of proj_cases.py."""
    import proj_cases as pc
    rng = np.random.default_rng(EXACT_SEED)
    order = np.concatenate([[EXACT_N - 1], rng.permutation(EXACT_N - 1)])
    out = []
    for k, w in enumerate(EXACT_WIDTHS):
        fix = np.ones(EXACT_N, dtype=bool)
        fix[order[:w]] = False
        out.append(pc.reduced_case("compact-eq-exact-w%d" % w, EXACT_MA, EXACT_N, None, EXACT_SEED + 1 + k, fix=fix))
    return out
