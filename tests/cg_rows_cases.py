"""Exact instances for the box-constrained CG loop on an IMPLICIT handle (helper of tests/test_cg_rows_exact_gpu.py, proved on the
CPU by tests/test_cg_rows_cases_cpu.py).  Not a test.

    row_stream_kernel<..., CGP = 1 | 2> + cg_reduce_update_kernel   option cg_fused = 1    (csrc/bh_matvec.hip.h, bh_cgfuse_body.hip.h)
    cg_step_reg_kernel / cg_step_kernel, cg_init*                   option cg_fused = 0    (csrc/bh_cg.hip.h)
    cg_reduce_update_compact_kernel                                 option free_image = 2  (csrc/bh_freeimg.hip.h)

The families C2 and C3 of tests/gram_cases.py are realised as J, C, mu and run unchanged on an implicit handle; what changes is
the geometry.  An implicit handle streams nrows = d + q rows (n + 1 for C2, n for C3), so grid = min(n_cu blocks_per_cu,
ceil(nrows / R)) and run c / CPT of p_j belongs to workgroup run % grid WITH THIS GRID (n = 100: 13 workgroups here, 14 on the
Gram form).  rows_placements puts the edge list of gram_cases.cg_placements on that grid, and the instances keep those indices
deciding (g != 0, q = +-1, u = 0) through cg_instance's `reserve`.

Further decision edges, all on the same two instances per width:

  T    C3 with k = s^2 live groups (the largest square <= (n - 2) / 9; the surplus gets g = 0).  |v|^2 = 9 k, so
       tol_cg = kappa2 3 s without a rounding, and r.v after iteration 2 is 45 k / 16.  kappa2 = 15 s / 16 makes
       |r.v| == tol_cg: :747 is a strict <, the loop goes on (iters 4).  nextafter(kappa2, +inf) stops it (iters 3).
  N    C2 with atol as the operand: pHp_2 = pHp_1 / 2.  atol = pHp_2 ends iteration 2 with negative_curvature and w = w_1
       untouched (:725 is <=, :727 a strict >); nextafter(pHp_2, 0) runs as usual; atol = pHp_1 ends iteration 1 with w = 0.
  C2n  the C2 instance with mu = -2 lam / m: G q = -lam q, pHp_1 = lam m, alpha_1 = 3 / lam, beta = 8, p_2 = -6 u - 12 c q,
       pHp_2 = -72 lam m < 0 — a real step to the boundary (:727-729) with one finite bound at gamma = 2^-4.

rows_model is projected_cg as the kernels form it from the rows: t = J p, c = C p, pHp = sum t_i^2 + mu sum c_i^2,
Hp = J'(t) + C'(mu c), r.v as a sum of products — every partial sum bounded in integers by the Ledger, so each is one float64
whatever the pass, slab or lane order."""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

import benlsip_ref as R
import gram_cases as gc
import rs_cases as rs

SIZES = gc.CG_SIZES + (4096,)            # + the benchmark's own width: n == ld, device pointers used unpadded
PLACED = ("C2", "C3")                    # the families whose cases sit on placements (C2n: the instance of C2 with another mu)
ROW_FAMILIES = {"C2": 1, "C3": 0, "C2n": 1}     # rows of C


# ------------------------------------------------------------------------------------------------------ geometry of the row form
def nrows_of(family, n):
    return n + ROW_FAMILIES[family]


def rows_geometry(family, n, n_cu, bpc):
    """What row_stream_kernel<CGP> does at width n on an implicit handle of `family`: the stream runs over nrows = d + q rows
    (pcg_make_plan), runs of CPT chunks of p_j are owned by workgroup run % grid."""
    path = rs.path_of(n)
    T, CPT, Rr, bpc_default = rs.config_of(path)
    ld = rs.ld_of(n)
    shape = rs.stream_shape(path, nrows_of(family, n), n_cu, bpc)
    nchunks = ld // 2
    return dict(path=path, T=T, CPT=CPT, R=Rr, ld=ld, nrows=nrows_of(family, n), nchunks=nchunks, grid=shape["grid"], ngroups=shape["ngroups"],
                passes=shape["passes"], busiest=shape["busiest"], nruns=-(-nchunks // CPT), bpc=bpc if bpc > 0 else bpc_default)


def rows_placements(family, n, n_cu, bpc):
    """[(index, edge)]: the edge list of gram_cases.cg_placements on the grid of the row form."""
    return gc.placements_of(n, rows_geometry(family, n, n_cu, bpc))


@functools.lru_cache(maxsize=None)
def rows_reserved(n):
    """Every index any design grid of either placed family places at width n (sorted tuple)."""
    return tuple(sorted({i for f in PLACED for n_cu in gc.N_CU_DESIGN for bpc in gc.cg_grids(n) for i, _ in rows_placements(f, n, n_cu, bpc)}))


# ---------------------------------------------------------------------------------------------------------------- instances
@functools.lru_cache(maxsize=4)
def rows_instance(family, n):
    """gram_cases.cg_instance with the placements of the row form reserved (at most four are kept: J and G of the widest are
    half a gigabyte each).  "C2n": the instance of C2 with mu = -2 lam / m; its G is formed on demand (dense_G)."""
    if family == "C2n":
        base = rows_instance("C2", n)
        m = float(base.q @ base.q)
        return base._replace(family="C2n", mu=-2.0 * gc.LAM / m, G=None)
    return gc.cg_instance.__wrapped__(family, n, rows_reserved(n))


@functools.lru_cache(maxsize=1)
def _c2n_G(n):
    inst = rows_instance("C2n", n)
    G = inst.mu * np.outer(inst.q, inst.q) + 0.0
    G[np.arange(n), np.arange(n)] += np.diag(inst.J) ** 2
    G.setflags(write=False)
    return G


def dense_G(inst):
    """J'J + mu C'C of an instance, entry by entry as gram_cases forms it (J diagonal, C one row); read-only."""
    return inst.G if inst.G is not None else _c2n_G(inst.n)


RowsCase = namedtuple("RowsCase", "group family n index kind side edge g w_l w_u kappa2 atol")


def _wrap(group, c, atol=gc.SQRT_EPS, family=None):
    return RowsCase(group, family or c.family, c.n, c.index, c.kind, c.side, c.edge, c.g, c.w_l, c.w_u, c.kappa2, atol)


def placed_cases(family, n, n_cu, bpc):
    """Every placement of (family, n, grid) once as a tie and once as a half step, the side alternating (gram_cases.cg_cases)."""
    inst = rows_instance(family, n)
    out = []
    for k, (i, edge) in enumerate(rows_placements(family, n, n_cu, bpc)):
        out.append(_wrap(family, gc.cg_case(family, n, i, "tie", ("upper", "lower")[k % 2], edge, inst=inst)))
        out.append(_wrap(family, gc.cg_case(family, n, i, "half", ("lower", "upper")[k % 2], edge, inst=inst)))
    return out


def short_case(family, n):
    return _wrap(family, gc.short_case(family, n, inst=rows_instance(family, n)))


def t_square(n):
    """s with k = s^2 the largest perfect square <= (n - 2) / 9."""
    return math.isqrt((n - 2) // 9)


def t_cases(n):
    """Family T on the instance of C3: no bounds; kappa2 = 15 s / 16 (the tie: the loop goes on) and its upper neighbour."""
    inst = rows_instance("C3", n)
    s = t_square(n)
    k = s * s
    live = np.flatnonzero((inst.g0 == 1.0) & ~inst.fix)                  # in the order the classes were dealt out: 0000 1111 2
    assert live.size >= 9 * k >= 9
    g = np.zeros(n)
    g[live[:9 * k]] = 1.0
    g[inst.fix] = 1.0
    assert [int(np.sum(inst.cls[live[:9 * k]] == c)) for c in (0, 1, 2)] == [4 * k, 4 * k, k]
    inf = np.full(n, np.inf)
    kappa2 = 15.0 * s / 16.0
    return [RowsCase("T", "C3", n, -1, "tie", "", "|r.v| == tol_cg after iteration 2", g, -inf, inf, kappa2, gc.SQRT_EPS),
            RowsCase("T", "C3", n, -1, "above", "", "tol_cg one ulp of kappa2 above |r.v|", g, -inf, inf, float(np.nextafter(kappa2, np.inf)), gc.SQRT_EPS)]


def n_cases(n):
    """Family N on the instance of C2: no bounds, g = u + q; atol is the operand."""
    inst = rows_instance("C2", n)
    m = float(inst.q @ inst.q)
    g = inst.g0 + inst.q
    g[inst.fix] = 1.0
    inf = np.full(n, np.inf)
    pHp1 = 6.0 * gc.LAM * m                                            # lam |u|^2 + 4 lam |q|^2
    pHp2 = pHp1 / 2.0
    mk = lambda kind, edge, atol: RowsCase("N", "C2", n, -1, kind, "", edge, g, -inf, inf, gc.KAPPA2, atol)
    return [mk("at2", "atol == pHp_2: negative curvature, w_1 untouched", pHp2),
            mk("below2", "atol one ulp below pHp_2: two iterations", float(np.nextafter(pHp2, 0.0))),
            mk("at1", "atol == pHp_1: negative curvature at once, w = 0", pHp1)]


def c2n_case(n, index, side, edge=""):
    inst = rows_instance("C2n", n)
    qi = inst.q[index]
    assert qi in (-1.0, 1.0) and inst.g0[index] == 0.0
    want = 1.0 if side == "upper" else -1.0
    c = -want * qi                                                       # p_2,i = -12 c q_i
    g = inst.g0 + c * inst.q
    g[inst.fix] = 1.0
    w1, p2 = (3.0 / gc.LAM) * (-c * qi), -12.0 * c * qi
    assert math.copysign(1.0, p2) == want
    w_l, w_u = np.full(n, -np.inf), np.full(n, np.inf)
    (w_u if side == "upper" else w_l)[index] = w1 + 2.0 ** -4 * p2
    return RowsCase("C2n", "C2n", n, index, "neg", side, edge, g, w_l, w_u, gc.KAPPA2, gc.SQRT_EPS)


def c2n_cases(n, n_cu, bpc):
    """Every placement of the C2 grid, from both sides."""
    return [c2n_case(n, i, side, edge) for i, edge in rows_placements("C2n", n, n_cu, bpc) for side in ("upper", "lower")]


def rows_oracle(case):
    """gram_cases.cg_oracle on the instance the case was placed on."""
    inst = rows_instance(case.family, case.n)
    return gc.cg_oracle(case, inst=inst, atol=case.atol, G=dense_G(inst))


# ------------------------------------------------------------------------------------------------------------- the row model
class Unchecked(gc.Ledger):
    """A ledger that proves nothing: for the faulted models of the sensitivity check, whose quotients need not be exact."""

    def note(self, what, bound):
        pass

    def dot(self, a, b, what):
        return float(np.dot(a, b))

    def quotient(self, a, b, what):
        return a / b

    def axpy(self, a, x, y, what):
        with np.errstate(invalid="ignore"):                          # (a dropped run leaves gamma = inf)
            return y + a * x


def row_operator(inst):
    """What rows_model needs of J, C, mu, checked once: J is diagonal and C has at most one row."""
    diag = np.diag(inst.J).copy()
    assert np.count_nonzero(inst.J) == np.count_nonzero(diag) and inst.C.shape[0] <= 1
    return dict(diag=diag, C=inst.C, mu=inst.mu)


def _mul(led, a, b, what):
    """Elementwise product (either may be a scalar): the largest numerator noted."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ea, eb = gc.dyadic_exp(a), gc.dyadic_exp(b)
    led.note(what, int(gc.units(a, ea).max(initial=0)) * int(gc.units(b, eb).max(initial=0)))
    return a * b


def rows_model(op, g, fix, w_l, w_u, kappa2, led, atol=gc.SQRT_EPS, atol_f2b=1e-10, geo=None, fault=None):
    """projected_cg (src/basic_tralcnlss.jl:690-764) with box constraints as the two-kernel iteration forms it from the rows of
    op = row_operator(inst), every operation through the ledger: returns (w, status, iters, trace rows).

    fault (the sensitivity check; geo names the grid): "ge" alpha >= gamma for :735, "le_tol" <= for :747, "lt_neg" < for :725,
    "drop_last_run" every workgroup leaves the last run it owns out of gamma, "stale_w" the boundary term reads w = 0."""
    n = g.shape[0]
    diag, C, mu = op["diag"], op["C"], op["mu"]
    free = ~fix
    w = np.zeros(n)
    r = g.copy()
    v = np.where(free, r, 0.0)
    rtv = led.dot(r, v, "r.v")
    p = -v
    tol_cg = kappa2 * math.sqrt(led.dot(v, v, "v.v"))
    it, max_iter = 1, 2 * int(free.sum())
    solved = outside = neg = False
    rows = []
    seen = np.ones(n, dtype=bool)
    if fault == "drop_last_run":
        run = (np.arange(n) // 2) // geo["CPT"]
        last_of = {}
        for rr in range(int(run.max()) + 1):
            last_of[rr % geo["grid"]] = rr
        seen = ~np.isin(run, list(last_of.values()))
    while not solved and not outside and not neg and it <= max_iter:
        t = _mul(led, diag, p, "t = J p")                            # one product per row
        pHp = led.dot(t, t, "sum t^2")
        Hp = _mul(led, diag, t, "J't")
        if C.shape[0]:
            c = led.dot(C[0], p, "c = C p")
            pHp = float(led.axpy(mu, np.array([led.dot(np.array([c]), np.array([c]), "c^2")]), np.array([pHp]), "pHp = sum t^2 + mu c^2")[0])
            Hp = led.axpy(1.0, _mul(led, _mul(led, mu, c, "mu c"), C[0], "C'(mu c)"), Hp, "Hp = J't + C'(mu c)")
        gamma = math.inf
        wk = np.zeros(n) if fault == "stale_w" else w
        for i in np.flatnonzero((np.abs(p) >= atol_f2b) & np.isfinite(np.where(p > 0, w_u, w_l)) & seen):
            wb = w_u[i] if p[i] > 0 else w_l[i]
            num = wb - wk[i]
            assert Fraction(num) == Fraction(wb) - Fraction(wk[i])
            gamma = min(gamma, led.quotient(num, p[i], "gamma"))
        if (pHp < atol) if fault == "lt_neg" else (pHp <= atol):     # :725
            neg = True
            if abs(pHp) > atol:                                      # :727
                w = led.axpy(gamma, p, w, "w")
                rows.append((pHp, math.nan, gamma, rtv))
            else:
                rows.append((pHp, math.nan, math.nan, rtv))
            break
        rtv = led.dot(r, v, "r.v")
        alpha = led.quotient(rtv, pHp, "alpha")
        outside = (alpha >= gamma) if fault == "ge" else (alpha > gamma)      # :735
        if outside:
            w = led.axpy(gamma, p, w, "w")
        else:
            w = led.axpy(alpha, p, w, "w")
            r = led.axpy(alpha, Hp, r, "r")
            v = np.where(free, r, 0.0)
            rtv_next = led.dot(r, v, "r.v")
            beta = led.quotient(rtv_next, rtv, "beta")
            p = led.axpy(beta, p, -v, "p")
            rtv = rtv_next
            solved = (abs(rtv) <= tol_cg) if fault == "le_tol" else (abs(rtv) < tol_cg)     # :747
            it += 1
        rows.append((pHp, alpha, gamma, rtv))
    status = (R.CGStatus.solved if solved else R.CGStatus.bound_hit if outside else R.CGStatus.negative_curvature if neg else
              R.CGStatus.max_iter_reached if it == max_iter else R.CGStatus.none)
    return w, int(status), it, np.array(rows).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------------------- the case table
def describe_rows(family, n, n_cu, bpc):
    """Lines of the case table for one (family, n, grid): the geometry, then one line per placement."""
    geo = rows_geometry(family, n, n_cu, bpc)
    lines = ["%s n=%-5d blocks_per_cu=%d: %d rows, geometry %d (T=%d CPT=%d R=%d) grid %d, %d row groups, %d pass(es) per workgroup (%d workgroups "
             "make the last), %d runs of %d chunks" % (family, n, bpc, geo["nrows"], geo["path"], geo["T"], geo["CPT"], geo["R"], geo["grid"],
                                                      geo["ngroups"], geo["passes"], geo["busiest"], geo["nruns"], geo["CPT"])]
    for i, edge in rows_placements(family, n, n_cu, bpc):
        wg, run = gc.owner(i, geo)
        lines.append("      i=%-5d run %-4d workgroup %-4d %s" % (i, run, wg, edge))
    return lines
