"""Exact instances for the three device paths of a Gram-form handle (helper of tests/test_gram_exact_gpu.py, proved on the CPU by
tests/test_gram_cases_cpu.py).  Not a test.

    gram_cg_kernel<T, CPT, R, NOPF>   option gram_cg_fused   families C2, C3   (csrc/bh_gramcg.hip.h, bh_cgfuse_body.hip.h)
    cauchy_gram_kernel<REG>           option cauchy_gram     family K          (csrc/bh_cauchygram.hip.h)
    cauchy_gram_eq_kernel             option cauchy_gram_eq  family E          (csrc/bh_cauchygrameq.hip.h)

Every operand is a dyadic rational small enough that every product and every partial sum the kernels can form, in any order, is
exact in fp64 (Ledger: the proof obligations), so the result is one bit pattern whatever the grid, the tile or the order of a
reduction — and a wrong tie, a dropped element or an update applied twice is another bit pattern.

Family C2 (dense G, two iterations).  G = lam I + (3 lam / m) q q', lam = 16, q in {0, +-1, +-2}^n with q'q = m a power of two,
realised as J = 4 I_n, C = q', mu = 3 lam / m.  G q = 4 lam q and G u = lam u for u orthogonal to q.  g = u + c q (c = +-1) with
|u|^2 = 2 m: alpha_1 = alpha_2 = 1 / (2 lam), beta = 1/2, r_3 = 0 — two iterations and a third launch whose prologue stops.
u = t (q_j e_i - q_i e_j) on P index pairs with q = +-1, t = sqrt(m / P).

Family C3 (diagonal G, three iterations).  G = lam diag(1 | 4 | 16), the three eigenvalues on 4k, 4k and k free variables with
g = +-1 (energies 4 : 4 : 1): alpha = (1/4, 1/8, 1/2) / lam, beta = 5/4, 1/4, r_4 = 0.  The remaining free variables have g = 0.

A case of C2 / C3 puts ONE finite bound on the deciding variable i so that on the second iteration gamma == alpha exactly
("tie": counts as inside, :735 is a strict >) or gamma == alpha / 2 ("half": outside, the step is gamma), from above (w_u decides)
or from below (w_l).  Two variables are fixed (their g is 1: masked).

Family K: refresh_cases.exact_instance with an explicit hitting order over the indices at which cauchy_gram_kernel changes thread,
wave, register slot or tile, and ties whose order shows in the active set (_tie).  Family E: refresh_cases.exact_equality_instance (per_row = 4) over the column slices of
cauchy_gram_eq_kernel and the 16-element blocks; one case of 130 passes crosses the re-formation of a and B at pass 128."""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

import benlsip_ref as R
import block_cases as bc
import refresh_cases as rc
import rs_cases as rs

MANT = 53                        # an integer below 2^53 in units of a power of two is a float64
LAM = 16.0
SQRT_EPS = float(np.sqrt(np.finfo(float).eps))


# ------------------------------------------------------------------------------------------------------------------ the ledger
def dyadic_exp(a):
    """Smallest e >= 0 with a * 2^e an array of integers (a: finite float64)."""
    a = np.asarray(a, dtype=np.float64).ravel()
    nz = a[a != 0.0]
    if nz.size == 0:
        return 0
    assert np.all(np.isfinite(nz))
    m, ex = np.frexp(nz)                                             # nz = m 2^ex, 1/2 <= |m| < 1
    mi = np.abs(m * 2.0 ** MANT).astype(np.int64)                    # the 53-bit mantissa as an integer
    tz = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)     # its trailing zeros (log2 of a power of two is exact)
    return int(max(0, np.max(MANT - tz - ex.astype(np.int64))))


def units(a, e):
    """|a| 2^e as int64 (a 2^e integral, checked)."""
    s = np.abs(np.asarray(a, dtype=np.float64)) * 2.0 ** e
    assert np.all(s == np.rint(s)) and (s.size == 0 or s.max() < 2.0 ** 62)
    return s.astype(np.int64)


class Ledger:
    """The proof that a float64 evaluation is exact.  A sum of products sum_j a_j b_j with a 2^ea and b 2^eb integral is, at every
    partial sum in every order (fused or not), an integer multiple of 2^-(ea + eb) of magnitude at most sum_j |a_j| |b_j|; if
    that bound is below 2^53 units every partial sum is a float64.  The bound is computed in integers; `bits` keeps the worst
    numerator width per kind of quantity."""

    def __init__(self):
        self.bits = {}

    def note(self, what, bound):
        b = int(bound).bit_length()
        self.bits[what] = max(self.bits.get(what, 0), b)
        assert b <= MANT, (what, b)

    def dot(self, a, b, what):
        ea, eb = dyadic_exp(a), dyadic_exp(b)
        ai, bi = units(a, ea), units(b, eb)
        assert int(ai.max(initial=0)) * int(bi.max(initial=0)) * max(ai.size, 1) < 2 ** 62
        self.note(what, int(np.dot(ai, bi)))
        val = float(np.dot(a, b))
        exact = Fraction(int(np.dot(np.where(a < 0, -ai, ai), np.where(b < 0, -bi, bi))), 2 ** (ea + eb))
        assert Fraction(val) == exact, what
        return val

    def matvec(self, M, v, what):
        """M.dense @ v for M = matrix_info(...): the bound of every row by (largest row sum of |M|) x max |v|."""
        ev = dyadic_exp(v)
        vmax = int(units(v, ev).max(initial=0))
        self.note(what, M["rowsum"] * vmax)
        return M["dense"] @ v

    def axpy(self, a, x, y, what):
        """y + a x elementwise: the product a x_i and the sum, both exact."""
        ea, ex, ey = dyadic_exp([a]), dyadic_exp(x), dyadic_exp(y)
        prod = int(units([a], ea)[0]) * int(units(x, ex).max(initial=0))
        self.note(what + " (product)", prod)
        e = max(ea + ex, ey)
        self.note(what, prod * 2 ** (e - ea - ex) + int(units(y, ey).max(initial=0)) * 2 ** (e - ey))
        return y + a * x

    def affine(self, a, B, y, what):
        """-a - B y: row i is -a_i - sum_j B_ij y_j, in the finest of the units of a and of the products."""
        ea, eB, ey = dyadic_exp(a), dyadic_exp(B), dyadic_exp(y)
        e = max(ea, eB + ey)
        rows = units(B, eB).sum(axis=1) if B.size else np.zeros(a.shape[0], dtype=np.int64)
        self.note(what, int(units(a, ea).max(initial=0)) * 2 ** (e - ea)
                  + int(rows.max(initial=0)) * int(units(y, ey).max(initial=0)) * 2 ** (e - eB - ey))
        return -a - B @ y

    def quotient(self, a, b, what):
        q = a / b
        assert Fraction(q) == Fraction(a) / Fraction(b), (what, a, b)
        self.note(what, abs(Fraction(q).numerator))
        return q


def matrix_info(dense):
    """A matrix with the integer facts Ledger.matvec needs: dyadic exponent and the largest row sum of |M| in its units."""
    e = dyadic_exp(dense)
    rowsum = np.abs(dense).sum(axis=1) * 2.0 ** e                  # integers below 2^53: exact in any order
    assert np.all(rowsum == np.rint(rowsum)) and rowsum.max(initial=0.0) < 2.0 ** MANT
    return dict(dense=dense, e=e, rowsum=int(rowsum.max(initial=0.0)) * 1)


# ------------------------------------------------------------------------------------------------- geometry of gram_cg_kernel
# Geometries 0, 1, 2, 3, 4, 5, 5, 6.  2050 and 4099 lie just behind the edges 2048 and 4096 (ld = 2064, 4112: the first sizes of
# geometries 4 and 5), so 2047 (odd, ld = 2048) is there for geometry 3 and 8190 (ld = 8192) is the upper edge of geometry 5.
CG_SIZES = (100, 500, 1000, 2047, 2050, 4099, 8190, 8200)


def cg_geometry(n, n_cu, bpc):
    """What gram_cg_kernel does at width n on n_cu compute units under option blocks_per_cu = bpc (0: the geometry's own): the row
    stream runs over the ld rows of the image of G (pcg_make_plan: nrows = ld), runs of CPT chunks are owned by workgroup
    run % grid."""
    path = rs.path_of(n)
    T, CPT, Rr, bpc_default = rs.config_of(path)
    ld = rs.ld_of(n)
    shape = rs.stream_shape(path, ld, n_cu, bpc)
    nchunks = ld // 2
    return dict(path=path, T=T, CPT=CPT, R=Rr, ld=ld, nchunks=nchunks, grid=shape["grid"], ngroups=shape["ngroups"], passes=shape["passes"],
                busiest=shape["busiest"], nruns=-(-nchunks // CPT), bpc=bpc if bpc > 0 else bpc_default)


def cg_grids(n):
    """The blocks_per_cu settings a size is run at: the default grid, and 1 where that is another grid."""
    return (0,) if rs.config_of(rs.path_of(n))[3] == 1 else (0, 1)


def owner(i, geo):
    """(workgroup, run) that owns element i of p_j and forms its factor_to_boundary term."""
    run = (i // 2) // geo["CPT"]
    return run % geo["grid"], run


def cg_placements(n, n_cu, bpc):
    """[(index, edge)]: 0, 1, n - 1 (with n odd the only element of the last, partial chunk), the first and last element of a
    run of CPT chunks inside the vector, and for the workgroup that owns the last run that holds an element (it owns as many runs
    as any): the first element of its first run, the last element of its last run (n - 1) and, where it owns several, the first
    element of its second run.  Edges that fall on one index are one placement."""
    return placements_of(n, cg_geometry(n, n_cu, bpc))


def placements_of(n, geo):
    """cg_placements for a geometry given as CPT, grid and nruns (the row form has another grid: tests/cg_rows_cases.py)."""
    per_run = 2 * geo["CPT"]
    out = [(0, "index 0"), (1, "index 1"), (n - 1, "index n-1" + (", half of the last chunk" if n % 2 else ""))]
    mid = max(1, geo["nruns"] // 2)
    out += [(mid * per_run, "first element of run %d" % mid), (min((mid + 1) * per_run, n) - 1, "last element of run %d" % mid)]
    last = (n - 1) // per_run                                        # the last run that holds an element (runs behind it are padding)
    wg = last % geo["grid"]                                          # its owner: the workgroup with as many runs as any
    out += [(wg * per_run, "first element of the first run (%d) of workgroup %d" % (wg, wg)),
            (n - 1, "last element of the last run (%d) of workgroup %d" % (last, wg))]
    if last >= geo["grid"]:                                          # that workgroup owns more than one run: one in between, or its second
        nxt = wg + geo["grid"]
        out.append((nxt * per_run, "first element of run %d, the second of workgroup %d" % (nxt, wg)))
    merged = {}
    for i, edge in out:
        merged[i] = (merged[i] + "; " + edge) if i in merged else edge
    return list(merged.items())


def all_cg_indices(n, n_cus=(256,)):
    """Every deciding index any grid of `n_cus` places at width n: the instance keeps g != 0 and q = +-1 there."""
    return sorted({i for n_cu in n_cus for bpc in cg_grids(n) for i, _ in cg_placements(n, n_cu, bpc)})


# ------------------------------------------------------------------------------------------------------ families C2 and C3
CgInstance = namedtuple("CgInstance", "family n lam J C mu G fix g0 q cls deciding")
CgCase = namedtuple("CgCase", "family n index kind side edge g w_l w_u kappa2")
KAPPA2 = 2.0 ** -10
N_CU_DESIGN = (256, 304, 64, 8)          # grids the placements are designed for (any other device: asserted at run time)


def _reserved(n, reserve=()):
    """The deciding indices of width n: the placements of gram_cg_kernel on the design grids and, for a caller that places cases
    elsewhere (tests/cg_rows_cases.py: the grids of the row form), the indices it names.  reserve = () is the instance the Gram
    module has always had."""
    assert all(0 <= i < n for i in reserve)
    return set(all_cg_indices(n, N_CU_DESIGN)) | set(reserve)


def _spare(n, count, taken):
    """`count` indices from n // 3 upwards that no placement uses."""
    out, i = [], n // 3
    while len(out) < count:
        if i not in taken:
            out.append(i)
        i += 1
        assert i < n
    return out


@functools.lru_cache(maxsize=None)
def cg_instance(family, n, reserve=()):
    """The shared part of a family at width n: J (n x n), C, mu, the dense G the oracle multiplies with, the fixed variables and
    the gradient g0 before a case chooses its signs.  Built once per (family, n, reserve), read-only.  `reserve`: a sorted tuple
    of further indices kept as deciding indices (_reserved)."""
    taken = _reserved(n, reserve)
    fixed = _spare(n, 2, taken)
    fix = np.zeros(n, dtype=bool)
    fix[fixed] = True
    taken = taken | set(fixed)
    nf = n - 2
    J = np.zeros((n, n))
    q = np.zeros(n)
    cls = np.zeros(n, dtype=np.int64)
    if family == "C2":
        m = 1 << max(nf - 1, 1).bit_length()                         # the power of two at or above nf
        k = nf - ((nf - m) % 3)                                      # support of q: a + b = k, a + 4 b = m
        b = (m - k) // 3
        assert 0 <= b <= k <= nf and (k - b) + 4 * b == m
        zeros = _spare(n, nf - k, taken)
        taken = taken | set(zeros)
        P = 4 if (m.bit_length() - 1) % 2 == 0 else 8                # m / P a perfect square
        t = math.isqrt(m // P)
        assert t * t * P == m
        pairs = _spare(n, 2 * P, taken)                              # support of u: q = +-1 there, never a deciding index
        taken = taken | set(pairs)
        rng = np.random.default_rng(300 + n)
        support = np.array([i for i in range(n) if not fix[i] and i not in set(zeros)])
        q[support] = rng.choice([-1.0, 1.0], support.size)
        twos = rng.permutation(np.array([i for i in support if i not in taken]))[:b]
        q[twos] *= 2.0
        assert float(q @ q) == m
        u = np.zeros(n)
        for a in range(P):
            i, j = pairs[2 * a], pairs[2 * a + 1]
            u[i], u[j] = t * q[j], -t * q[i]
        assert float(u @ q) == 0.0 and float(u @ u) == 2.0 * m
        J[np.arange(n), np.arange(n)] = math.sqrt(LAM)
        C = q.reshape(1, n).copy()
        mu = 3.0 * LAM / m
        G = mu * np.outer(q, q) + 0.0                                # (+ 0.0: the zeros of q give +0.0, as a sum that starts at +0.0 does)
        G[np.arange(n), np.arange(n)] += LAM
        g0 = u.copy()                                                # a case adds c q
    else:
        k = nf // 9
        assert k >= 1
        zeros = _spare(n, nf - 9 * k, taken)
        live = np.array([i for i in range(n) if not fix[i] and i not in set(zeros)])
        pattern = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2])
        cls[live] = pattern[np.arange(live.size) % 9]
        diag = math.sqrt(LAM) * 2.0 ** cls                           # 4, 8, 16: G = lam (1, 4, 16)
        J[np.arange(n), np.arange(n)] = diag
        C = np.zeros((0, n))
        mu = 0.0
        G = np.zeros((n, n))
        G[np.arange(n), np.arange(n)] = diag * diag
        g0 = np.zeros(n)
        g0[live] = 1.0
    g0[fix] = 1.0                                                    # masked by the projection
    for arr in (J, C, G, fix, g0, q, cls):
        arr.setflags(write=False)
    return CgInstance(family, n, LAM, J, C, mu, G, fix, g0, q, cls, tuple(sorted(_reserved(n, reserve))))


def _p2_sign_c2(inst, i, c):
    return math.copysign(1.0, c * inst.q[i])                        # p_2 = -u + c q / 2, u_i = 0 at a deciding index


def cg_case(family, n, index, kind, side, edge="", inst=None):
    """One bounded case: g and the one finite bound.  p_2,i > 0 is stopped by w_u (side "upper"), p_2,i < 0 by w_l.  `inst`: the
    instance to place it on (default: cg_instance(family, n))."""
    inst = cg_instance(family, n) if inst is None else inst
    want = 1.0 if side == "upper" else -1.0
    g = inst.g0.copy()
    if family == "C2":
        assert inst.q[index] in (-1.0, 1.0, -2.0, 2.0) and inst.g0[index] == 0.0
        c = want * math.copysign(1.0, inst.q[index])
        g = g + c * inst.q
        g[inst.fix] = 1.0
        alpha1 = alpha2 = 1.0 / (2.0 * LAM)
        p1 = -g[index]
        p2 = c * inst.q[index] / 2.0
    else:
        assert inst.g0[index] == 1.0
        coef = (-2.0, -1.25, 1.75)[int(inst.cls[index])]             # p_2 = coef g by eigenvalue class
        g[index] = want * math.copysign(1.0, coef)
        alpha1, alpha2 = 0.25 / LAM, 0.125 / LAM
        p1 = -g[index]
        p2 = coef * g[index]
    assert math.copysign(1.0, p2) == want
    gamma2 = alpha2 if kind == "tie" else alpha2 / 2.0
    bound = alpha1 * p1 + gamma2 * p2                                # w_1,i + gamma_2 p_2,i: dyadic, exact
    w_l, w_u = np.full(n, -np.inf), np.full(n, np.inf)
    (w_u if side == "upper" else w_l)[index] = bound
    return CgCase(family, n, index, kind, side, edge, g, w_l, w_u, KAPPA2)


def short_case(family, n, inst=None):
    """A one-iteration call for the same handle: the bound of variable 0 is met at gamma_1 = alpha_1 / 2."""
    c = cg_case(family, n, 0, "half", "upper", inst=inst)
    alpha1 = 1.0 / (2.0 * LAM) if family == "C2" else 0.25 / LAM
    p1 = -c.g[0]
    w_l, w_u = np.full(n, -np.inf), np.full(n, np.inf)
    (w_u if p1 > 0 else w_l)[0] = (alpha1 / 2.0) * p1
    return CgCase(family, n, 0, "short", "upper" if p1 > 0 else "lower", "one iteration", c.g, w_l, w_u, KAPPA2)


def cg_cases(family, n, n_cu, bpc):
    """The cases of one (family, n, grid): every placement once as a tie and once as a half step, the side alternating so that
    both w_l and w_u decide in both kinds."""
    out = []
    for k, (i, edge) in enumerate(cg_placements(n, n_cu, bpc)):
        out.append(cg_case(family, n, i, "tie", ("upper", "lower")[k % 2], edge))
        out.append(cg_case(family, n, i, "half", ("lower", "upper")[k % 2], edge))
    return out


def cg_model(M, g, fix, w_l, w_u, kappa2, led, atol=SQRT_EPS, atol_f2b=1e-10):
    """projected_cg (src/basic_tralcnlss.jl:690-764) with box constraints, every operation through the ledger: returns
    (w, status, iters, trace rows).  M = matrix_info(G)."""
    n = g.shape[0]
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
    while not solved and not outside and not neg and it <= max_iter:
        Hp = led.matvec(M, p, "G p")
        pHp = led.dot(p, Hp, "p'Hp")
        gamma = math.inf
        for i in np.flatnonzero((np.abs(p) >= atol_f2b) & np.isfinite(np.where(p > 0, w_u, w_l))):
            wb = w_u[i] if p[i] > 0 else w_l[i]
            num = wb - w[i]
            assert Fraction(num) == Fraction(wb) - Fraction(w[i])
            gamma = min(gamma, led.quotient(num, p[i], "gamma"))
        if pHp <= atol:                                              # :725 (only with an atol or a mu of the caller's: the
            neg = True                                               # families of this module never get here)
            if abs(pHp) > atol:                                      # :727
                w = led.axpy(gamma, p, w, "w")
                rows.append((pHp, math.nan, gamma, rtv))
            else:
                rows.append((pHp, math.nan, math.nan, rtv))
            break
        rtv = led.dot(r, v, "r.v")
        alpha = led.quotient(rtv, pHp, "alpha")
        outside = alpha > gamma
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
            solved = abs(rtv) < tol_cg
            it += 1
        rows.append((pHp, alpha, gamma, rtv))
    status = (R.CGStatus.solved if solved else R.CGStatus.bound_hit if outside else R.CGStatus.negative_curvature if neg else
              R.CGStatus.max_iter_reached if it == max_iter else R.CGStatus.none)
    return w, int(status), it, np.array(rows).reshape(-1, 4)


def cg_oracle(case, inst=None, atol=SQRT_EPS, G=None):
    """The oracle's projected_cg on a case with its Gram-form H*v: (J'J + mu C'C) @ p with the matrix formed first — here handed
    over (cg_instance's G; tests/test_gram_cases_cpu.py checks it against J'J + mu C'C), because J'J of an 8200 x 8200 J costs
    more than the whole suite.  Returns (w, status, iters, trace rows).  `inst`, `G`: the instance the case was placed on and its
    matrix (default: cg_instance(case.family, case.n) and its G); `atol`: the curvature threshold (:711)."""
    inst = cg_instance(case.family, case.n) if inst is None else inst
    G = inst.G if G is None else G
    Ho = R.AlHessian(inst.J, inst.C, inst.mu)
    cons = R.make_mixed_constraints(np.zeros((0, case.n)), R.chol_lower(np.zeros((0, 0))), inst.fix)
    tr = R.CGTrace()
    w, st, it = R.projected_cg(case.g, Ho, case.w_l, case.w_u, cons, case.kappa2, atol=atol, hmul_fn=lambda H, v: G @ v, trace=tr)
    return w, int(st), int(it), np.array(tr.rows).reshape(-1, 4)


def describe_cg(n, n_cu, bpc):
    """Lines of the case table for one (n, grid): the geometry, then one line per placement (each is run as a tie and as a half
    step, from w_l and from w_u, in both families)."""
    geo = cg_geometry(n, n_cu, bpc)
    lines = ["C2/C3 n=%-5d blocks_per_cu=%d: geometry %d (T=%d CPT=%d R=%d) grid %d, %d row groups, %d pass(es) per workgroup (%d workgroups make "
             "the last), %d runs of %d chunks" % (n, bpc, geo["path"], geo["T"], geo["CPT"], geo["R"], geo["grid"], geo["ngroups"], geo["passes"],
                                                  geo["busiest"], geo["nruns"], geo["CPT"])]
    for i, edge in cg_placements(n, n_cu, bpc):
        wg, run = owner(i, geo)
        lines.append("      i=%-5d run %-4d workgroup %-4d %s" % (i, run, wg, edge))
    return lines


# ------------------------------------------------------------------------------------------------- geometry of the Cauchy kernels
CA_T = 512                       # threads of cauchy_gram_kernel (csrc/bh_cauchy.hip.h)
CG_E = 8                         # elements of a tile per thread
TILE = CG_E * CA_T               # 4096: REG = true up to here
EQ_BLOCK = 16                    # elements per workgroup of cauchy_gram_eq_rows_body
EQ_REFRESH = 128                 # kCauchyGramEqRefresh (csrc/bh_api.hip)
MFMA_PANEL = 4096


def elem_owner(i):
    """(tile, thread, wave, register slot k) of element i in cauchy_gram_kernel: elem(base, k) = base + (k >> 1) 1024 + 2 tid + (k & 1)."""
    tile, o = divmod(i, TILE)
    hi, lo = divmod(o, 2 * CA_T)
    tid = lo // 2
    return tile, tid, tid // 64, 2 * hi + (lo & 1)


def cpg_of(mA):
    return (mA + 15) >> 4


# ------------------------------------------------------------------------------------------------------------------- family K
K_ROWS, K_Q = 40, 3
K_SIZES = (1030, 4095, 4096, 4097, 8193)
K_HITS = (0, 1, 126, 127, 128, 129, 1022, 1023, 1024, 1025, 4094, 4095, 4096)
KCase = namedtuple("KCase", "name n inst note")        # inst = (J, C, mu, A, x, g, xlow, xupp, delta)


def k_hits(n):
    return [i for i in K_HITS if i < n - 1] + [n - 1]


def _k_exact(n, order):
    return rc.exact_instance(K_ROWS, n, K_Q, len(order) + 1, order=order)


def tie_states(inst, first, second, theta):
    """phi' (a Fraction) right after the tie at theta, with `first` fixed and `second` still free, and the other way round — for an
    instance whose only moving variables are the two (d = 1 for both)."""
    J, C, mu = inst[:3]
    Jt = np.vstack([J, C])
    wts = np.ones(Jt.shape[0])
    wts[J.shape[0]:] = mu
    cols = Jt[:, [first, second]]
    G2 = cols.T @ (wts[:, None] * cols)                              # 2 x 2, dyadic: exact
    d = [Fraction(float(-inst[5][first])), Fraction(float(-inst[5][second]))]
    Gd = [Fraction(float(G2[k, 0])) * d[0] + Fraction(float(G2[k, 1])) * d[1] for k in (0, 1)]
    th = Fraction(theta)
    return (th * Gd[1] - d[1]) * d[1], (th * Gd[0] - d[0]) * d[0], Gd, d


def _tie(n, first, second):
    """A tie whose ORDER shows.  On exact data two breakpoints at one theta commute — whichever goes first, the other follows at
    theta = 0 and the state behind both is the same bits — unless the search ends between them.  Only `first` < `second` move
    (d_i = 1, 1/2 or 1/4, every other g = 0), both meet their bound at theta, and theta is chosen between the two thresholds
    d_i / (G d)_i, below the minimiser d'd / d'Gd of pass 0: with one of the two fixed phi' >= 0 and the search ends there (2 passes, one variable
    fixed), with the other fixed phi' < 0 and it goes on (3 passes, both fixed).  Which one the reference fixes first — the smaller
    index (:555 is a strict <) — decides the active set and the pass count."""
    J, C, mu, A, x, _, xlow, _, delta = _k_exact(n, [])
    for da, db in ((1.0, 1.0), (1.0, 0.5), (0.5, 1.0), (1.0, 0.25), (0.25, 1.0)):       # the first pair of lengths whose thresholds differ
        g = np.zeros(n)
        g[first], g[second] = -da, -db
        _, _, Gd, d = tie_states((J, C, mu, A, x, g), first, second, 0.0)
        if not (Gd[0] > 0 and Gd[1] > 0 and d[0] / Gd[0] != d[1] / Gd[1]):
            continue
        lo, star = min(d[0] / Gd[0], d[1] / Gd[1]), (d[0] * d[0] + d[1] * d[1]) / (d[0] * Gd[0] + d[1] * Gd[1])
        theta = Fraction(int(lo * 1024) + 1, 1024)                   # the first multiple of 2^-10 above the lower threshold
        if lo < theta < star:
            xupp = 1024.0 * np.ones(n)
            xupp[first], xupp[second] = float(theta) * da, float(theta) * db
            return J, C, mu, A, x, g, xlow, xupp, delta
    raise AssertionError("no order-sensitive tie for (%d, %d) at n = %d" % (first, second, n))


def k_cases(n):
    """The searches of family K at width n (all end at an interior minimiser unless the name says otherwise)."""
    hits = k_hits(n)
    out = [KCase("ascending", n, _k_exact(n, hits), "hits %s in ascending order" % hits),
           KCase("descending", n, _k_exact(n, hits[::-1]), "the same hits, last index first"),
           KCase("interleaved", n, _k_exact(n, hits[::2] + hits[1::2][::-1]), "even positions upwards, then odd positions downwards")]
    out.append(KCase("tie_2_1024", n, _tie(n, 2, 1024), "thread 1's first element against thread 0's third, met in the wave: 2 goes first"))
    out.append(KCase("tie_127_128", n, _tie(n, 127, 128), "across waves 0 | 1"))
    out.append(KCase("tie_0_1024", n, _tie(n, 0, 1024), "inside thread 0: its first element against its third (the strict < of the per-thread scan)"))
    if n > TILE:
        out.append(KCase("tie_0_4096", n, _tie(n, 0, 4096), "inside thread 0, across its tiles 0 | 1"))
        out.append(KCase("tie_4095_4096", n, _tie(n, 4095, 4096),
                         "across tiles 0 | 1" + (": 4096 is the one element of the last tile" if n == TILE + 1 else "")))
    if n in (1030, 4097):
        J, C, mu, A, x, g, xlow, xupp, delta = _k_exact(n, hits)
        g = np.where(xupp < 1024.0, g, 0.0)                          # only the bounded variables move: d = 0 once all are fixed
        out.append(KCase("ends_at_phi_p_0", n, (J, C, mu, A, x, g, xlow, xupp, delta), "d = 0 after the last breakpoint: phi' = 0 >= 0"))
        out.append(KCase("stationary", n, (J, C, mu, A, x, np.zeros(n), xlow, xupp, delta), "g = 0: phi' = 0 >= 0 at pass 0"))
    return out


def k_all_fixed():
    """block_cases.all_fixed: every variable fixed, the search ends on nfix == nmm after n + 1 passes."""
    out = []
    for n, rows in ((6, 5), (9, 7)):
        J, C, mu, x, g, xlow, xupp, delta = bc.all_fixed(n, rows)
        out.append(KCase("all_fixed_n%d" % n, n, (J, np.zeros((0, n)), mu, np.zeros((0, n)), x, g, xlow, xupp, delta), "nfix == nmm"))
    return out


def k_no_breakpoint(n):
    """block_cases.no_breakpoint at width n: J = 0, infinite bounds and trust region — phi' < 0, phi'' = 0, ind < 0 at pass 0."""
    g = -(2.0 ** -(np.arange(n) % 3).astype(np.float64))
    return KCase("no_breakpoint", n, (np.zeros((4, n)), np.zeros((0, n)), 0.0, np.zeros((0, n)), np.zeros(n), g, -np.inf * np.ones(n),
                                      np.inf * np.ones(n), np.inf), "ind < 0: the error flag")


# ------------------------------------------------------------------------------------------------------------------- family E
E_ROWS, E_Q, E_PASSES = 96, 8, 6
E_CASES = [(300, 1, 6), (300, 16, 6), (300, 17, 6), (300, 33, 6), (300, 64, 6), (271, 64, 6), (272, 64, 6), (273, 64, 6), (4100, 64, 6),
           (300, 3, 130)]


def e_instance(n, mA, npass):
    """Past one 4096-column panel the first seed is taken whose A has an entry in the columns behind it on a variable that stays
    free: only then does the K-tail of image_b_mfma_kernel add something to B."""
    for seed in range(64):
        inst = rc.exact_equality_instance(E_ROWS, n, E_Q, npass, mA, per_row=4, seed=seed, theta_exp=14 if npass - 1 > 127 else 13)
        if n <= MFMA_PANEL or inst[3][:, MFMA_PANEL:].any():
            return inst
    raise AssertionError("no seed places an equality in the K-tail")


def describe_e(n, mA, npass):
    cpg = cpg_of(mA)
    past = [(grp, k) for grp in range(16) for k in range(cpg) if grp * cpg + k >= mA]
    return ("E  n=%-5d mA=%-2d cpg %d, %d (group, k) slots past mA; %d blocks of 16, the last with %d element(s); %d passes, a and B formed %d "
            "time(s)%s" % (n, mA, cpg, len(past), -(-n // EQ_BLOCK), n - (n - 1) // EQ_BLOCK * EQ_BLOCK, npass, 1 + (npass - 1) // EQ_REFRESH,
                           "; K-tail of %d columns past the %d-column panel" % (rs.ld_of(n) - MFMA_PANEL, MFMA_PANEL) if n > MFMA_PANEL else ""))


# --------------------------------------------------------------------------------------------- the search from G, through the ledger
def gram_matrix(inst, led):
    """matrix_info of G = J'J + mu C'C of an instance; every entry is a sum of `rows` products w_r J_ri J_rj (the bound noted)."""
    J, C, mu = inst[:3]
    Jt = np.vstack([J, C]) if C is not None and C.shape[0] else J
    wts = np.ones(Jt.shape[0])
    wts[J.shape[0]:] = mu
    eJ = dyadic_exp(Jt)
    led.note("G", Jt.shape[0] * int(units(Jt, eJ).max(initial=0)) ** 2 * max(1, int(units([mu], dyadic_exp([mu]))[0])))
    return matrix_info(Jt.T @ (wts[:, None] * Jt))


def gram_search_model(inst, led, refresh=EQ_REFRESH, log=None, M=None):
    """cauchy_step (src/basic_tralcnlss.jl:574-639) as the Gram-form kernels compute it, every operation through the ledger.
    Box constraints (no rows in A): Hd = G d once, then Hd -= d_ind G[ind, :] per breakpoint (cauchy_gram_kernel).  Equalities:
    y = (A_free A_free')^-1 A_free (-g), d = -D g - D A'y, a = G D g, B = G D A', Hd = -a - B y, a and B carried over a breakpoint
    by one row of G and formed again at every pass index that is a positive multiple of `refresh` (cauchy_gram_eq_kernel); the
    carried and the re-formed a, B must be the same bits.  Returns (s, active set, passes, err)."""
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    n = J.shape[1]
    M = gram_matrix(inst, led) if M is None else M
    G = M["dense"]
    mA = A.shape[0]
    fix = ((x - xlow) <= SQRT_EPS) | ((xupp - x) <= SQRT_EPS)
    d_u, d_l = np.minimum(xupp - x, delta), np.maximum(xlow - x, -delta)
    s = np.zeros(n)

    def direction():
        free = ~fix
        if mA == 0:
            return np.where(free, -g, 0.0), None
        Af = A * free[None, :]
        AAt = Af @ Af.T
        per_row = AAt[0, 0]
        assert np.array_equal(AAt, per_row * np.eye(mA)) and per_row in (4.0, 16.0)       # the factor is sqrt(per_row) I: exact
        y = np.array([led.quotient(led.dot(Af[r], -g, "A (-g)"), per_row, "y") for r in range(mA)])
        assert np.all((Af != 0).sum(axis=0) <= 1)                    # A'y: one product per component
        Aty = Af.T @ y
        return np.where(free, led.axpy(-1.0, Aty, -g, "d"), 0.0), y

    def form_ab():
        free = ~fix
        a = led.matvec(M, np.where(free, g, 0.0), "a = G D g")
        B = np.stack([led.matvec(M, np.where(free, A[j], 0.0), "B = G D A'") for j in range(mA)], axis=1)
        return a, B

    d, y = direction()
    if mA == 0:
        Hd = led.matvec(M, d, "Hd")
    else:
        a, B = form_ab()
    passes, err, ind = 0, 0, -1
    while True:
        if mA:
            if passes > 0 and passes % refresh == 0:
                a2, B2 = form_ab()
                assert np.array_equal(a2.view(np.uint64), a.view(np.uint64)) and np.array_equal(B2.view(np.uint64), B.view(np.uint64))
                a, B = a2, B2
                if log is not None:
                    log.append(passes)
            Hd = led.affine(a, B, y, "Hd = -a - B y")
        shd = led.dot(s, Hd, "s'Hd")
        dhd = led.dot(d, Hd, "d'Hd")
        gd = led.dot(g, d, "g'd")
        phi_p = shd + gd
        assert Fraction(phi_p) == Fraction(shd) + Fraction(gd)
        phi_pp = dhd
        free = ~fix
        # next_breakpoint (:536-562): the numerators d_u - s_c, d_l - s_c are exact; a quotient that becomes a step is exact too
        # (checked where the step is taken; the others are single correctly rounded quotients of exact operands and are only
        # compared); first index on a tie
        theta, ind = math.inf, -1
        live = np.flatnonzero(free & (d != 0.0))
        if live.size:
            bnd = np.where(d[live] > 0, d_u[live], d_l[live])
            fin = np.isfinite(bnd)
            led.axpy(-1.0, s[live][fin], bnd[fin], "d_u - s_c")
            with np.errstate(over="ignore"):
                t = (bnd - s[live]) / d[live]
            k = int(np.argmin(t))
            if t[k] < math.inf:
                theta, ind, theta_num = float(t[k]), int(live[k]), float(bnd[k] - s[live[k]])
        passes += 1
        if not (int(fix.sum()) < n - mA):
            break
        if phi_p >= 0:
            break
        delta_t = (-phi_p / phi_pp) if phi_pp > 0 else 0.0           # the one correctly rounded quotient
        if phi_pp > 0 and delta_t < theta:
            s = s + delta_t * d                                      # product, then sum: __dmul_rn, __dadd_rn
            break
        if ind < 0:
            err = 1
            break
        led.quotient(theta_num, float(d[ind]), "theta")             # a theta that becomes a step is exact
        s = led.axpy(theta, d, s, "s")
        if mA == 0:
            Hd = led.axpy(-d[ind], G[ind], Hd, "Hd downdate")
        else:
            a = led.axpy(-g[ind], G[ind], a, "a downdate")
            for j in range(mA):
                if A[j, ind] != 0.0:
                    B[:, j] = led.axpy(-A[j, ind], G[ind], B[:, j], "B downdate")
        fix[ind] = True
        d, y = direction()
    return s, fix, passes, err
