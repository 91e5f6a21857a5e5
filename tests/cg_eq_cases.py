"""Exact instances for the CG loop WITH LINEAR EQUALITIES on an implicit handle (helper of tests/test_cg_eq_exact_gpu.py, proved on
the CPU by tests/test_cg_eq_cases_cpu.py).  Not a test.

    cg_reduce_update_kernel<GEN = true> + proj_apply_linv_kernel<INIT>   cg_fused = 1   (csrc/bh_cgfuse_body.hip.h, bh_proj.hip.h)
    ... + trsv_small_kernel + proj_left_mul_tr_kernel<true, 4>           cg_fused = 2
    cg_step kernels, left_mul, trsv, left_mul_tr (seven kernels)         cg_fused = 0, proj_form 1 | 0, and every mA > 64
    cg_reduce_update_compact_kernel                                      free_image_eq = 1, free_image = 2
    gram_cg_kernel, its equality arm                                     a Gram-form handle, gram_cg_fused = 1

Family EC2 is C2 of tests/gram_cases.py with equalities that do not commute with H.  lam = 16, J = 4 I_n, C = q', mu = 3 lam / mt.

  A     mA rows of four entries +-1 on disjoint supports that touch no fixed variable: A_free A_free' = 4 I, the factor is 2 I, the
        explicit inverse I / 2, the refinement residual exactly zero, P = I - A'A / 4; augmented: B B' = diag(4 I, I).
  q     on a support the row's own sign on two of its four entries and 0 on the other two (a.q = 2); +-1 on Q further free
        variables; 0 elsewhere.  qt = P q = q - a / 2 has entries +-1/2 on the supports and |qt|^2 = mA + Q = mt.
  u     2 (q_j e_i - q_i e_j) on mt / 4 pairs of the Q outside indices: |u|^2 = 2 mt, u orthogonal to qt, A u = 0.
  g     u + c qt + A'z, c = +-1, z half-integers in [-3/2, 3/2] without a zero (the part every projection must remove); two
        variables are fixed with g = 1.

P H P qt = 4 lam qt and H u = lam u, so as in C2: alpha_1 = alpha_2 = 1/32, beta = 1/2, pHp = 6 lam mt, 3 lam mt, r.v = 3 mt / 2, 0,
iters 3.  But H p_1 has a component in range(A') (A q != 0): the projection removes A'z in iteration 1 and A'z - (3 c / 2)(q - qt)
in iteration 2, so a y, a partial of A_free r or an explicit inverse left over from the iteration before gives other bits.

mt is the smallest power of two >= 2 (mA + the deciding indices kept outside the supports) (so Q - mt / 2 outside indices stay
free of u: the deciding ones); the T instance takes the smallest 3 4^k >= 2 mA + 8 instead.

Cases (the decision edges of tests/cg_rows_cases.py, on EC2):
  tie / half   one finite bound on a deciding index i with gamma_2 == alpha_2 (inside: :735 is a strict >, solved, iters 3) or
               alpha_2 / 2 (bound_hit, iters 2), from w_u and from w_l, for i outside every support (p_i through the mask only) and
               inside one (p_i through left_mul_tr).
  T            mt = 3 4^k: |v_1| = 3 2^k, kappa2 = |v_1| / 2 makes |r.v| == tol_cg after iteration 1: goes on (iters 3);
               nextafter(kappa2, +inf) stops (iters 2).
  N            atol = pHp_2: negative_curvature in iteration 2, w = w_1; nextafter(pHp_2, 0): runs on; atol = pHp_1: w = 0.
  EC2n         mu = -2 lam / mt: pHp_1 = lam mt, alpha_1 = 3/16, pHp_2 = -72 lam mt — a step to the one bound at gamma = 2^-4.

Sizes and what each alone reaches (nblk = ceil(ld / 32) partial blocks of A_free r, per = ceil(nblk / 4) per wave of
proj_apply_linv_kernel, which takes them in batches of 32):
  100    geometry 0; 4 blocks, the last of 8 chunks; per = 1; one projection workgroup; every stream workgroup owns several runs
  2047   odd, ld = 2048: 64 full blocks, per = 16; geometry 3
  2050   ld = 2064: 65 blocks (half a block of padding behind n), per = 17: the last quarter is short; geometry 4
  4096   n == ld: 128 blocks, per = 32, exactly one full batch; device pointers used in place
  4099   129 blocks, per = 33: the second batch runs once, for one block; odd n: column n - 1 is half a chunk; geometry 5
  8200   257 blocks, per = 65: three batches; geometry 6; cg_step_kernel (vectors not in registers) in the separate shape
mA: 1 (scalar factor, no refinement by rule), 16 (the row slots rl + 16 k exactly full at k = 0), 17 (one row in k = 1), 33,
64 (every slot of the explicit inverse), 65 (separate shape, blocked factor).  n = 100 holds 98 free variables, fewer than the
4 mA + Q an instance with mA >= 16 needs: it takes mA = 1 and, so that the width also runs a factor of
several rows, mA = 3.  Every other size takes all six.  With mA = 1 the four entries of A sit in column 0, in column n - 1, in the last
block of quarter 0 and in the first block of quarter 1; every larger mA covers every block of wanted_blocks."""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

import benlsip_ref as R
import cg_rows_cases as cr
import gram_cases as gc
import rs_cases as rs

LAM = gc.LAM
SIZES = (100, 2047, 2050, 4096, 4099, 8200)
MAS = (1, 16, 17, 33, 64, 65)
TABLE = ((100, 1), (100, 3)) + tuple((n, mA) for n in SIZES[1:] for mA in MAS)
T_TABLE = ((100, 1), (2047, 17), (2050, 17), (2050, 65), (4096, 17), (4099, 17), (4099, 64), (8200, 17))     # mt = 12, 48, 192
UPD_CHUNKS = 16                  # chunks (of two columns) per workgroup of cg_reduce_update_kernel: one partial block of A_free r
PRJ_CHUNKS = 64                  # chunks per workgroup of proj_apply_linv_kernel
PRJ_BATCH = 32                   # partial blocks a wave of proj_apply_linv_kernel loads at once
BLOCK = 2 * UPD_CHUNKS           # columns of a partial block


# ------------------------------------------------------------------------------------------------------------------ geometry
def eq_geometry(n, n_cu, bpc):
    """The stream grid of the implicit handle (nrows = n + 1: cg_rows_cases.rows_geometry of C2) and the blocks of the two
    projection-side kernels."""
    geo = cr.rows_geometry("C2", n, n_cu, bpc)
    geo.update(block_geometry(n))
    return geo


def block_geometry(n):
    nch = rs.ld_of(n) // 2
    nblk = -(-nch // UPD_CHUNKS)
    per = (nblk + 3) // 4
    quarters = [(rg * per, min(nblk, rg * per + per)) for rg in range(4)]
    return dict(nch=nch, nblk=nblk, per=per, quarters=quarters, batches=max(-(-(b1 - b0) // PRJ_BATCH) for b0, b1 in quarters),
                nprj=-(-nch // PRJ_CHUNKS))


def eq_placements(n, n_cu, bpc):
    """[(index, edge)]: the edge list of gram_cases.placements_of on the stream grid of the implicit handle."""
    return cr.rows_placements("C2", n, n_cu, bpc)


@functools.lru_cache(maxsize=None)
def eq_reserved(n):
    """Every deciding index any design grid places at width n (sorted tuple)."""
    return tuple(sorted({i for n_cu in gc.N_CU_DESIGN for bpc in gc.cg_grids(n) for i, _ in eq_placements(n, n_cu, bpc)}))


def wanted_blocks(n):
    """The partial blocks some row of A must touch, in order of priority: the first and the last block of every quarter a wave of
    proj_apply_linv_kernel folds, then the first block of every further batch of quarter 0 (block 32 at n = 4099, where it is
    also the quarter's last; 32 and 64 at n = 8200).  Past n = 4096 the last block of quarter 3 is a block >= 128."""
    bg = block_geometry(n)
    out = []
    for b0, b1 in bg["quarters"]:
        if b0 < b1:
            out += [b0, b1 - 1]
    b0, b1 = bg["quarters"][0]
    out += [b for b in range(b0 + PRJ_BATCH, b1, PRJ_BATCH)]         # the first block of every further batch of quarter 0
    seen, uniq = set(), []
    for b in out:
        if b not in seen:
            seen.add(b)
            uniq.append(b)
    return uniq


# ---------------------------------------------------------------------------------------------------------------- instances
EqInstance = namedtuple("EqInstance", "kind n mA lam mt Q diag q qt u z S sign fix g0 inside outside")


def _mt_of(kind, mA, n_out):
    if kind == "T":
        mt = 12
        while mt < 2 * mA + 8:
            mt *= 4
        return mt
    return 1 << (2 * (mA + max(n_out, 4)) - 1).bit_length()


@functools.lru_cache(maxsize=None)
def eq_instance(n, mA, kind="EC2"):
    """The shared part of EC2 (kind "EC2": mt a power of two, the deciding indices reserved) or of T (mt = 3 4^k, no deciding
    index) at (n, mA).  S, sign: the supports of A (mA x 4 columns, ascending) and their signs.  inside / outside: the deciding
    indices that sit in a support / in none.  Read-only, built once."""
    rng = np.random.default_rng(7000 + 97 * n + mA + (500000 if kind == "T" else 0))
    reserved = eq_reserved(n) if kind == "EC2" else (0, n - 1)
    fixed = gc._spare(n, 2, set(reserved))
    fix = np.zeros(n, dtype=bool)
    fix[fixed] = True
    blk = lambda j: j // BLOCK
    # ---- which columns A must hold, in order of priority; what does not fit 4 mA entries is left out (mA = 1 holds four)
    wanted = [0, n - 1]
    for b in wanted_blocks(n):
        if b in (blk(0), blk(n - 1)):
            continue
        j = b * BLOCK + 5
        while j in reserved or fix[j]:
            j += 1
        assert blk(j) == b and j < n
        wanted.append(j)
    others = [i for i in reserved if i not in (0, n - 1)]
    wanted += others[1::2]                                           # every second deciding index goes inside a support
    wanted = wanted[:4 * mA]
    rows = [[] for _ in range(mA)]
    ptr = 0
    for j in wanted:                                                 # round robin, never two entries of a row in one block
        for t in range(mA):
            r = (ptr + t) % mA
            if len(rows[r]) < 4 and all(blk(k) != blk(j) for k in rows[r]):
                rows[r].append(j)
                ptr = r + 1
                break
        else:
            raise AssertionError("no row takes column %d at n = %d, mA = %d" % (j, n, mA))
    inside = tuple(sorted(i for i in reserved if any(i in r for r in rows)))
    outside = tuple(i for i in reserved if i not in inside)
    taken = set(reserved) | set(fixed) | {j for r in rows for j in r}
    spare = [int(j) for j in rng.permutation(n) if j not in taken]
    for r in rows:                                                   # fill up from the spare columns, in other blocks
        k = 0
        while len(r) < 4:
            j = spare[k]
            if all(blk(j) != blk(i) for i in r):
                r.append(spare.pop(k))
            else:
                k += 1
    S = np.array([sorted(r) for r in rows], dtype=np.int64)
    sign = rng.choice([-1.0, 1.0], size=(mA, 4))
    assert len(set(S.ravel().tolist())) == 4 * mA and not fix[S].any()
    # ---- q, qt
    mt = _mt_of(kind, mA, len(outside))
    Q = mt - mA
    assert len(spare) >= Q - len(outside), (n, mA, mt)
    out_idx = list(outside) + spare[:Q - len(outside)]               # the deciding ones first: u lives on the others
    q = np.zeros(n)
    q[out_idx] = rng.choice([-1.0, 1.0], size=Q)
    qt = q.copy()
    for r in range(mA):
        two = rng.permutation(4)[:2]
        q[S[r, two]] = sign[r, two]
        qt[S[r]] = -sign[r] / 2.0
        qt[S[r, two]] = sign[r, two] / 2.0
    # ---- u on the outside indices that decide nothing
    upairs = out_idx[len(outside):len(outside) + mt // 2]
    assert len(upairs) == mt // 2 and mt % 4 == 0
    u = np.zeros(n)
    for a in range(mt // 4):
        i, j = upairs[2 * a], upairs[2 * a + 1]
        u[i], u[j] = 2.0 * q[j], -2.0 * q[i]
    z = rng.choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], size=mA)
    g0 = u.copy()
    for r in range(mA):
        g0[S[r]] += sign[r] * z[r]
    g0[fix] = 1.0
    diag = np.full(n, math.sqrt(LAM))
    for arr in (diag, q, qt, u, z, S, sign, fix, g0):
        arr.setflags(write=False)
    return EqInstance(kind, n, mA, LAM, mt, Q, diag, q, qt, u, z, S, sign, fix, g0, inside, outside)


def dense_A(inst):
    A = np.zeros((inst.mA, inst.n))
    for r in range(inst.mA):
        A[r, inst.S[r]] = inst.sign[r]
    return A


def dense_J(inst):
    """J = 4 I in column-major order (symmetric: the library takes it as it stands)."""
    J = np.zeros((inst.n, inst.n), order="F")
    J[np.arange(inst.n), np.arange(inst.n)] = inst.diag
    return J


def mu_of(inst, family="EC2"):
    return (-2.0 if family == "EC2n" else 3.0) * LAM / inst.mt


def factor_aug(inst):
    """The reference's augmented factor of B B' = diag(4 I, I) (exact: a diagonal of 2s and 1s)."""
    cons = R.make_mixed_constraints(dense_A(inst), R.chol_lower(4.0 * np.eye(inst.mA)), inst.fix)
    return cons.chol_L


# -------------------------------------------------------------------------------------------------------------------- cases
EqCase = namedtuple("EqCase", "group kind_of_instance n mA index kind side edge inside g w_l w_u kappa2 atol mu")


def _g(inst, c):
    g = inst.g0 + c * inst.qt
    g[inst.fix] = 1.0
    return g


def _unbounded(n):
    return np.full(n, -np.inf), np.full(n, np.inf)


def placed_case(inst, index, kind, side, edge=""):
    """One bounded case: p_2,i = c qt_i / 2 > 0 is stopped by w_u (side "upper"), < 0 by w_l."""
    qi = inst.qt[index]
    assert abs(qi) == (0.5 if index in inst.inside else 1.0) and inst.u[index] == 0.0 and not inst.fix[index]
    want = 1.0 if side == "upper" else -1.0
    c = want * math.copysign(1.0, qi)
    alpha = 1.0 / (2.0 * LAM)
    p1, p2 = -c * qi, c * qi / 2.0
    assert math.copysign(1.0, p2) == want
    gamma2 = alpha if kind == "tie" else alpha / 2.0
    w_l, w_u = _unbounded(inst.n)
    (w_u if side == "upper" else w_l)[index] = alpha * p1 + gamma2 * p2          # w_1,i + gamma_2 p_2,i: dyadic, exact
    return EqCase("EC2", "EC2", inst.n, inst.mA, index, kind, side, edge, index in inst.inside, _g(inst, c), w_l, w_u, gc.KAPPA2, gc.SQRT_EPS,
                  mu_of(inst))


def placed_cases(n, mA, n_cu, bpc):
    """Every placement of (n, grid) once as a tie and once as a half step; the side alternates within the placements inside a
    support and within those outside, so that w_l and w_u decide in both kinds in both classes."""
    inst = eq_instance(n, mA)
    out, rank = [], {True: 0, False: 0}
    for i, edge in eq_placements(n, n_cu, bpc):
        k = rank[i in inst.inside]
        rank[i in inst.inside] += 1
        out.append(placed_case(inst, i, "tie", ("upper", "lower")[k % 2], edge))
        out.append(placed_case(inst, i, "half", ("lower", "upper")[k % 2], edge))
    return out


def short_case(n, mA):
    """A one-iteration call for the same handles: the bound of variable 0 (inside a support) is met at gamma_1 = alpha_1 / 2."""
    inst = eq_instance(n, mA)
    p1 = -inst.qt[0]                                                 # c = 1
    w_l, w_u = _unbounded(n)
    (w_u if p1 > 0 else w_l)[0] = (1.0 / (4.0 * LAM)) * p1
    return EqCase("EC2", "EC2", n, mA, 0, "short", "upper" if p1 > 0 else "lower", "one iteration", True, _g(inst, 1.0), w_l, w_u, gc.KAPPA2,
                  gc.SQRT_EPS, mu_of(inst))


def t_cases(n, mA):
    """Family T on its own instance (mt = 3 4^k): no bounds; kappa2 = |v_1| / 2 (the tie: goes on) and its upper neighbour."""
    inst = eq_instance(n, mA, "T")
    s = math.isqrt(3 * inst.mt)
    assert s * s == 3 * inst.mt
    kappa2 = s / 2.0
    w_l, w_u = _unbounded(n)
    mk = lambda kind, edge, k2: EqCase("T", "T", n, mA, -1, kind, "", edge, False, _g(inst, 1.0), w_l, w_u, k2, gc.SQRT_EPS, mu_of(inst))
    return [mk("tie", "|r.v| == tol_cg after iteration 1", kappa2),
            mk("above", "tol_cg one ulp of kappa2 above |r.v|", float(np.nextafter(kappa2, np.inf)))]


def n_cases(n, mA):
    """Family N on the instance of EC2: no bounds, c = 1; atol is the operand."""
    inst = eq_instance(n, mA)
    pHp1 = 6.0 * LAM * inst.mt
    pHp2 = pHp1 / 2.0
    w_l, w_u = _unbounded(n)
    mk = lambda kind, edge, atol: EqCase("N", "EC2", n, mA, -1, kind, "", edge, False, _g(inst, 1.0), w_l, w_u, gc.KAPPA2, atol, mu_of(inst))
    return [mk("at2", "atol == pHp_2: negative curvature, w_1 untouched", pHp2),
            mk("below2", "atol one ulp below pHp_2: two iterations", float(np.nextafter(pHp2, 0.0))),
            mk("at1", "atol == pHp_1: negative curvature at once, w = 0", pHp1)]


def ec2n_case(inst, index, side, edge=""):
    qi = inst.qt[index]
    want = 1.0 if side == "upper" else -1.0
    c = -want * math.copysign(1.0, qi)                               # p_2,i = -12 c qt_i
    w1, p2 = (3.0 / LAM) * (-c * qi), -12.0 * c * qi
    assert math.copysign(1.0, p2) == want and inst.u[index] == 0.0
    w_l, w_u = _unbounded(inst.n)
    (w_u if side == "upper" else w_l)[index] = w1 + 2.0 ** -4 * p2
    return EqCase("EC2n", "EC2", inst.n, inst.mA, index, "neg", side, edge, index in inst.inside, _g(inst, c), w_l, w_u, gc.KAPPA2, gc.SQRT_EPS,
                  mu_of(inst, "EC2n"))


def ec2n_cases(n, mA, n_cu, bpc):
    """Every placement, from both sides."""
    inst = eq_instance(n, mA)
    return [ec2n_case(inst, i, side, edge) for i, edge in eq_placements(n, n_cu, bpc) for side in ("upper", "lower")]


def instance_of(case):
    return eq_instance(case.n, case.mA, case.kind_of_instance)


# ------------------------------------------------------------------------------------------------------------------ the oracle
@functools.lru_cache(maxsize=8)
def _oracle_cons(n, mA, kind):
    inst = eq_instance(n, mA, kind)
    A = dense_A(inst)
    return R.make_mixed_constraints(A, R.chol_lower(A @ A.T), inst.fix)


def structured_hmul(inst, mu):
    """benlsip_ref.hmul for the diagonal J of an instance, operation by operation (J v, (mu C) v, J'(J v) + C'(mu C v)), without
    the n x n array; tests/test_cg_eq_cases_cpu.py holds it to hmul on the dense J."""
    C = inst.q.reshape(1, -1)
    muC = mu * C

    def hmul(H, v):
        Jv = inst.diag * v
        return inst.diag * Jv + C.T @ (muC @ v)
    return hmul


def eq_oracle(case, hmul_fn=None, H=None):
    """The oracle's projected_cg on a case (the augmented projection with the reference's own factor): (w, status, iters, trace
    rows)."""
    inst = instance_of(case)
    cons = _oracle_cons(case.n, case.mA, case.kind_of_instance)
    tr = R.CGTrace()
    w, st, it = R.projected_cg(case.g, H, case.w_l, case.w_u, cons, case.kappa2, atol=case.atol,
                               hmul_fn=structured_hmul(inst, case.mu) if hmul_fn is None else hmul_fn, trace=tr)
    return w, int(st), int(it), np.array(tr.rows).reshape(-1, 4)


# -------------------------------------------------------------------------------------------------------------------- the model
def _mul(led, a, b, what):
    """cg_rows_cases._mul; a faulted model (cg_rows_cases.Unchecked) need not stay dyadic and is only multiplied."""
    if isinstance(led, cr.Unchecked):
        return np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    return cr._mul(led, a, b, what)


def eq_model(inst, case, led, geo=None, fault=None, fault_block=None, atol_f2b=1e-10):
    """projected_cg (src/basic_tralcnlss.jl:690-764) as the kernels of the equality loop form it, every operation through the
    ledger: t = J p, c = C p, pHp = sum t^2 + mu c^2 (and dot(p, Hp): the same bits), Hp = J't + C'(mu c); the projection as
    the per-block partials of A_free r, their sum, u = Linv t, y = Linv'u, v = r - A'y on the free variables; r.v, v.v.  The
    augmented form's operands (B r, the solve with diag(2 I, I), B'y) are formed next to it and must give the same v.
    Returns (w, status, iters, trace rows).

    fault (the sensitivity check; geo names the stream grid): "ge" alpha >= gamma for :735, "le_tol" <= for :747, "drop_block"
    the partial block `fault_block` of A_free r is left out, "stale_y" the projections of the loop reuse the y of the one before,
    "drop_last_run" every stream workgroup leaves the last run it owns out of gamma."""
    n, mA, S, sign, fix = inst.n, inst.mA, inst.S, inst.sign, inst.fix
    g, w_l, w_u, mu = case.g, case.w_l, case.w_u, case.mu
    free = ~fix
    blk = S // BLOCK
    Cq = inst.q
    state = {"y": None}

    def project(r, first):
        rm = np.where(free, r, 0.0)
        t = np.zeros(mA)
        for i in range(mA):
            keep = np.ones(4, dtype=bool) if fault != "drop_block" or first else blk[i] != fault_block
            t[i] = led.dot(sign[i][keep], rm[S[i][keep]], "A_free r")                     # slabs, blocks, quarters: every partial sum
        uu = _mul(led, 0.5, t, "Linv t")
        y = _mul(led, 0.5, uu, "Linv'u")
        if fault == "stale_y" and not first and state["y"] is not None:
            y, state["y"] = state["y"], y
        else:
            state["y"] = y
        Aty = np.zeros(n)
        Aty[S.ravel()] = _mul(led, sign, y[:, None], "A'y").ravel()                   # one product per component
        v = np.where(free, led.axpy(-1.0, Aty, r, "v = r - A'y"), 0.0)
        # the augmented form: B r = [A r; r_fix], y = [t / 4; r_fix], v = r - B'y
        ta = np.array([led.dot(sign[i], r[S[i]], "A r") for i in range(mA)])
        ya = _mul(led, 0.25, ta, "(L L')^-1 B r")
        Btya = np.zeros(n)
        Btya[S.ravel()] = _mul(led, sign, ya[:, None], "B'y").ravel()
        Btya[fix] = r[fix]
        va = led.axpy(-1.0, Btya, r, "v = r - B'y")
        if fault is None:
            assert np.array_equal((va + 0.0).view(np.uint64), (v + 0.0).view(np.uint64)), "the two projection forms differ"
        return v

    w = np.zeros(n)
    r = g.copy()
    v = project(r, True)
    rtv = led.dot(r, v, "r.v")
    p = -v
    tol_cg = case.kappa2 * math.sqrt(led.dot(v, v, "v.v"))
    it, max_iter = 1, 2 * (int(free.sum()) - mA)
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
        t = _mul(led, inst.diag, p, "t = J p")
        c = led.dot(Cq, p, "c = C p")
        pHp = led.dot(t, t, "sum t^2")
        pHp = float(led.axpy(mu, np.array([led.dot(np.array([c]), np.array([c]), "c^2")]), np.array([pHp]), "pHp = sum t^2 + mu c^2")[0])
        Hp = led.axpy(1.0, _mul(led, _mul(led, mu, c, "mu c"), Cq, "C'(mu c)"), _mul(led, inst.diag, t, "J't"), "Hp = J't + C'(mu c)")
        assert led.dot(p, Hp, "dot(p, Hp)") == pHp or fault is not None
        gamma = math.inf
        for i in np.flatnonzero((np.abs(p) >= atol_f2b) & np.isfinite(np.where(p > 0, w_u, w_l)) & seen):
            wb = w_u[i] if p[i] > 0 else w_l[i]
            num = wb - w[i]
            assert Fraction(num) == Fraction(wb) - Fraction(w[i])
            gamma = min(gamma, led.quotient(num, p[i], "gamma"))
        if pHp <= case.atol:                                         # :725
            neg = True
            if abs(pHp) > case.atol:                                 # :727
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
            v = project(r, False)
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
def describe_eq(n, mA, n_cu, bpc):
    """Lines of the case table for one (n, mA, grid)."""
    geo = eq_geometry(n, n_cu, bpc)
    inst = eq_instance(n, mA)
    lines = ["EC2 n=%-5d mA=%-2d blocks_per_cu=%d: mt=%d Q=%d; %d rows, geometry %d (T=%d CPT=%d R=%d) grid %d, %d runs of %d chunks; %d partial "
             "blocks, %d per wave in %d batch(es), %d projection workgroup(s)"
             % (n, mA, bpc, inst.mt, inst.Q, geo["nrows"], geo["path"], geo["T"], geo["CPT"], geo["R"], geo["grid"], geo["nruns"], geo["CPT"],
                geo["nblk"], geo["per"], geo["batches"], geo["nprj"])]
    for i, edge in eq_placements(n, n_cu, bpc):
        wg, run = gc.owner(i, geo)
        lines.append("      i=%-5d run %-4d workgroup %-4d %-7s %s" % (i, run, wg, "inside" if i in inst.inside else "outside", edge))
    return lines
