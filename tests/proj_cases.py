"""Operands and exactly computed results for the null-space projection kernels of csrc/bh_proj.hip.h (pure NumPy and Python
integers, no device, no oracle).  tests/test_proj_cases_cpu.py proves that the cases are what they claim; tests/test_proj_exact_gpu.py
feeds them to the library (bh_left_mul, bh_left_mul_tr, bh_project, bh_project_dev, bh_pcg).

Reduced form (proj_form = 1).  The free columns of A hold A_free = T Q:

* Q: rows picked from a block-diagonal matrix of Sylvester-Hadamard blocks of sizes 64, 16, 4 (and 1 for what is left over) laid
  over the free columns, so Q Q' = D is diagonal with entries 4^k;
* T = Z diag(a) S 1_lower S: unit-lower Z = [[I, 0], [R, I]] with a few small integers in R, a in {1, 2}, S signs, 1_lower the
  lower triangle of ones.  T is a dense integer lower triangle with the positive diagonal a, and
  T^-1 = S (I - shift) S diag(1/a) Z^-1 is sparse and dyadic;
* the fixed columns hold integers in -3..3 and are interleaved with the free ones; r is integer, with large values on the fixed
  components (they must be masked out).

Then M = A_free A_free' = T D T' is an integer matrix, its Cholesky factor is T sqrt(D) exactly, every intermediate of a right-looking
factorisation is an integer, both substitutions, the explicit inverse and v = r_free - A_free' M^-1 A_free r are dyadic numbers of a
few bits: whatever the order of summation, float64 arithmetic is exact (ProjCase.sum_bits holds the proof: the largest sum of
absolute terms of any accumulation in the chain, in units of the granularity of its terms, stays below 2^53).

Augmented form (proj_form = 0).  The kernels compute v = r - B'(L L')^-1 B r with B = [A; E_fix] for WHATEVER lower triangle L the
caller hands over.  These cases hand over L = T sqrt(D) of order mpp = mA + nfix built as above (dense, dyadic, power-of-two diagonal)
next to an arbitrary integer A: their expected value is that formula evaluated exactly.  This is an exact check of the three kernels
(gather, blocked substitution, scatter), not a projector: L L' is not B B'.

The float64 restatements below (restate_reduced, restate_augmented) follow the kernels' orders: right-looking Cholesky with 64-column
panels (potrf / trsm / syrk), column substitutions, the 64-wide blocked substitution with its forward trailing update in four slices
or in one, and the Linv'(Linv t) form.  `tol` of a reduced-form case is 64 x the largest deviation of 32 such runs whose reciprocal
diagonals carry a random factor 1 +- 2^-52 (chol_small_body forms 1 / sqrt(pivot) from the hardware's reciprocal square root and two
Newton steps: exact for the pivots 4^k of these cases if the seed is exact, possibly one unit off if it is not)."""
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

TRSV_LDS_BYTES = 160 * 1024            # kLdsPerCu of csrc/bh_api.hip (checked by the CPU test)


def trsv_split_for(m):
    """csrc/bh_api.hip: the forward trailing update of trsv_pair_kernel runs in four slices while their partials fit the LDS."""
    m2 = (m + 1) & ~1
    return 4 if (5 * m2 + 64 * 65) * 8 <= TRSV_LDS_BYTES else 1


def hadamard(k):
    H = np.ones((1, 1), dtype=np.int64)
    while H.shape[0] < k:
        H = np.block([[H, H], [H, -H]])
    assert H.shape[0] == k
    return H


_H = {k: hadamard(k) for k in (1, 4, 16, 64)}


def block_sizes(nf):
    out = []
    for s in (64, 16, 4, 1):
        out += [s] * (nf // s)
        nf %= s
    return out


def block_rows(nf, rows):
    """Rows `rows` of the block-diagonal Hadamard matrix over nf columns, and the squared norm of each."""
    sizes = block_sizes(nf)
    off = np.concatenate([[0], np.cumsum(sizes)])
    Q = np.zeros((len(rows), nf), dtype=np.int64)
    D = np.zeros(len(rows), dtype=np.int64)
    for i, rho in enumerate(rows):
        b = int(np.searchsorted(off, rho, side="right") - 1)
        Q[i, off[b]:off[b + 1]] = _H[sizes[b]][rho - off[b]]
        D[i] = sizes[b]
    return Q, D


def granularity(*arrays):
    """The largest power of two of which every entry is a multiple (float; 1.0 for all-zero input)."""
    e_min = None
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).ravel()
        a = a[a != 0.0]
        if a.size == 0:
            continue
        mant, ex = np.frexp(np.abs(a))
        mi = np.ldexp(mant, 53).astype(np.int64)
        low = mi & -mi
        e = int((ex - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)).min())
        e_min = e if e_min is None else min(e_min, e)
    return 1.0 if e_min is None else math.ldexp(1.0, e_min)


# ------------------------------------------------------------------------------------------------------------------ T
@dataclass
class Tri:
    """T = Z diag(a) S 1_lower S of order m, in its factors."""
    m: int
    a: np.ndarray
    s: np.ndarray
    R: np.ndarray          # (m - m1) x m1

    @property
    def m1(self):
        return self.R.shape[1]

    def dense(self):
        X = np.tril(np.outer(self.a * self.s, self.s)).astype(np.float64)
        if self.m1 and self.R.any():
            X[self.m1:] += self.R.astype(np.float64) @ X[:self.m1]          # small integers: exact in float64
        return X

    def inv_scaled(self, t):
        """amax * T^-1 t for an integer vector t (int64)."""
        z = np.array(t, dtype=np.int64)
        if self.m1:
            z[self.m1:] -= self.R @ z[:self.m1]
        z = self.s * (z * (int(self.a.max()) // self.a))
        z[1:] = z[1:] - z[:-1].copy()
        return self.s * z

    def inv_t_scaled(self, w):
        """amax * T^-T w."""
        z = self.s * np.array(w, dtype=np.int64)
        z[:-1] = z[:-1] - z[1:].copy()
        z = (self.s * z) * (int(self.a.max()) // self.a)
        if self.m1:
            z[:self.m1] -= self.R.T @ z[self.m1:]
        return z


def make_tri(m, rng):
    m1 = m // 2
    a = 2 ** rng.integers(0, 2, size=m).astype(np.int64)
    s = np.where(rng.random(m) < 0.5, -1, 1).astype(np.int64)
    R = rng.integers(-2, 3, size=(m - m1, m1)).astype(np.int64)
    R[rng.random(R.shape) >= min(1.0, 3.0 / max(m1, 1))] = 0
    return Tri(m, a, s, R)


class Eye:
    """T = I."""

    def __init__(self, m):
        self.m = m
        self.a = np.ones(m, dtype=np.int64)

    def dense(self):
        return np.eye(self.m)

    def inv_scaled(self, t):
        return np.array(t, dtype=np.int64)

    inv_t_scaled = inv_scaled


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclass
class ProjCase:
    name: str
    form: int                          # 1 reduced, 0 augmented
    n: int
    mA: int
    A: np.ndarray                      # mA x n, float64 integers
    fix: np.ndarray                    # n bool
    r: np.ndarray
    tri: object                        # T in its factors (order mA reduced, mpp augmented)
    D: np.ndarray                      # the squares of the factor's column scales (4^k)
    x_lm: np.ndarray = None            # operand of left_mul (n integers)
    y_lmt: np.ndarray = None           # operand of left_mul_tr (mpp integers)
    lm: np.ndarray = None              # expected [A x; x_fix]
    lmt: np.ndarray = None             # expected A'y_A + scatter(y_fix)
    v: np.ndarray = None               # expected projection
    y: np.ndarray = None               # the exact multipliers (M^-1 A_free r, or (L L')^-1 B r)
    granularity: float = 0.0
    sum_bits: float = 0.0              # log2 of the largest sum of |terms| / granularity of the terms, over the whole chain
    gram: tuple = (1,)                 # gram_mfma settings this case runs under (reduced form)
    _L: Optional[np.ndarray] = field(default=None, repr=False)
    _tol: Optional[float] = field(default=None, repr=False)

    def __repr__(self):
        return self.name

    @property
    def nfix(self):
        return int(self.fix.sum())

    @property
    def mpp(self):
        return self.mA + self.nfix

    @property
    def order(self):
        return self.mA if self.form == 1 else self.mpp

    def factor(self):
        """T sqrt(D): the exact Cholesky factor (reduced form), the factor to hand over (augmented form); upper triangle zero."""
        if self._L is None:
            self._L = self.tri.dense() * np.sqrt(self.D.astype(np.float64))[None, :]
        return self._L

    def factor_with_nan(self):
        L = self.factor().copy()
        if L.shape[0] > 1:
            L[np.triu_indices(L.shape[0], 1)] = np.nan
        return L

    @property
    def tol(self):
        if self._tol is None:
            self._tol = perturbation_tol(self)
        return self._tol


def _exact_solve(tri, D, t):
    """(T D T')^-1 t for an integer vector t: (numerator int64 vector, scale) with value = numerator / scale."""
    amax = int(tri.a.max())
    u = tri.inv_scaled(t)
    assert np.all(np.abs(u) < 2 ** 40)
    u = u * (64 // D)
    yn = tri.inv_t_scaled(u)
    assert np.all(np.abs(yn) < 2 ** 60)
    return yn, amax * amax * 64


def _to_float(num, scale):
    out = np.ldexp(num.astype(np.float64), -int(round(math.log2(scale))))
    assert np.array_equal(np.ldexp(out, int(round(math.log2(scale)))).astype(np.int64), num), "not representable"
    return out


def _finish(c, rng):
    """Exact expected outputs and the any-order proof of a case, in integers."""
    n, mA, fix = c.n, c.mA, c.fix
    Ai, ri = c.A.astype(np.int64), c.r.astype(np.int64)
    free = ~fix
    fidx = np.flatnonzero(fix)
    c.x_lm = rng.integers(-9, 10, size=n).astype(np.float64)
    c.y_lmt = rng.integers(-5, 6, size=c.mpp).astype(np.float64)
    c.lm = np.concatenate([Ai @ c.x_lm.astype(np.int64), c.x_lm.astype(np.int64)[fidx]]).astype(np.float64)
    lmt = Ai.T @ c.y_lmt[:mA].astype(np.int64)
    lmt[fidx] += c.y_lmt[mA:].astype(np.int64)
    c.lmt = lmt.astype(np.float64)
    bits = [np.abs(Ai) @ np.abs(c.x_lm), np.abs(Ai).T @ np.abs(c.y_lmt[:mA]) + 5.0]
    if c.form == 1:
        Af = Ai * free[None, :]
        t = Af @ ri
        yn, sc = _exact_solve(c.tri, c.D, t)
        vn = sc * (ri * free) - Af.T @ yn
        vn[fix] = 0
        L = c.factor()
        absA = np.abs(Af).astype(np.float64)
        bits += [absA @ np.abs(ri * free), absA @ absA.T, np.abs(L) @ np.abs(L).T]            # A r, M, every Cholesky intermediate
    else:
        t = np.concatenate([Ai @ ri, ri[fidx]])
        yn, sc = _exact_solve(c.tri, c.D, t)
        sub = Ai.T @ yn[:mA]
        sub[fidx] += yn[mA:]
        vn = sc * ri - sub
        L = c.factor()
        bits += [np.abs(Ai).astype(np.float64) @ np.abs(ri)]
    c.y = _to_float(yn, sc)
    c.v = _to_float(vn, sc)
    c.granularity = granularity(c.v) if np.any(c.v) else granularity(c.y)      # v == 0 (square A_free): the multipliers' instead
    # the substitutions: u = L^-1 t (forward), y (backward); every partial sum of t_i - sum_j L_ij u_j is bounded by |t| + |L||u|
    sq = np.sqrt(c.D.astype(np.float64))
    u = _to_float(c.tri.inv_scaled(t), int(c.tri.a.max())) / sq
    absL = np.abs(L)
    gu, gy = granularity(u), granularity(c.y)
    bits += [(np.abs(t) + absL @ np.abs(u)) / gu, (np.abs(u) + absL.T @ np.abs(c.y)) / min(gu, gy)]
    if c.form == 1:
        bits += [(np.abs(ri) + np.abs(Af).T.astype(np.float64) @ np.abs(c.y)) / gy]
        if mA <= 64:
            W = exact_linv(c)
            gw = granularity(W)
            bits += [np.abs(W) @ np.abs(t) / gw, np.abs(W).T @ np.abs(u) / (gw * gu)]
    else:
        bits += [(np.abs(ri) + np.abs(Ai).T.astype(np.float64) @ np.abs(c.y[:mA]) + np.abs(np.concatenate([c.y[mA:], [0.0]])).max()) / gy]
    c.sum_bits = max(float(np.log2(max(np.max(b, initial=1.0), 1.0))) for b in bits)
    return c


def exact_linv(c):
    """sqrt(D)^-1 T^-1, dense (order <= 64 in practice): dyadic."""
    m = c.order
    amax = int(c.tri.a.max())
    W = np.stack([c.tri.inv_scaled(e) for e in np.eye(m, dtype=np.int64)], axis=1).astype(np.float64) / amax
    return W / np.sqrt(c.D.astype(np.float64))[:, None]


def reduced_case(name, mA, n, nfix, seed, gram=(1,), identity=False, rows=None, fix=None, dead_row=None):
    """dead_row: that row of Q is zero on the free columns (its entries sit on fixed columns only): D = 0 there — the rank-deficient
    instance, without expected outputs."""
    rng = np.random.default_rng(seed)
    if fix is None:
        fix = np.zeros(n, dtype=bool)
        if nfix:
            fix[rng.choice(n - 1, nfix, replace=False)] = True                 # the last column stays free: the j1 < n tails carry data
    nf = n - int(fix.sum())
    assert mA <= nf
    if rows is None:
        rows = np.concatenate([rng.choice(nf - 1, mA - 1, replace=False), [nf - 1]]).astype(np.int64)
        rows = rows[rng.permutation(mA)]
    Q, D = block_rows(nf, rows)
    tri = Eye(mA) if identity else make_tri(mA, rng)
    A = rng.integers(-3, 4, size=(mA, n)).astype(np.int64)
    if dead_row is not None:
        Q[dead_row] = 0
        D[dead_row] = 0
    A[:, ~fix] = tri.dense().astype(np.int64) @ Q
    r = rng.integers(-9, 10, size=n).astype(np.int64)
    r[fix] = rng.integers(100, 1000, size=int(fix.sum())) * np.where(rng.random(int(fix.sum())) < 0.5, -1, 1)
    c = ProjCase(name, 1, n, mA, A.astype(np.float64), fix, r.astype(np.float64), tri, D, gram=tuple(gram))
    return c if dead_row is not None else _finish(c, rng)


def augmented_case(name, mA, n, nfix, seed):
    rng = np.random.default_rng(seed)
    fix = np.zeros(n, dtype=bool)
    fix[rng.choice(n, nfix, replace=False)] = True
    mpp = mA + nfix
    tri = make_tri(mpp, rng)
    D = 4 ** rng.integers(0, 4, size=mpp).astype(np.int64)
    A = rng.integers(-3, 4, size=(mA, n)).astype(np.float64)
    r = rng.integers(-9, 10, size=n).astype(np.float64)
    r[fix] = rng.integers(-50, 51, size=nfix)
    return _finish(ProjCase(name, 0, n, mA, A, fix, r, tri, D), rng)


SMALL_MA = (1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64)
LARGE_MA = (65, 96, 97, 128, 129, 193, 257)
AUG_ORDERS = {3: (1, 17, 2), 64: (5, 131, 59), 65: (5, 131, 60), 128: (65, 203, 63), 129: (20, 203, 109),
              3264: (2, 3400, 3262), 3265: (2, 3400, 3263)}          # mpp -> (mA, n, nfix)
AUG_ORACLE_MAX = 600

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def reduced_cases():
    def make():
        out = []
        for mA in SMALL_MA:
            n = 131 if mA <= 33 else 203
            out.append(reduced_case("red-mA%d-n%d" % (mA, n), mA, n, n // 3, 2000 + mA, gram=(0, 2)))
        for mA in LARGE_MA:
            out.append(reduced_case("red-mA%d-n523" % mA, mA, 523, 200, 2000 + mA, gram=(0, 1, 2)))
        for mA in (17, 65):                                                      # fixrank == nullptr
            out.append(reduced_case("red-nofix-mA%d-n131" % mA, mA, 131, 0, 3000 + mA, gram=(0, 2)))
        for mA in (16, 64):                                                      # mA + nfix == n: one whole Hadamard block
            n = 131 if mA == 16 else 203
            out.append(reduced_case("red-full-mA%d-n%d" % (mA, n), mA, n, n - mA, 4000 + mA, gram=(0, 2), rows=np.arange(mA)))
        out.append(reduced_case("red-mA3-n4112", 3, 4112, 4112 // 3, 5001, gram=(0, 2)))      # second 8 x 256-chunk batch of left_mul_row
        out.append(reduced_case("red-mA1-n16", 1, 16, 5, 5002, gram=(0, 2)))                  # one chunk row: the clamped loads hit one chunk
        # 264 chunks: thread 8 of left_mul_row meets c0 + 256 == nch, and the last chunk holds the (free) column n - 1
        out.append(reduced_case("red-mA3-n527", 3, 527, 175, 5003, gram=(0, 2)))
        return out
    return _cached("reduced", make)


def identity_case():
    """M = diag(4^k): T = I, mA = 64 — what the device's reciprocal square root makes of exact powers of four."""
    return _cached("identity", lambda: reduced_case("red-identity-mA64-n203", 64, 203, 67, 6001, identity=True))


def rank_deficient_case():
    """mA = 40; row 32 of Q is supported on fixed columns only: the pivot of column 33 is an exact zero."""
    return _cached("rankdef", lambda: reduced_case("red-rankdef-mA40-n203", 40, 203, 67, 6002, dead_row=32))


def sequence_cases(n=203, mA=20, seed=7001):
    """One A, the fixed sets F1, F2 (F1 a subset of F2), F1 again.  Under F1 the rows of Q come from the two 64-blocks, ten from each
    with distinct indices inside the 16-block (H_64 = H_4 (x) H_16); F2 fixes three of the four 16-column segments of either block
    as well, so every row of Q keeps +- one row of H_16 and its free squared norm goes 64 -> 16.  A stale factor, or a stale explicit
    inverse, gives the other set's answer."""
    def make():
        rng = np.random.default_rng(seed)
        fix1 = np.zeros(n, dtype=bool)
        fix1[rng.choice(n - 1, 67, replace=False)] = True
        nf = n - 67
        assert nf >= 128
        rows = []
        for b in range(2):
            i16 = rng.choice(16, 10, replace=False)
            rows += [64 * b + 16 * int(rng.integers(0, 4)) + int(k) for k in i16]
        rows = np.array(rows)[rng.permutation(mA)]
        c1 = reduced_case("seq-F1-mA%d-n%d" % (mA, n), mA, n, 67, seed, fix=fix1, rows=rows)
        fidx = np.flatnonzero(~fix1)
        fix2 = fix1.copy()
        for b, keep in ((0, 2), (1, 0)):
            for seg in range(4):
                if seg != keep:
                    fix2[fidx[64 * b + 16 * seg:64 * b + 16 * seg + 16]] = True
        c2 = ProjCase("seq-F2-mA%d-n%d" % (mA, n), 1, n, mA, c1.A, fix2, c1.r.copy(), c1.tri, np.full(mA, 16, dtype=np.int64))
        c2.r[fix2 & ~fix1] = 777.0
        c1b = ProjCase(c1.name + "-again", 1, n, mA, c1.A, fix1, c1.r, c1.tri, c1.D)
        return [c1, _finish(c2, rng), _finish(c1b, rng)]
    return _cached(("seq", n, mA, seed), make)


def augmented_cases(max_order=None):
    out = []
    for mpp, (mA, n, nfix) in AUG_ORDERS.items():
        if max_order is None or mpp <= max_order:
            out.append(_cached(("aug", mpp), lambda: augmented_case("aug-mpp%d-mA%d-n%d" % (mpp, mA, n), mA, n, nfix, 8000 + mpp)))
    return out


CG_MA = (1, 16, 17, 33, 64, 65)
CG_N = (203, 208)
CG_C = 16.0


def cg_case(mA, n):
    """Reduced-form case whose r serves as the gradient g of the exact CG iteration."""
    return _cached(("cg", mA, n), lambda: reduced_case("cg-mA%d-n%d" % (mA, n), mA, n, n // 3, 9000 + 10 * mA + n))


def cg_jacobian(n):
    """J with J'J = 16 I: a block-diagonal stack of H_16, 2 H_4 and 4 H_1 blocks."""
    J = np.zeros((n, n))
    o = 0
    for s, f in ((16, 1.0), (4, 2.0), (1, 4.0)):
        while o + s <= n:
            J[o:o + s, o:o + s] = f * _H[s]
            o += s
    assert o == n
    return J


# ------------------------------------------------------------------------------------------------------------------ restatements
def zero_sub_diagonal(L):
    """A copy of L with one non-zero sub-diagonal entry of every 64 x 64 diagonal block set to zero (the first one of the block's last
    row that has one); None if there is no such entry at all."""
    L = L.copy()
    hit = False
    for k0 in range(0, L.shape[0], 64):
        nb = min(64, L.shape[0] - k0)
        for i in range(k0 + nb - 1, k0, -1):
            nz = np.flatnonzero(L[i, k0:i])
            if nz.size:
                L[i, k0 + nz[0]] = 0.0
                hit = True
                break
    return L if hit else None


def chol_blocked(M, pert=None):
    """Right-looking Cholesky in the kernels' order: per 64-column panel potrf (rank-one updates, the column scaled by the reciprocal
    square root of its pivot: chol_small_body), trsm (one row at a time, columns in order, times the reciprocal diagonal:
    chol_trsm_kernel), syrk (chol_syrk_kernel).  pert[j] multiplies the reciprocal of column j.  Returns (L, dinv)."""
    m = M.shape[0]
    L = np.tril(M).astype(np.float64)
    dinv = np.zeros(m)
    for k0 in range(0, m, 64):
        nb = min(64, m - k0)
        B = L[k0:k0 + nb, k0:k0 + nb]
        for j in range(nb):
            piv = B[j, j]
            rinv = (1.0 / math.sqrt(piv)) * (1.0 if pert is None else pert[k0 + j])
            dinv[k0 + j] = rinv
            B[j + 1:, j] *= rinv
            B[j, j] = piv * rinv
            col = B[j + 1:, j]
            B[j + 1:, j + 1:] -= np.tril(np.outer(col, col))
        rem = m - k0 - nb
        if rem > 0:
            X = L[k0 + nb:, k0:k0 + nb]
            for j in range(nb):
                X[:, j] = (X[:, j] - X[:, :j] @ B[j, :j]) * dinv[k0 + j]
            L[k0 + nb:, k0 + nb:] -= np.tril(X @ X.T)
    return L, dinv


def trsv_small(L, dinv, t):
    """trsv_small_body: column substitutions with the reciprocal diagonal."""
    x = t.astype(np.float64).copy()
    m = x.shape[0]
    for j in range(m):
        x[j] *= dinv[j]
        x[j + 1:] -= L[j + 1:, j] * x[j]
    for j in range(m - 1, -1, -1):
        x[j] *= dinv[j]
        x[:j] -= L[j, :j] * x[j]
    return x


def trsv_pair(L, t, split, drop=None):
    """trsv_pair_kernel: 64-wide blocked substitution, 1.0 / diagonal inside a block, forward trailing update in `split` slices,
    backward update by whole columns.  drop = (block, slice): that slice of that block's trailing update loses its last column."""
    m = t.shape[0]
    x = t.astype(np.float64).copy()
    nblk = (m + 63) // 64
    for b in range(nblk):
        j0 = 64 * b
        nb = min(64, m - j0)
        for jj in range(nb):
            j = j0 + jj
            x[j] *= 1.0 / L[j, j]
            x[j + 1:j0 + nb] -= L[j + 1:j0 + nb, j] * x[j]
        i0 = j0 + nb
        if i0 < m:
            per = (nb + 3) >> 2 if split == 4 else nb
            parts = []
            for q in range(split):
                jlo, jhi = q * per, min(nb, q * per + per)
                if drop == (b, q):
                    jhi -= 1
                parts.append(L[i0:, j0 + jlo:j0 + jhi] @ x[j0 + jlo:j0 + jhi])
            x[i0:] -= ((parts[0] + parts[1]) + (parts[2] + parts[3])) if split == 4 else parts[0]
    for b in range(nblk - 1, -1, -1):
        j0 = 64 * b
        nb = min(64, m - j0)
        for jj in range(nb - 1, -1, -1):
            j = j0 + jj
            x[j] *= 1.0 / L[j, j]
            x[j0:j] -= L[j, j0:j] * x[j]
        if b > 0:
            x[j0 - 64:j0] -= L[j0:, j0 - 64:j0].T @ x[j0:]
    return x


def tri_inv(L, dinv):
    """Linv by column substitution with the reciprocal diagonal (tri_inv_small_kernel forms the same entries by block recursion)."""
    m = L.shape[0]
    W = np.zeros((m, m))
    for i in range(m):
        acc = np.eye(m)[i] - L[i, :i] @ W[:i]
        W[i] = acc * dinv[i]
    return W


def restate_reduced(c, pert=None, linv=False, unmask=None, swap_r=None, zero_sub=False, drop=None, fix=None):
    """bh_project in the reduced form, in float64: masked Gram matrix, blocked Cholesky, substitutions (trsv_small up to 64 rows,
    trsv_pair above; linv = True: y = Linv'(Linv t), with `drop` = q losing the last column of the q-th 16-column quarter of Linv t),
    v = r_free - A_free'y.  The keyword arguments are the structural changes the CPU test applies."""
    fix = (c.fix if fix is None else fix).copy()
    if unmask is not None:
        fix[unmask] = False
    r = c.r.copy()
    if swap_r is not None:
        r[list(swap_r)] = r[list(swap_r)[::-1]]
    Af = c.A * (~fix)[None, :]
    M = Af @ Af.T
    L, dinv = chol_blocked(M, pert)
    if zero_sub:
        L = zero_sub_diagonal(L)
    t = Af @ r
    m = c.mA
    if linv:
        W = tri_inv(L, dinv)
        if drop is None:
            u = W @ t
        else:
            keep = np.ones(m, dtype=bool)
            keep[min(16 * drop + 15, m - 1)] = False
            u = W[:, keep] @ t[keep]
        y = W.T @ u
    elif m <= 64:
        y = trsv_small(L, dinv, t)
    else:
        y = trsv_pair(L, t, trsv_split_for(m), drop)
    v = np.where(fix, 0.0, r - Af.T @ y)
    return v


def restate_augmented(c, split=None, zero_sub=False, drop=None, swap_r=None):
    r = c.r.copy()
    if swap_r is not None:
        r[list(swap_r)] = r[list(swap_r)[::-1]]
    L = c.factor()
    if zero_sub:
        L = zero_sub_diagonal(L)
    fidx = np.flatnonzero(c.fix)
    t = np.concatenate([c.A @ r, r[fidx]])
    y = trsv_pair(L, t, trsv_split_for(c.mpp) if split is None else split, drop)
    sub = c.A.T @ y[:c.mA]
    sub[fidx] += y[c.mA:]
    return r - sub


def perturbation_tol(c, runs=32):
    """64 x the largest infinity-norm deviation from the exact projection over `runs` restatements whose reciprocal diagonals carry a
    random factor 1 +- 2^-52 (the factor 64 stands for the orders and fused operations that the restatement does not model)."""
    rng = np.random.default_rng(sum(map(ord, c.name)))
    worst = 0.0
    for k in range(runs):
        pert = 1.0 + np.where(rng.random(c.mA) < 0.5, -1.0, 1.0) * 2.0 ** -52
        worst = max(worst, float(np.max(np.abs(restate_reduced(c, pert, linv=(c.mA <= 64 and k % 2 == 1)) - c.v))))
    return 64.0 * worst
