"""The sorted rows form of the box-constrained Cauchy search on an implicit handle (bh_hess_set_cauchy_rows, bh_cauchy_info form 6;
csrc/bh_cauchyrowsort.hip.h) restated in float64 NumPy, in the kernels' written-out summation orders, every operation a single
rounding.  Helper of tests/test_cauchy_rowsort_gpu.py, proved on the CPU by tests/test_rowsort_cases_cpu.py.  Not a test.

    cauchy_sort_rank_kernel        unchanged (tests/sorted_cases.py: keys_and_ranks)
    cauchy_rowsort_rows_kernel     thread t owns RS_EPT consecutive ranks of a row staged in rank order; suffix of a d descending and
                                   prefix of a b ascending inside the thread, Kogge-Stone over the 64 thread totals of a wave, the
                                   wave totals serially; w S^2 and w P S added per segment over the rows of a workgroup in ascending
                                   order (row group = RS_R rows, workgroup x takes the groups x, x + grid, ...)
    cauchy_rowsort_reduce_kernel   the slabs over the workgroups in ascending order from +0
    cauchy_rowsort_scan_kernel     the suffix sums of g d in the order of cauchy_sort_scan_kernel, then every decision

The bits depend on `grid` (which rows meet in which slab), as on the device; on the exact instances every partial sum is exact and
any grid gives the same bits.  The geometry constants are parsed out of the kernel header."""
import math
import os
import re
from collections import namedtuple
from fractions import Fraction

import numpy as np

import gram_cases as gc
import refresh_cases as rc
import sorted_cases as sc

_HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benlsip.jl_amd", "csrc", "bh_cauchyrowsort.hip.h")


def _const(name):
    return int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(_HDR).read()).group(1))


T, EPT, R, GRID_PER_CU = _const("RS_T"), _const("RS_EPT"), _const("RS_R"), _const("RS_GRID_PER_CU")
MAXN = T * EPT                                                       # RS_MAXN: the widest padded row served
NW = T // 64
SCAN_T = sc.SCAN_T
FAULTS = ("prefix_for_suffix", "tie_order", "missing_row_weight", "b_from_the_wrong_side", "row_group_dropped", "wave_prefix_dropped")
INF = math.inf


def ld_of(n):
    return -(-n // 16) * 16


def served(n):
    return n >= 1 and ld_of(n) <= MAXN


def grid_of(rows, n_cu=256):
    """Workgroups of the row scan (bh_api.hip: cauchy_rows_grid)."""
    return max(1, min(-(-rows // R), GRID_PER_CU * n_cu))


def _ks(v, suffix):
    """Kogge-Stone inclusive scan over the last axis (64 lanes): off = 1, 2, .., 32; suffix: v_l + v_{l + off}, prefix: v_{l - off} + v_l."""
    v = v.copy()
    off = 1
    while off < 64:
        o = v.copy()
        if suffix:
            v[..., :64 - off] = o[..., :64 - off] + o[..., off:]
        else:
            v[..., off:] = o[..., :64 - off] + o[..., off:]
        off <<= 1
    return v


def row_scan(Jt, w, dr, br, grid, fault=None, rows_per_step=256):
    """Kernel 2: the slabs [grid][2][MAXN].  Jt: the image rows with the free columns in RANK order, padded with zeros to MAXN
    columns by the caller's dr, br (length MAXN, zero behind nfree)."""
    rows, nfree = Jt.shape
    slabs = np.zeros((grid, 2, MAXN))
    for r0 in range(0, rows, rows_per_step):
        r1 = min(r0 + rows_per_step, rows)
        m = r1 - r0
        A = np.zeros((m, MAXN))
        A[:, :nfree] = Jt[r0:r1]
        x, y = (A * dr).reshape(m, T, EPT), (A * br).reshape(m, T, EPT)
        Ss, Pp = np.zeros((m, T, EPT)), np.zeros((m, T, EPT))
        ts, tp = np.zeros((m, T)), np.zeros((m, T))
        for e in range(EPT - 1, -1, -1):                             # suffix of a d descending from +0
            ts = x[:, :, e] + ts
            Ss[:, :, e] = ts
        for e in range(EPT):                                         # prefix of a b ascending from +0
            Pp[:, :, e] = tp
            tp = tp + y[:, :, e]
        if fault == "prefix_for_suffix":                             # J~ d over the ranks below k instead of the ranks from k on
            ts = np.zeros((m, T))
            for e in range(EPT):
                Ss[:, :, e] = ts
                ts = ts + x[:, :, e]
        suffix = fault != "prefix_for_suffix"
        iS, iP = _ks(ts.reshape(m, NW, 64), suffix), _ks(tp.reshape(m, NW, 64), False)
        exS, exP = np.zeros((m, NW, 64)), np.zeros((m, NW, 64))
        if suffix:
            exS[..., :63] = iS[..., 1:]
            wtS = iS[..., 0]
        else:
            exS[..., 1:] = iS[..., :63]
            wtS = iS[..., 63]
        exP[..., 1:] = iP[..., :63]
        wtP = iP[..., 63]
        bS, bP = np.zeros((m, NW)), np.zeros((m, NW))
        acc = np.zeros(m)
        for v in (range(NW - 1, -1, -1) if suffix else range(NW)):   # the wave totals behind wave w from the last wave downwards
            bS[:, v] = acc
            acc = wtS[:, v] + acc
        acc = np.zeros(m)
        for v in range(NW):                                          # before wave w from wave 0 upwards
            bP[:, v] = acc
            acc = acc + wtP[:, v]
        if fault == "wave_prefix_dropped":                           # the prefix of a wave starts from +0: the totals of the waves before it lost
            bP[:] = 0.0
        offS = (exS + bS[:, :, None]).reshape(m, T)
        offP = (bP[:, :, None] + exP).reshape(m, T)
        S = (Ss + offS[:, :, None]).reshape(m, MAXN)
        P = (offP[:, :, None] + Pp).reshape(m, MAXN)
        ww = w[r0:r1, None]
        tS, tX = (ww * S) * S, (ww * P) * S
        for i in range(r0, r1):                                      # per segment over the rows of a workgroup in ascending order
            grp = i // R
            if fault == "row_group_dropped" and grp == 1:
                continue
            slabs[grp % grid, 0] = slabs[grp % grid, 0] + tS[i - r0]
            slabs[grp % grid, 1] = slabs[grp % grid, 1] + tX[i - r0]
    return slabs


RowsResult = namedtuple("RowsResult", "s fix n_hmul err handback kstar phi_p phi_pp terms")


def rowsort_search(inst, grid=None, fault=None):
    """cauchy_step (src/basic_tralcnlss.jl:574-639) as the kernels of the sorted rows form compute it.  inst = (J, C, mu, A, x, g, xlow,
    xupp, delta) with no rows in A; grid: workgroups of the row scan (default: a device of 256 compute units)."""
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    assert A is None or A.shape[0] == 0
    n = J.shape[1]
    assert served(n), n
    Jt = np.vstack([J, C]) if C is not None and C.shape[0] else J
    w = np.ones(Jt.shape[0])
    w[J.shape[0]:] = mu
    if fault == "missing_row_weight":
        w[:] = 1.0
    grid = grid_of(Jt.shape[0]) if grid is None else grid
    with np.errstate(invalid="ignore"):
        fix0 = ((x - xlow) <= gc.SQRT_EPS) | ((xupp - x) <= gc.SQRT_EPS)  # active_bounds! (poly:211)
        d_u, d_l = np.minimum(xupp - x, delta), np.maximum(xlow - x, -delta)
    Tk, b, rank, order, bad = sc.keys_and_ranks(g, d_l, d_u, fix0, fault if fault in ("tie_order", "b_from_the_wrong_side") else None)
    nfree = order.size
    d = np.where(fix0, 0.0, -g)
    with np.errstate(all="ignore"):
        dr, br = np.zeros(MAXN), np.zeros(MAXN)
        dr[:nfree], br[:nfree] = d[order], b[order]
        slabs = row_scan(Jt[:, order], w, dr, br, grid, fault)
        red = np.zeros((2, MAXN))
        for gi in range(grid):                                       # kernel 3: ascending from +0
            red = red + slabs[gi]
        F, X = red[0].copy(), red[1].copy()
        F[nfree:], X[nfree:] = 0.0, 0.0
        # ---- kernel 4 ------------------------------------------------------------------------------------------------------------
        go, To = g[order], Tk[order]
        E = -(-(n + 1) // SCAN_T)
        pad = SCAN_T * E
        gb = np.zeros(pad)
        gb[:nfree] = go * (-go)
        gb = gb.reshape(SCAN_T, E)
        Wg = np.zeros((SCAN_T, E))
        wg = np.zeros(SCAN_T)
        for e in range(E - 1, -1, -1):
            wg = gb[:, e] + wg
            Wg[:, e] = wg
        gsum = (Wg + sc.block_offsets(wg)[:, None]).reshape(pad)
        phi_pp, Xk = np.zeros(pad), np.zeros(pad)
        m = min(pad, MAXN)
        phi_pp[:m], Xk[:m] = F[:m], X[:m]
    head, seg = sc.stop_and_finish(g, b, order, To, fix0, bad, gsum, Xk, phi_pp)
    return RowsResult(*head, dict(T=Tk, b=b, rank=rank, order=order, d=d, X=Xk[:nfree + 1], Jt=Jt, w=w, grid=grid, **seg))


# ------------------------------------------------------------------------------------------------------------ exactness
def prove_exact(res, led):
    """The proof obligations of a sorted rows search on an exact instance, for the segments up to the stop: every S_ik and P_ik is a
    sum of products whose magnitudes stay below 2^53 units in any order; so are phi''_k and X_k over the rows (and slabs, in any
    order: any grid gives the same bits); phi'_k and phi''_k equal their rational values."""
    t = res.terms
    Jt, w, order, kstar = t["Jt"], t["w"], t["order"], res.kstar
    nfree = order.size
    a = Jt[:, order]
    d, b = t["d"][order], np.where(np.isfinite(t["T"][order]), t["b"][order], 0.0)
    ea, ed, eb, ew = gc.dyadic_exp(a), gc.dyadic_exp(d), gc.dyadic_exp(b[:kstar]), gc.dyadic_exp(w)
    ai, di, bi, wi = gc.units(a, ea), gc.units(d, ed), gc.units(b[:kstar], eb), gc.units(w, ew)
    Smax = ai @ di                                                   # per row: the bound of every sub-sum of a d, in units 2^-(ea + ed)
    Pmax = ai[:, :kstar] @ bi if kstar else np.zeros(a.shape[0], dtype=np.int64)
    led.note("S", int(Smax.max(initial=0)))
    led.note("P", int(Pmax.max(initial=0)))
    led.note("w S", int((wi * Smax).max(initial=0)))
    led.note("w P", int((wi * Pmax).max(initial=0)))
    led.note("phi''", int(sum(int(x) * int(s) * int(s) for x, s in zip(wi, Smax))))
    led.note("X", int(sum(int(x) * int(p) * int(s) for x, p, s in zip(wi, Pmax, Smax))))
    F = Fraction
    gq = [-F(float(v)) * F(float(v)) for v in t["d"][order]]
    eg = gc.dyadic_exp(np.asarray([float(v) for v in gq]))
    led.note("sum g d", int(sum(abs(v) for v in gq) * 2 ** eg))
    for k in range(kstar + 1):
        Sk = a[:, k:] @ d[k:]                                        # (exact: bounded above)
        Pk = a[:, :k] @ b[:k] if k else np.zeros(a.shape[0])
        ppq = sum((F(float(wv)) * F(float(s)) ** 2 for wv, s in zip(w, Sk)), F(0))
        xq = sum((F(float(wv)) * F(float(p)) * F(float(s)) for wv, p, s in zip(w, Pk, Sk)), F(0))
        tprev = F(float(t["T"][order[k - 1]])) if k else F(0)
        pq = sum(gq[k:], F(0)) + xq + tprev * ppq
        assert F(float(t["phi_pp"][k])) == ppq and F(float(t["X"][k])) == xq and F(float(t["phi_p"][k])) == pq, k
        led.note("T phi''", abs((tprev * ppq).numerator))
    return led


# ------------------------------------------------------------------------------------------------------------ edge placements
def column_owner(j):
    """(thread, wave, chunk) of cauchy_rowsort_rows_kernel that loads column j and stages it at its rank."""
    ch = j // 2
    return ch % T, (ch % T) // 64, ch // T


def rank_owner(r):
    """(thread, wave, slot) that owns rank r of a staged row."""
    return r // EPT, (r // EPT) // 64, r % EPT


def edge_cases(n):
    """Placements on the ownership edges of the row scan at width n (family K's instance: refresh_cases.exact_instance).  Ties are
    placed by COLUMN across the staging edges (thread: columns 1 | 2, wave: 127 | 128, chunk: 2 T - 1 | 2 T); their ranks are 0 and
    1 — an order-sensitive tie ends the search between its members, so it cannot sit at a later rank edge.  The rank edge of a thread
    (EPT - 1 | EPT) and the stops around it are reached by search lengths; the rank edge of a wave (64 EPT - 1 | 64 EPT) lies beyond
    the 255 exactly representable breakpoints of the family: LONG_CASES cross it (and every later wave edge) on random data."""
    K = gc.KCase
    out = []
    for length in (EPT - 1, EPT, EPT + 1, 4 * EPT + 1):
        if length <= n:
            order = [(37 * k + 11) % n for k in range(length)]
            out.append(K("stop_after_rank_%d" % (length - 1), n, gc._k_exact(n, order), "%d breakpoints: the stop is slot %d of thread %d"
                         % (length, length % EPT, length // EPT)))
    for a, b, note in ((1, 2, "staged by threads 0 | 1"), (127, 128, "staged by waves 0 | 1"), (2 * T - 1, 2 * T, "chunks 0 | 1: the last thread | thread 0")):
        if b < n:
            out.append(sc._tie_across(n, b, note))
    if n > 9:
        out.append(K("tie_5_9", n, gc._tie(n, 5, 9), "both staged inside one wave"))
    hits = gc.k_hits(n)
    Jm, C, mu, A, x, g, xlow, xupp, delta = gc._k_exact(n, hits)
    xupp = np.where(xupp < 1024.0, xupp, np.inf)
    out.append(K("infinite_tail", n, (Jm, C, mu, A, x, g, xlow, xupp, np.inf), "%d finite breakpoints, then T = Inf with d != 0" % len(hits)))
    return out


# d, n, q, nact, delta / ||g||, seed (the generator of the oracle cases): searches whose stop lies beyond the first wave's ranks
# (64 EPT = 512), so that the cross-wave carries of both scans decide the result.  The first ends with every variable fixed
# (924 breakpoints: waves 0 and 1), the second passes 3 764 breakpoints (all eight waves) and ends at an interior minimiser.
LONG_CASES = [(3000, 1024, 0, 100, 1e-9, 13), (60, 4096, 1, 50, 0.001, 14)]


def fixed_at_the_start(c):
    """Family-K case `c` with every third variable that has no early breakpoint put on its lower bound: fixed by the initial
    active_bounds!, its column dropped from the staged rows (rank -1).  J, C, mu unchanged."""
    J, C, mu, A, x, g, xlow, xupp, delta = c.inst
    x = x.copy()
    sel = np.flatnonzero(xupp >= 1024.0)[1::3]
    x[sel] = xlow[sel]
    return gc.KCase(c.name + "_fixed_at_the_start", c.n, (J, C, mu, A, x, g, xlow, xupp, delta), "%d variables fixed at the start" % sel.size)


def row_count_cases(n_cu=256):
    """(rows, q) of the image at, one below and one above the row-group and the per-workgroup boundaries: a group is R rows, the grid
    holds GRID_PER_CU * n_cu groups before workgroup 0 takes a second one."""
    full = R * GRID_PER_CU * n_cu
    return [(1, 0), (R - 1 or 1, 0), (R, 0), (R + 1, 1), (full - 1, 0), (full, 3), (full + 1, 0), (2 * full + R + 1, 3)]


def describe(n, rows, n_cu=256):
    return ("rowsort n=%-5d ld %d: %d rows in %d groups of %d on %d workgroups; thread t owns ranks %d t .. %d t + %d; scan %d segments per thread"
            % (n, ld_of(n), rows, -(-rows // R), R, grid_of(rows, n_cu), EPT, EPT, EPT - 1, -(-(n + 1) // SCAN_T)))
