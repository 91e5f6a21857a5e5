"""The sorted form of the box-constrained Cauchy search on a Gram-form handle (bh_hess_set_cauchy_search, bh_cauchy_info form 5;
csrc/bh_cauchysort.hip.h) restated in float64 NumPy, in the kernels' summation orders, with the edge placements of the kernels' own
geometry.  Helper of tests/test_cauchy_sorted_gpu.py, proved on the CPU by tests/test_sorted_cases_cpu.py.  Not a test.

    cauchy_sort_rank_kernel   thread (x, tid) of workgroup (x, y) owns index 256 x + tid and counts the keys of tile y (512 keys)
    cauchy_sort_rows_kernel   row group = the rows of 4 consecutive variables; a row is summed per panel of 4096 columns: the per-lane chain over the
                              chunks tid + 512 c (x before y), the wave butterfly (a balanced tree over the 64 lanes), the 8 waves in
                              ascending order; kernel 3 adds the panels in ascending order
    cauchy_sort_scan_kernel   thread t owns the segments t E .. t E + E - 1, E = ceil((n + 1) / 1024); the orders are stated there

What the restatement does not model is the fusion of a product and a sum into one rounding in the row sums (fma): on the exact
instances both forms give the same bits (every partial sum is exact, test_sorted_cases_cpu.py), elsewhere they differ by roundings.
The geometry constants are parsed out of the kernel header."""
import math
import os
import re
from collections import namedtuple
from fractions import Fraction

import numpy as np

import gram_cases as gc
import refresh_cases as rc

_HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "benlsip.jl_amd", "csrc", "bh_cauchysort.hip.h")


def _const(name):
    return int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, open(_HDR).read()).group(1))


RANK_T, RANK_TILE = _const("CS_RANK_T"), _const("CS_RANK_TILE")
ROW_T, ROW_CPT, ROW_R = _const("CS_ROW_T"), _const("CS_ROW_CPT"), _const("CS_ROW_R")
SCAN_T, MAX_PANELS = _const("CS_SCAN_T"), _const("CS_MAX_PANELS")
PANEL = 2 * ROW_T * ROW_CPT                                          # columns of a panel
FAULTS = ("tie_order", "own_term_in_U", "prefix_for_suffix", "b_from_the_wrong_side")
INF = math.inf


def decide(phi_p, phi_pp, th, ind, nfix, nmm):
    """cauchy_decide of csrc/bh_cauchy.hip.h (:615-636): (done, min_found, err, advance, step, delta_t)."""
    delta_t = (-phi_p / phi_pp) if phi_pp > 0.0 else 0.0
    if not (nfix < nmm):
        return 1, 0, 0, 0, 0.0, delta_t
    if phi_p >= 0.0:
        return 1, 1, 0, 0, 0.0, delta_t
    if phi_p < 0.0 and phi_pp > 0.0 and delta_t < th:
        return 1, 1, 0, 0, delta_t, delta_t
    if ind < 0:
        return 1, 0, 1, 0, 0.0, delta_t
    return 0, 0, 0, 1, th, delta_t


def keys_and_ranks(g, d_l, d_u, fix, fault=None):
    """Kernel 1: T_i, b_i (0 unless T_i is finite), rank_i (-1: fixed at the start), the inverse permutation, the hand-back flag."""
    n = g.shape[0]
    free = ~fix
    d = -g
    flip = fault == "b_from_the_wrong_side"
    lo, up = (d_u, d_l) if flip else (d_l, d_u)
    T = np.full(n, np.nan)
    with np.errstate(all="ignore"):
        T[free] = np.where(d[free] < 0, (lo[free] - 0.0) / d[free], np.where(d[free] > 0, (up[free] - 0.0) / d[free], INF))
    bad = bool(np.any(free & (~np.isfinite(g) | np.isnan(d_l) | np.isnan(d_u) | np.isnan(np.where(free, T, 0.0)) | (T == -INF))))
    b = np.where(free & np.isfinite(T), np.where(d < 0, lo, up), 0.0)
    idx = np.flatnonzero(free)
    # rank_i = #{free j: T_j < T_i or (T_j == T_i and j < i)}: the position in the order by (T, index)
    order = idx[np.lexsort((-idx if fault == "tie_order" else idx, T[idx]))]
    rank = np.full(n, -1, dtype=np.int64)
    rank[order] = np.arange(order.size)
    return T, b, rank, order, bad


def _tree64(v):
    """wave_reduce of csrc/bh_reduce.hip.h with OpSum over the last axis (64 lanes): lane ^ 1, ^ 2, the mirrors inside 8 and 16, the
    row swaps — a balanced tree over the lanes in natural order (a + b == b + a)."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def row_sums(G, d, b, rank, order, fault=None, rows_per_step=128):
    """Kernel 2: U_r, L_r (by rank) from the rows G[i, :] of the free variables, as [npanels][nfree] parts in the kernel's order."""
    n = d.shape[0]
    nfree = order.size
    ld = -(-n // 16) * 16
    npanels = -(-(ld // 2) // (ROW_T * ROW_CPT))
    cols = npanels * PANEL
    dp, bp = np.zeros(cols), np.zeros(cols)
    dp[:n], bp[:n] = d, b
    rp = np.full(cols, -1, dtype=np.int64)
    rp[:n] = rank
    Up, Lp = np.zeros((npanels, nfree)), np.zeros((npanels, nfree))
    for r0 in range(0, nfree, rows_per_step):
        rr = np.arange(r0, min(r0 + rows_per_step, nfree))
        Gb = np.zeros((rr.size, cols))
        Gb[:, :n] = G[order[rr], :]
        above = (rp[None, :] >= rr[:, None]) if fault == "own_term_in_U" else (rp[None, :] > rr[:, None])
        for sel, out in ((np.where(above, dp[None, :], 0.0), Up), (np.where(rp[None, :] < rr[:, None], bp[None, :], 0.0), Lp)):
            prod = (Gb * sel).reshape(rr.size, npanels, ROW_CPT, ROW_T, 2)       # column = 4096 p + 2 (tid + 512 c) + xy
            lane = np.zeros((rr.size, npanels, ROW_T))
            for c in range(ROW_CPT):
                lane = lane + prod[:, :, c, :, 0]
                lane = lane + prod[:, :, c, :, 1]
            waves = _tree64(lane.reshape(rr.size, npanels, ROW_T // 64, 64))
            tot = np.zeros((rr.size, npanels))
            for w in range(ROW_T // 64):
                tot = tot + waves[:, :, w]
            out[:, rr] = tot.T
    return Up, Lp


def _fold(parts):
    out = parts[0].copy()
    for p in range(1, parts.shape[0]):
        out = out + parts[p]
    return out


def block_offsets(tot, ascending=False):
    """cauchy_carry_behind / cauchy_carry_before on the SCAN_T block totals of the scan kernel: descending, the totals behind lane l
    from lane 63 downwards and the wave totals behind wave w from the last wave downwards, A + B; ascending, those before lane l
    from lane 0 upwards and before wave w from wave 0 upwards, B + A."""
    NW = SCAN_T // 64
    t = tot.reshape(NW, 64)
    a = np.zeros((NW, 64))
    acc = np.zeros(NW)
    for u in (range(64) if ascending else range(63, -1, -1)):
        a[:, u] = acc
        acc = (acc + t[:, u]) if ascending else (t[:, u] + acc)
    bw = np.zeros(NW)
    accw = 0.0
    for v in (range(NW) if ascending else range(NW - 1, -1, -1)):
        bw[v] = accw
        accw = (accw + acc[v]) if ascending else (acc[v] + accw)
    return ((bw[:, None] + a) if ascending else (a + bw[:, None])).reshape(SCAN_T)


def stop_and_finish(g, b, order, To, fix0, bad, gsum, cross, phi_pp):
    """What both sorted forms do behind the scanned sums (cauchy_sort_stop, cauchy_sort_finish): theta and phi' of every segment
    from sum_{r >= k} g d, the cross term (sum_{r < k} c, or X_k) and phi''_k; the first segment at which the search ends; the
    hand-back (`bad`: the keys' flag), or s and the active set.  Returns the result tuple without its `terms`, and the segment
    arrays that go into them."""
    n, nfree, pad = g.shape[0], order.size, phi_pp.shape[0]
    nfix0, nmm = int(fix0.sum()), n
    with np.errstate(all="ignore"):
        tprev = np.zeros(pad)
        tprev[1:nfree + 1] = To
        tk = np.full(pad, INF)
        tk[:nfree] = To
        theta = np.where(np.isfinite(tk), tk - tprev, INF)
        phi_p = (gsum + cross) + tprev * phi_pp
    kstar, q, seg_bad = None, None, False
    for k in range(nfree + 1):
        ind = int(order[k]) if k < nfree and math.isfinite(tk[k]) else -1
        q = decide(float(phi_p[k]), float(phi_pp[k]), float(theta[k]), ind, nfix0 + k, nmm)
        seg_bad = not (math.isfinite(phi_p[k]) and math.isfinite(phi_pp[k]))
        if q[0] or seg_bad:
            kstar = k
            break
    seg = dict(phi_p=phi_p[:nfree + 1], phi_pp=phi_pp[:nfree + 1], theta=theta[:nfree + 1])
    if bad or seg_bad:
        return (None, None, None, None, True, kstar, None, None), seg
    done, min_found, err, advance, step, delta_t = q
    s = np.zeros(n)
    fix = fix0.copy()
    fixed_now = order[:kstar]
    s[fixed_now] = b[fixed_now]
    fix[fixed_now] = True
    rest = order[kstar:]
    with np.errstate(all="ignore"):
        s[rest] = (0.0 + tprev[kstar] * (-g[rest])) + step * (-g[rest])
    return (s, fix, kstar + 1, err, False, kstar, float(phi_p[kstar]), float(phi_pp[kstar])), seg


SortedResult = namedtuple("SortedResult", "s fix n_hmul err handback kstar phi_p phi_pp terms")


def sorted_search(inst, G=None, fault=None):
    """cauchy_step (src/basic_tralcnlss.jl:574-639) as the three kernels of the sorted form compute it.  inst = (J, C, mu, A, x, g, xlow,
    xupp, delta) with no rows in A; G: J'J + mu C'C when the caller has it.  `fault`: one of FAULTS, a wrong kernel."""
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    assert A is None or A.shape[0] == 0
    n = J.shape[1]
    if G is None:
        Jt = np.vstack([J, C]) if C is not None and C.shape[0] else J
        wts = np.ones(Jt.shape[0])
        wts[J.shape[0]:] = mu
        G = Jt.T @ (wts[:, None] * Jt)
    with np.errstate(invalid="ignore"):
        fix0 = ((x - xlow) <= gc.SQRT_EPS) | ((xupp - x) <= gc.SQRT_EPS)  # active_bounds! (poly:211)
        d_u, d_l = np.minimum(xupp - x, delta), np.maximum(xlow - x, -delta)
    T, b, rank, order, bad = keys_and_ranks(g, d_l, d_u, fix0, fault)
    nfree = order.size
    d = np.where(fix0, 0.0, -g)
    with np.errstate(all="ignore"):
        Up, Lp = row_sums(G, d, b, rank, order, fault)
        U, L = (_fold(Up), _fold(Lp)) if nfree else (np.zeros(0), np.zeros(0))
        # ---- kernel 3: the terms by rank -----------------------------------------------------------------------------------------
        go, do, bo, To = g[order], -g[order], b[order], T[order]
        shell = do * (G[order, order] * do + 2.0 * U)
        c = np.where(np.isfinite(To), bo * U - do * L, 0.0)
        gd = go * do
        E = -(-(n + 1) // SCAN_T)
        pad = SCAN_T * E

        def blocks(v):
            out = np.zeros(pad)
            out[:nfree] = v
            return out.reshape(SCAN_T, E)
        cb, sb, gb = blocks(c), blocks(shell), blocks(gd)
        P, W, Wg = np.zeros((SCAN_T, E)), np.zeros((SCAN_T, E)), np.zeros((SCAN_T, E))
        p = np.zeros(SCAN_T)
        for e in range(E):                                           # prefix of c ascending from +0
            P[:, e] = p
            p = p + cb[:, e]
        ws, wg = np.zeros(SCAN_T), np.zeros(SCAN_T)
        for e in range(E - 1, -1, -1):                               # suffixes of shell and g d descending from +0
            ws = sb[:, e] + ws
            wg = gb[:, e] + wg
            W[:, e], Wg[:, e] = ws, wg
        if fault == "prefix_for_suffix":                             # phi'' from the ranks below k instead of the ranks from k on
            ws2 = np.zeros(SCAN_T)
            for e in range(E):
                W[:, e] = ws2
                ws2 = ws2 + sb[:, e]
        offC = block_offsets(p, True)
        offS = block_offsets(ws if fault != "prefix_for_suffix" else ws2, fault == "prefix_for_suffix")
        offG = block_offsets(wg)
        phi_pp = (W + offS[:, None]).reshape(pad)
        gsum = (Wg + offG[:, None]).reshape(pad)
        csum = (offC[:, None] + P).reshape(pad)
    head, seg = stop_and_finish(g, b, order, To, fix0, bad, gsum, csum, phi_pp)
    return SortedResult(*head, dict(T=T, b=b, rank=rank, order=order, U=U, L=L, shell=shell, c=c, gd=gd, d=d, G=G, **seg))


# ------------------------------------------------------------------------------------------------------------ exactness
def _units_sum(led, what, terms):
    """Every partial sum of `terms`, in any order, is exact: all are integer multiples of one power of two and the sum of their
    magnitudes stays below 2^53 of them."""
    terms = np.asarray(terms, dtype=np.float64)
    e = gc.dyadic_exp(terms)
    led.note(what, int(gc.units(terms, e).sum()))


def prove_exact(inst, res, led, M=None):
    """The proof obligations of a sorted search on an exact instance: G d and G b bounded row by row (any subset, any order), every
    term equal to its rational value, every sum of terms exact in any order, phi' and phi'' up to the stop equal to their rationals."""
    t = res.terms
    M = gc.gram_matrix(inst, led) if M is None else M
    fin = np.isfinite(t["T"])
    led.matvec(M, t["d"], "U = sum G d")
    led.matvec(M, np.where(fin, t["b"], 0.0), "L = sum G b")
    order = t["order"]
    F = Fraction
    G = t["G"]
    kstar = res.kstar
    shell_q, c_q, gd_q = [], [], []
    for r, i in enumerate(order):
        di, Ur, Lr = F(float(t["d"][i])), F(float(t["U"][r])), F(float(t["L"][r]))
        sq = di * (F(float(G[i, i])) * di + 2 * Ur)
        cq = (F(float(t["b"][i])) * Ur - di * Lr) if fin[i] else F(0)
        gq = -di * di
        assert F(float(t["shell"][r])) == sq and F(float(t["c"][r])) == cq and F(float(t["gd"][r])) == gq, r
        shell_q.append(sq); c_q.append(cq); gd_q.append(gq)
    _units_sum(led, "sum shell", t["shell"])
    _units_sum(led, "sum c", t["c"])
    _units_sum(led, "sum g d", t["gd"])
    _units_sum(led, "sum g d + sum c", np.concatenate([t["gd"], t["c"]]))
    suf_s, suf_g = sum(shell_q, F(0)), sum(gd_q, F(0))
    pre_c, tprev = F(0), F(0)
    for k in range(kstar + 1):
        ppq = suf_s
        pq = suf_g + pre_c + tprev * ppq
        assert F(float(t["phi_pp"][k])) == ppq and F(float(t["phi_p"][k])) == pq, k
        led.note("T phi''", abs((tprev * ppq).numerator) if tprev * ppq != 0 else 0)
        if k < len(order):
            suf_s -= shell_q[k]; suf_g -= gd_q[k]; pre_c += c_q[k]
            tprev = F(float(t["T"][order[k]])) if fin[order[k]] else F(0)
    return led


# ------------------------------------------------------------------------------------------------------------ edge placements
def owner_of_key(i):
    """(workgroup, thread) of cauchy_sort_rank_kernel that ranks index i, and (tile, slot) at which every workgroup meets its key."""
    return i // RANK_T, i % RANK_T, i // RANK_TILE, i % RANK_TILE


def _tie_across(n, edge, note):
    """An order-sensitive tie (gram_cases._tie) whose members lie on both sides of `edge`, as close to it as the instance allows."""
    for a in range(8):
        for b in range(8):
            try:
                inst = gc._tie(n, edge - 1 - a, edge + b)
            except AssertionError:
                continue
            return gc.KCase("tie_%d_%d" % (edge - 1 - a, edge + b), n, inst, note)
    raise AssertionError("no order-sensitive tie across %d at n = %d" % (edge, n))


def edge_cases(n):
    """New placements on the edges of the sorted form's geometry at width n (family K's instance: refresh_cases.exact_instance)."""
    K = gc.KCase
    last = n - 1
    t1 = RANK_TILE                                                   # the first key of tile 1
    out = []
    # rank 0 on the last index, then the last key of tile 0, the first key of tile 1, the last / first thread of a workgroup of kernel 1
    order = [last, t1 - 1, t1, RANK_T - 1, RANK_T, 0]
    out.append(K("rank0_on_the_last_index", n, gc._k_exact(n, order), "ranks 0..5 on indices %s: tile and workgroup edges of kernel 1" % order))
    # the rows kernel 2 reads first and last in a row group, in the first and in the last group, fixed in that order
    order = list(dict.fromkeys([ROW_R - 1, ROW_R, 2 * ROW_R - 1, last - last % ROW_R, last]))      # (a last group of one row: one index)
    out.append(K("row_group_edges", n, gc._k_exact(n, order), "ranks 0..4 on rows %s: last row of group 0, first and last row of group 1, first "
                 "and last row of the last group (%d row(s))" % (order, last % ROW_R + 1)))
    # search lengths around a multiple of the group size (the scan kernel's blocks are E segments long: E and E + 1 too)
    E = -(-(n + 1) // SCAN_T)
    for length in sorted({ROW_R - 1, ROW_R, ROW_R + 1, E, E + 1}):
        order = [(37 * k + 11) % n for k in range(length)]
        out.append(K("stop_after_rank_%d" % (length - 1), n, gc._k_exact(n, order), "%d breakpoints: the stop is segment %d of scan thread %d"
                     % (length, length % E, length // E)))
    # ties: in one tile, across the workgroups 0 | 1 of kernel 1, and across its tiles 0 | 1
    out.append(K("tie_5_9", n, gc._tie(n, 5, 9), "both keys in one tile, ranked by one workgroup"))
    out.append(_tie_across(n, RANK_T, "ranked by workgroups 0 | 1 of kernel 1"))
    out.append(_tie_across(n, RANK_TILE, "the keys sit in tiles 0 | 1 of kernel 1"))
    # a tail of T = Inf variables with d != 0, and the stop behind the last finite breakpoint: the hits of `ascending`, every other
    # bound and the radius infinite — the search passes every finite breakpoint and ends at the minimiser of the open segment
    hits = gc.k_hits(n)
    J, C, mu, A, x, g, xlow, xupp, delta = gc._k_exact(n, hits)
    xupp = np.where(xupp < 1024.0, xupp, np.inf)
    out.append(K("infinite_tail", n, (J, C, mu, A, x, g, xlow, xupp, np.inf), "%d finite breakpoints, %d variables with T = Inf and d != 0;"
                 " the stop lies behind the last finite breakpoint (rank %d, then theta = Inf)" % (len(hits), n - len(hits), len(hits) - 1)))
    # (rank nfree - 1 is reached by gram_cases.k_all_fixed: every variable ends fixed)
    return out


def nan_bound_past_the_first_trip(fixed):
    """n = 1030, 20 rows: a NaN upper bound on variable 1027, which the scan kernel's threads reach on their second trip over the
    indices (1027 >= CS_SCAN_T).  fixed: the variable sits on its lower bound, so the initial active_bounds! fixes it."""
    n = 1030
    rng = np.random.default_rng(3)
    J = rng.standard_normal((20, n)) / np.sqrt(20.0)
    g = rng.standard_normal(n)
    x, xlow, xupp = np.zeros(n), -np.ones(n), np.ones(n)
    xupp[1027] = np.nan
    if fixed:
        x[1027] = xlow[1027]
    return (J, None, 0.0, None, x, g, xlow, xupp, 10.0)


EDGE_SIZES = (1030, 4097)


def describe(n):
    ld = -(-n // 16) * 16
    npanels = -(-(ld // 2) // (ROW_T * ROW_CPT))
    return ("sorted n=%-5d ld %d: kernel 1 %d workgroups x %d keys, %d tile(s) of %d; kernel 2 %d panel(s) of %d columns, %d row groups of %d; "
            "kernel 3 %d segments per thread" % (n, ld, -(-ld // RANK_T), RANK_T, -(-n // RANK_TILE), RANK_TILE, npanels, PANEL, -(-n // ROW_R), ROW_R,
                                                 -(-(n + 1) // SCAN_T)))
