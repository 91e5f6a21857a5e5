// bh_cauchysort.hip.h — the box-constrained Cauchy search from ONE sorted sweep over G (bh_hess_set_cauchy_search, form 5)
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bh_reduce.hip.h"
#include "bh_cg.hip.h"
#include "bh_cauchy.hip.h"
#include "bh_cauchy_sort_layout.h"

namespace bh {

// ------------------------------------------------------------------------------------------
// cauchy_step (src/basic_tralcnlss.jl:574-639) on a Gram-form handle with box constraints, without the walk over the breakpoints.
// d_i = -g_i while variable i is free (:592, :632), so every breakpoint time T_i = b_i / d_i (b_i = d_l,i for d_i < 0, d_u,i for
// d_i > 0) is known before the first pass, and the order in which variables are fixed is the sort order of (T_i, i) (:555 is a
// strict <: the smaller index first among equal T).  Variables with T = Inf (d_i = 0, or an infinite bound) come last.  In RANKS
// (segment k has the ranks < k fixed; T^(0) = 0, T^(k) = T_{k-1}; theta_k = T_k - T^(k), or Inf when rank k has no finite T):
//     U_r = sum_{j > r} G_rj d_j                 L_r = sum_{j < r, T_j finite} G_rj b_j
//     shell_r = d_r (G_rr d_r + 2 U_r)           c_r = b_r U_r - d_r L_r        (0 for T_r = Inf)
//     phi''_k = sum_{r >= k} shell_r                                             (= d'Hd of segment k, :611 / :635)
//     phi'_k  = (sum_{r >= k} g_r d_r + sum_{r < k} c_r) + T^(k) phi''_k         (= g'd + s_c'Hd, :610 / :634)
// and the search stops at the first k at which cauchy_decide(phi'_k, phi''_k, theta_k, ind_k, nfix0 + k, nmm) is done (:615-636).
// phi''_k and sum g_r d_r are TRUE suffix sums — formed over the ranks >= k and nothing else, never "total minus prefix": the tail
// shrinks by orders of magnitude during a search.
//
// Three launches behind cauchy_init_kernel, whatever the number of breakpoints:
//   1. cauchy_sort_rank_kernel   T_i, b_i and rank_i = #{free j : (T_j, j) < (T_i, i)}, counted against LDS tiles of the keys
//   2. cauchy_sort_rows_kernel   U_r, L_r from the contiguous rows G[i, :] of the free variables (the only launch that reads G)
//   3. cauchy_sort_scan_kernel   one workgroup: the suffix / prefix sums, every decision, s_c, d, the active set, the loop state
// Fixed orders everywhere (stated at each kernel), no atomics on doubles (the counts of kernel 1 are integers: their sum does not
// depend on the order): the bits do not depend on the grid, and a repeated search is bit-identical.  A non-finite g, a NaN bound
// of a free variable or a non-finite phi', phi'' at the stop raises the hand-back code in the progress word: the host runs that
// call again on the stepwise path.  The sorted rows form (bh_cauchyrowsort.hip.h) calls kernel 1 and the tail of kernel 3.
// ------------------------------------------------------------------------------------------
constexpr int CS_RANK_T = 256;           // threads of cauchy_sort_rank_kernel: one key each
constexpr int CS_RANK_TILE = 512;        // keys per LDS tile: workgroup (x, y) counts the keys of tile y
constexpr int CS_ROW_T = 512;            // threads of cauchy_sort_rows_kernel
constexpr int CS_ROW_CPT = 4;            // 16-byte chunks of a row per thread: a panel is 2 * CS_ROW_T * CS_ROW_CPT = 4096 columns
constexpr int CS_ROW_R = 4;              // rows (consecutive variables) per group
constexpr int CS_MAX_PANELS = 4;         // n <= 16384
constexpr int CS_SCAN_T = 1024;          // threads of cauchy_sort_scan_kernel
constexpr int kCauchyHandBack = 8;       // error field of the progress word: run this call on the stepwise path

static_assert(CS_MAX_PANELS == kCauchySortMaxPanels, "bh_cauchy_sort_layout.h: kCauchySortMaxPanels");

// What the keys, the stop and the write-back need: shared with the sorted rows form (bh_cauchyrowsort.hip.h).
struct CauchySortCore {
    CauchyArgs c;                // st, g, d, s, dl, du, xlow, xupp, fixrank, n, nmm, mirror, tag (as left by cauchy_init_kernel)
    int64_t ld;                  // padded width
    double* T; double* b;        // by index (ld each): T_i (NaN: fixed at the start), b_i (0 unless T_i is finite)
    int* rank; int* inv;         // rank[i] (-1: fixed at the start or padding; zeroed before kernel 1), inv[rank] = i (the scan kernel)
    int* flag;                   // hand-back flag of kernel 1 (cleared again by the scan kernel)
};

struct CauchySortArgs : CauchySortCore {
    const double* G;             // ld x ld row-major, padding rows and columns zero
    double* UL;                  // [2][npanels][ld] by rank: the per-panel parts of U, then of L
    double* scan;                // [3][ld + 16] by rank: prefix of c, suffix of shell, suffix of g d inside a thread's block
    int npanels;
};

// Key of variable i (i < n): T_i with the arithmetic of cauchy_breakpoint_theta at s_c = 0, and b_i.  NaN marks "fixed at the start"
// (a NaN never compares below or equal to anything: such a key is counted by nobody).  bad: the hand-back conditions.
__device__ __forceinline__ double cauchy_sort_key(const CauchyArgs& a, int i, double* b_out, bool* bad) {
    const double NaN = __longlong_as_double(0x7ff8000000000000ll);
    *b_out = 0.0;
    if (a.fixrank[i] >= 0) return NaN;
    const double gi = a.g[i], li = a.dl[i], ui = a.du[i];
    const double di = -gi;                                            // d = projection(lincons, -g), box constraints (:592)
    const double t = cauchy_breakpoint_theta(di, 0.0, li, ui);
    if (!(fabs(gi) < __longlong_as_double(0x7ff0000000000000ll)) || li != li || ui != ui || !(t == t) ||
        t == -__longlong_as_double(0x7ff0000000000000ll)) {
        *bad = true;
        return __longlong_as_double(0x7ff0000000000000ll);
    }
    if (fabs(t) < __longlong_as_double(0x7ff0000000000000ll)) *b_out = di < 0.0 ? li : ui;
    return t;
}

// 1. Keys and ranks.  Workgroup (x, y): thread tid owns index i = 256 x + tid < ld and counts the keys of tile y (512 keys, formed by
// the workgroup, 2 per thread) that come before its own: broadcast LDS reads, integer counts added into rank[i] (zero before the
// launch) — deterministic, no sort network; 1 + (n - 1) / 512 tiles spread the n^2 comparisons over the chip.
__global__ __launch_bounds__(CS_RANK_T) void cauchy_sort_rank_kernel(CauchySortCore sa) {
    __shared__ __attribute__((aligned(16))) double tile[CS_RANK_TILE];
    const CauchyArgs& a = sa.c;
    const int n = a.n, tid = threadIdx.x;
    const int i = (int)blockIdx.x * CS_RANK_T + tid;
    const int t0 = (int)blockIdx.y * CS_RANK_TILE;
    const double NaN = __longlong_as_double(0x7ff8000000000000ll);
    double Ti = NaN, bi = 0.0;
    bool bad = false;
    if (i < n) Ti = cauchy_sort_key(a, i, &bi, &bad);
    const bool free_i = Ti == Ti;
#pragma unroll
    for (int k = 0; k < CS_RANK_TILE / CS_RANK_T; ++k) {
        const int j = t0 + tid + k * CS_RANK_T;
        double bj;
        bool badj = false;
        tile[tid + k * CS_RANK_T] = j < n ? cauchy_sort_key(a, j, &bj, &badj) : NaN;
    }
    __syncthreads();
    const int m = min(CS_RANK_TILE, n - t0);                          // (keys behind n are NaN: the tile may be read to an even end)
    int cnt = 0;
    if (free_i) {
        const double2* tile2 = reinterpret_cast<const double2*>(tile);
#pragma unroll 8
        for (int j = 0; j < (m + 1) >> 1; ++j) {
            const double2 tj = tile2[j];
            const int j0 = t0 + 2 * j;
            cnt += (tj.x < Ti || (tj.x == Ti && j0 < i)) ? 1 : 0;
            cnt += (tj.y < Ti || (tj.y == Ti && j0 + 1 < i)) ? 1 : 0;
        }
        if (cnt > 0) atomicAdd(sa.rank + i, cnt);
    }
    if (blockIdx.y == 0 && i < (int)sa.ld) {
        sa.T[i] = Ti; sa.b[i] = bi;
        if (!free_i) sa.rank[i] = -1;                                 // (no tile adds to the rank of a fixed variable)
    }
    if (bad) *sa.flag = 1;                                            // (every writer stores the same value)
}

// 2. Row sums.  Row group grp holds the rows of the variables 4 grp .. 4 grp + 3; workgroup (x, panel) takes the groups x, x + gridDim.x, ... and of
// each row the 4096 columns of its panel: thread tid owns the chunks tid + 512 c (c < 4) of the panel and keeps d_j, b_j, rank_j of
// their columns in registers for all its rows.  Per row and panel: the per-lane fma chain in chunk order (x before y), the wave
// butterfly, the waves in ascending order; the panels are summed in ascending order by kernel 3.  Nothing of this depends on the grid.
// The next group's 16-byte loads are issued before the current group's reduction.  Rows of variables fixed at the start are not read.
__global__ __launch_bounds__(CS_ROW_T) void cauchy_sort_rows_kernel(CauchySortArgs sa) {
    constexpr int T = CS_ROW_T, CPT = CS_ROW_CPT, R = CS_ROW_R, NW = T / 64;
    __shared__ double red[2][2][R][NW];
    const CauchyArgs& a = sa.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const int panel = (int)blockIdx.y;
    const int64_t ld2 = sa.ld >> 1;
    const int c0 = panel * T * CPT;
    const double2* __restrict__ G2 = reinterpret_cast<const double2*>(sa.G);
    const int ngroups = (n + R - 1) / R;
    const int NG = (int)gridDim.x;

    bool act[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) act[c] = (int64_t)(c0 + tid + c * T) < ld2;
    double2 A[R][CPT], B[R][CPT];
    auto load_group = [&](double2 (&dst)[R][CPT], int grp) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = grp * R + r;
            const bool rv = i < n && sa.rank[i] >= 0;                  // (a variable fixed at the start: no load)
            const double2* rp = G2 + (int64_t)(rv ? i : 0) * ld2 + c0;
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                dst[r][c] = make_double2(0.0, 0.0);
                if (rv && act[c]) {
                    const dvec2 t = __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(rp + tid + c * T));
                    dst[r][c] = make_double2(t.x, t.y);
                }
            }
        }
    };
    int g = (int)blockIdx.x;
    if (g < ngroups) load_group(A, g);                                 // the first row group does not wait for the column vectors
    double2 dc[CPT], bc[CPT];
    int2 rk[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        dc[c] = bc[c] = make_double2(0.0, 0.0);
        rk[c] = make_int2(-1, -1);
        if (act[c]) {
            const int ch = c0 + tid + c * T;
            dc[c] = reinterpret_cast<const double2*>(a.d)[ch];         // d_j: -g_j, 0 for a fixed variable and in the padding
            bc[c] = reinterpret_cast<const double2*>(sa.b)[ch];        // b_j: 0 unless T_j is finite
            rk[c] = reinterpret_cast<const int2*>(sa.rank)[ch];
        }
    }
    int buf = 0;
    auto process = [&](double2 (&X)[R][CPT], int grp) {
        double su[R], sl[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = grp * R + r;
            const int rr = i < n ? sa.rank[i] : -1;                    // the rank of this row's variable
            double au = 0.0, al = 0.0;
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                au = fma(X[r][c].x, rk[c].x > rr ? dc[c].x : 0.0, au);
                au = fma(X[r][c].y, rk[c].y > rr ? dc[c].y : 0.0, au);
                al = fma(X[r][c].x, rk[c].x < rr ? bc[c].x : 0.0, al);
                al = fma(X[r][c].y, rk[c].y < rr ? bc[c].y : 0.0, al);
            }
            su[r] = wave_sum(au);
            sl[r] = wave_sum(al);
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) { red[buf][0][r][wave] = su[r]; red[buf][1][r][wave] = sl[r]; }
        }
        __syncthreads();
        if (tid < R) {
            double t0 = 0.0, t1 = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) { t0 += red[buf][0][tid][w]; t1 += red[buf][1][tid][w]; }
            const int i = grp * R + tid;
            const int rr = i < n ? sa.rank[i] : -1;
            if (rr >= 0) {
                sa.UL[(int64_t)panel * sa.ld + rr] = t0;
                sa.UL[(int64_t)(sa.npanels + panel) * sa.ld + rr] = t1;
            }
        }
        buf ^= 1;                                                      // (one barrier per group: the slot written next is the other one)
    };
    if (g < ngroups) {
        while (true) {
            int gn = g + NG;
            if (gn < ngroups) load_group(B, gn);
            process(A, g);
            if (gn >= ngroups) break;
            g = gn;
            gn = g + NG;
            if (gn < ngroups) load_group(A, gn);
            process(B, g);
            if (gn >= ngroups) break;
            g = gn;
        }
    }
}

// What rank r adds to the three sums.  Every operation is a single rounding (no contraction): the CPU restatement
// (tests/sorted_cases.py) does the same.
struct CauchySortTerm { double shell, c, gd; };
__device__ __forceinline__ CauchySortTerm cauchy_sort_term(const CauchySortArgs& sa, int r) {
    const CauchyArgs& a = sa.c;
    const int i = sa.inv[r];
    const double gi = a.g[i], di = -gi, bi = sa.b[i], Ti = sa.T[i];
    double U = sa.UL[r], L = sa.UL[(int64_t)sa.npanels * sa.ld + r];
    for (int p = 1; p < sa.npanels; ++p) {                            // the panels in ascending order
        U = __dadd_rn(U, sa.UL[(int64_t)p * sa.ld + r]);
        L = __dadd_rn(L, sa.UL[(int64_t)(sa.npanels + p) * sa.ld + r]);
    }
    const double grr = sa.G[(int64_t)i * sa.ld + i];
    CauchySortTerm t;
    t.shell = __dmul_rn(di, __dadd_rn(__dmul_rn(grr, di), __dmul_rn(2.0, U)));
    const bool fin = fabs(Ti) < __longlong_as_double(0x7ff0000000000000ll);
    t.c = fin ? __dsub_rn(__dmul_rn(bi, U), __dmul_rn(di, L)) : 0.0;
    t.gd = __dmul_rn(gi, di);
    return t;
}

// ---- the tail both sorted forms share (one workgroup of CS_SCAN_T threads; the kernels own the barriers) -------------------------
// The inverse permutation, this thread's indices (read behind the caller's barrier).  True: a free variable of this thread has a
// NaN bound.  d_l, d_u hide it (fmax, fmin of cauchy_init_kernel drop a NaN operand), so the keys cannot see it: hand back.
__device__ __forceinline__ bool cauchy_sort_invert(const CauchySortCore& sa) {
    const CauchyArgs& a = sa.c;
    bool nan_bound = false;
    for (int i = threadIdx.x; i < a.n; i += CS_SCAN_T) {
        const int r = sa.rank[i];
        const double lo = a.xlow[i], up = a.xupp[i];                    // (beside the rank load, not behind it)
        if (r >= 0) {
            sa.inv[r] = i;
            nan_bound = nan_bound || lo != lo || up != up;
        }
    }
    return nan_bound;
}

// Carries of N arrays of totals (array j at tot + j * stride), each a chain of its own, from +0: the totals behind position pos
// from position `last` downwards (acc = tot + acc), and the totals before pos from position 0 upwards (acc = acc + tot).  The lanes
// of a wave carry the block totals (last = 63), the waves carry the wave totals (last = 15).
template <int N>
__device__ __forceinline__ void cauchy_carry_behind(const double* tot, int stride, int last, int pos, double (&acc)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    for (int u = last; u > pos; --u)
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = __dadd_rn(tot[j * stride + u], acc[j]);
}
__device__ __forceinline__ double cauchy_carry_before(const double* tot, int pos) {
    double acc = 0.0;
    for (int u = 0; u < pos; ++u) acc = __dadd_rn(acc, tot[u]);
    return acc;
}

// phi', theta and the decision of segment k from phi''_k, the cross term (sum_{r < k} c_r, or X_k) and sum_{r >= k} g_r d_r.
struct CauchySortSeg { double phi_p, phi_pp, theta, t_prev; int ind; bool bad; CauchyDecision q; };
__device__ __forceinline__ CauchySortSeg cauchy_sort_stop(const CauchySortCore& sa, int k, int nfree, int nfix0, double phi_pp, double cross,
                                                          double gd) {
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    CauchySortSeg o;
    o.phi_pp = phi_pp;
    o.t_prev = k > 0 ? sa.T[sa.inv[k - 1]] : 0.0;
    const int ik = k < nfree ? sa.inv[k] : -1;
    const double tk = ik >= 0 ? sa.T[ik] : INF;
    const bool fin = fabs(tk) < INF;
    o.theta = fin ? __dsub_rn(tk, o.t_prev) : INF;
    o.ind = fin ? ik : -1;
    o.phi_p = __dadd_rn(__dadd_rn(gd, cross), __dmul_rn(o.t_prev, o.phi_pp));
    o.bad = !(fabs(o.phi_p) < INF) || !(fabs(o.phi_pp) < INF);
    o.q = cauchy_decide(o.phi_p, o.phi_pp, o.theta, o.ind, nfix0 + k, sa.c.nmm);       // :615-636
    return o;
}

// The end of the search at segment ks (sg: its stop).  Hand-back: nothing of the search is written.  Else s_c, d, the active set,
// the loop state and the progress word.
__device__ __forceinline__ void cauchy_sort_finish(const CauchySortCore& sa, const CauchySortSeg& sg, int ks, int nfix0, bool hand_back) {
    const CauchyArgs& a = sa.c;
    CgState* st = a.st;
    const int tid = threadIdx.x;
    if (hand_back || sg.bad) {
        if (tid == 0) {
            *sa.flag = 0;
            st->done = 1; st->need_proj = 0;
            publish_cauchy_word(a, kCauchyHandBack, 1, 0, 1);
        }
        return;
    }
    const double step = sg.q.step, tstar = sg.t_prev;
    for (int i = tid; i < a.n; i += CS_SCAN_T) {
        const int r = sa.rank[i];
        if (r < 0) continue;                                           // fixed at the start: s_c = +0, d = 0 (cauchy_init_kernel)
        if (r < ks) {
            a.s[i] = sa.b[i];
            a.d[i] = 0.0; a.fixrank[i] = 0;                            // add_active!: fixvars[i] = true (poly:246); d_i = 0 (:632)
        } else {
            const double di = -a.g[i];
            a.s[i] = __dadd_rn(__dadd_rn(0.0, __dmul_rn(tstar, di)), __dmul_rn(step, di));     // :628 per segment, then :625
        }
    }
    if (tid == 0) {
        st->rtv = sg.phi_p; st->pHp = sg.phi_pp; st->gamma = sg.theta; st->alpha = sg.q.delta_t;
        st->n_hmul = ks + 1;
        st->approx_solved = sg.q.min_found; st->neg_curvature = sg.q.err;
        st->iter = nfix0 + ks; st->pad = ks;
        if (ks > 0) { const int il = sa.inv[ks - 1]; st->status = il; st->beta = -a.g[il]; }
        st->done = 1; st->need_proj = 0;
        publish_cauchy_word(a, sg.q.err, 1, ks, ks + 1);
    }
}

// 3. Scan, decision, write-back: one workgroup of 1024 threads.  Thread t owns the block of E = ceil((n + 1) / 1024) consecutive
// segments k = t E .. t E + E - 1 (k <= nfree).  The fixed order of the sums:
//   inside a block   prefix of c ascending from +0 (P_k = sum of c_r, lo <= r < k); suffix of shell and of g d descending from +0
//                    (W_k = term_k + W_{k+1});
//   inside a wave    the block totals behind lane l from lane 63 downwards (A = tot + A), before lane l from lane 0 upwards;
//   across waves     the wave totals behind wave w from wave 15 downwards, before wave w from wave 0 upwards;
//   phi''_k = W_k + (A + B),  sum_{r >= k} g_r d_r likewise,  sum_{r < k} c_r = (B + A) + P_k.
__global__ __launch_bounds__(CS_SCAN_T) void cauchy_sort_scan_kernel(CauchySortArgs sa) {
    constexpr int T = CS_SCAN_T, NW = T / 64;
    __shared__ double totC[T], totD[2][T];                            // block totals: c; shell and g d (the descending pair)
    __shared__ double wtC[NW], wtD[2][NW];
    __shared__ int kmin, nan_bound;
    const CauchyArgs& a = sa.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const int nfix0 = a.st->iter, nfree = n - nfix0;
    const int flag_in = *sa.flag;
    const int64_t sl = sa.ld + 16;
    const int E = (n + 1 + T - 1) / T;
    const int lo = min(tid * E, nfree + 1), hi = min(lo + E, nfree + 1);
    if (tid == 0) { kmin = 0x7fffffff; nan_bound = 0; }
    const bool nb = cauchy_sort_invert(sa);
    __syncthreads();
    if (nb) nan_bound = 1;                                             // (every writer stores the same value; read behind two more barriers)
    // ---- the terms of this block: prefix of c ascending; shell and g d parked, then their suffixes descending --------------------
    double p = 0.0;
    for (int k = lo; k < hi; ++k) {
        sa.scan[k] = p;
        CauchySortTerm t{0.0, 0.0, 0.0};
        if (k < nfree) t = cauchy_sort_term(sa, k);
        p = __dadd_rn(p, t.c);
        sa.scan[sl + k] = t.shell; sa.scan[2 * sl + k] = t.gd;
    }
    double ws = 0.0, wg = 0.0;
    for (int k = hi - 1; k >= lo; --k) {
        ws = __dadd_rn(sa.scan[sl + k], ws); wg = __dadd_rn(sa.scan[2 * sl + k], wg);
        sa.scan[sl + k] = ws; sa.scan[2 * sl + k] = wg;
    }
    totC[tid] = p; totD[0][tid] = ws; totD[1][tid] = wg;
    __syncthreads();
    double aD[2], bD[2];
    const double aC = cauchy_carry_before(totC + 64 * wave, lane);
    cauchy_carry_behind(&totD[0][64 * wave], T, 63, lane, aD);
    if (lane == 63) wtC[wave] = __dadd_rn(aC, p);
    if (lane == 0) { wtD[0][wave] = __dadd_rn(ws, aD[0]); wtD[1][wave] = __dadd_rn(wg, aD[1]); }
    __syncthreads();
    const double bC = cauchy_carry_before(wtC, wave);
    cauchy_carry_behind(&wtD[0][0], NW, NW - 1, wave, bD);
    const double offC = __dadd_rn(bC, aC), offS = __dadd_rn(aD[0], bD[0]), offG = __dadd_rn(aD[1], bD[1]);
    totC[tid] = offC; totD[0][tid] = offS; totD[1][tid] = offG;       // (every read of the block totals lies before the barrier above)
    // ---- the first segment of this block at which the search ends ----------------------------------------------------------------
    auto segment = [&](int k, double oC, double oS, double oG) {
        return cauchy_sort_stop(sa, k, nfree, nfix0, __dadd_rn(sa.scan[sl + k], oS), __dadd_rn(oC, sa.scan[k]), __dadd_rn(sa.scan[2 * sl + k], oG));
    };
    for (int k = lo; k < hi; ++k) {
        const CauchySortSeg sg = segment(k, offC, offS, offG);
        if (sg.q.done || sg.bad) { atomicMin(&kmin, k); break; }
    }
    __syncthreads();
    const int ks = kmin;                                               // (segment nfree always ends the search: nfix0 + nfree = n)
    const int owner = ks / E;
    cauchy_sort_finish(sa, segment(ks, totC[owner], totD[0][owner], totD[1][owner]), ks, nfix0, flag_in != 0 || nan_bound != 0);
}

}  // namespace bh
