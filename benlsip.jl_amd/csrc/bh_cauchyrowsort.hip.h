// bh_cauchyrowsort.hip.h — the box-constrained Cauchy search on an implicit handle from ONE sorted sweep over J (bh_hess_set_cauchy_rows, form 6)
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bh_reduce.hip.h"
#include "bh_cg.hip.h"
#include "bh_cauchy.hip.h"
#include "bh_cauchysort.hip.h"

namespace bh {

// ------------------------------------------------------------------------------------------
// cauchy_step (src/basic_tralcnlss.jl:574-639) with box constraints in the row space of J~ = [J; C] (weights w_i = 1 for the rows of
// J, mu for the rows of C), without the walk over the breakpoints.  As in bh_cauchysort.hip.h, d_i = -g_i while variable i is free,
// so the order pi in which variables are fixed is the sort order of (T_i, i) and is known before the first pass.  With
// a_ir = J~[i, pi(r)] (free variables only, in RANK order), per row i and segment k (the ranks < k fixed):
//     S_ik = sum_{r >= k} a_ir d_r                 (J~ d of segment k: a TRUE suffix sum, summed from the tail)
//     P_ik = sum_{r < k, T_r finite} a_ir b_r      (the part of J~ s_c already at its bounds: a prefix sum)
//     phi''_k = sum_i w_i S_ik^2                   (= d'Hd, :611 / :635)
//     X_k     = sum_i w_i P_ik S_ik
//     phi'_k  = (sum_{r >= k} g_r d_r + X_k) + T^(k) phi''_k          (= g'd + s_c'Hd, :610 / :634: J~ s_c = P + T^(k) S)
// and the search stops at the first k at which cauchy_decide is done.  Every segment has freshly summed images: nothing is carried
// through rank-one updates.
//
// Four launches behind cauchy_init_kernel, whatever the number of breakpoints:
//   1. cauchy_sort_rank_kernel        T_i, b_i, rank_i (bh_cauchysort.hip.h, unchanged)
//   2. cauchy_rowsort_rows_kernel     the only launch that reads J: per row the two scans in rank order, w S^2 and w P S added into
//                                     per-workgroup accumulators; one slab of 2 ld doubles per workgroup
//   3. cauchy_rowsort_reduce_kernel   the slabs summed over the workgroups in ascending order: phi''_k, X_k
//   4. cauchy_rowsort_scan_kernel     one workgroup: the suffix sums of g d, every decision, s_c, d, the active set, the loop state —
//                                     by the functions cauchy_sort_scan_kernel calls (cauchy_sort_stop, cauchy_sort_finish)
// Fixed orders everywhere (stated at each kernel), no atomics on doubles: a repeated search is bit-identical.  The bits depend on the
// grid of kernel 2 (which rows meet in which slab), as the row-stream slabs do.  Hand-back as in form 5: one code path.
//
// On a row-sharded handle (bh_hess_set_cauchy_rows_ranks) the kernels are the same: kernel 2 runs over this rank's rows (nrows = 0: a
// grid of 1, no row group, one slab of +0), and between kernels 3 and 4 the host enqueues ONE all-reduce of `red` (2 ld doubles:
// phi'', then X) — reduce_exchange_kernel with G = 0 or ncclAllReduce (bh_api.hip: cauchy_launch_sorted).  Kernel 4 then runs
// replicated on identical inputs.
// ------------------------------------------------------------------------------------------
constexpr int RS_T = 512;                // threads of cauchy_rowsort_rows_kernel
constexpr int RS_EPT = 8;                // consecutive ranks a thread owns: a row holds RS_T * RS_EPT = 4096 free entries
constexpr int RS_R = 2;                  // rows per group: one pair of barriers serves RS_R rows
constexpr int RS_MAXN = RS_T * RS_EPT;   // the widest padded row served (bh_cauchy_rows_plan.h: kCauchyRowsMaxN)
constexpr int RS_GRID_PER_CU = 1;        // persistent grid: min(row groups, RS_GRID_PER_CU * CUs) workgroups, one slab each
constexpr int RS_RED_T = 256;            // threads of cauchy_rowsort_reduce_kernel: one segment each
static_assert(RS_MAXN == 4096, "bh_cauchy_rows_plan.h: kCauchyRowsMaxN");

struct CauchyRowSortArgs : CauchySortCore {
    double* scan;                // [ld + 16] by rank: suffix of g d inside a thread's block
    const double* J; int64_t nrows, d_rows; double mu;      // the image: nrows x ld row-major, the rows >= d_rows are those of C
    double* slab;                // [grid][2][ld] by segment: w S^2, then w P S, of the rows of one workgroup
    double* red;                 // [2][ld] by segment: phi''_k, X_k
    int grid;                    // workgroups of kernel 2
};

// 2. Row scan.  Row group grp holds the image rows RS_R grp .. RS_R grp + RS_R - 1; workgroup x takes the groups x, x + grid, ...
// A row is loaded in 16-byte chunks (thread tid: the chunks tid + 512 c, c < 4; the next group's loads are issued before the current
// group's scans) and staged through LDS: column j is stored at position rank_j, the columns of variables fixed at the start are
// dropped.  Thread t then owns the ranks 8 t .. 8 t + 7 with d_r, b_r in registers.  The fixed order of the sums of one row:
//   inside a thread  suffix of a d descending from +0 (S_e = a_e d_e + S_{e+1}); prefix of a b ascending from +0;
//   inside a wave    Kogge-Stone over the thread totals: for off = 1, 2, .., 32: v_l = v_l + v_{l + off} (suffix; l + off < 64),
//                    v_l = v_{l - off} + v_l (prefix; l >= off); the exclusive value is the neighbour's inclusive one;
//   across waves     the wave totals behind wave w from wave 7 downwards, before wave w from wave 0 upwards;
//   S_ik = S_e + (excl + behind),  P_ik = (before + excl) + P_e;
//   per segment      acc = acc + (w S) S,  acc = acc + (w P) S  over the rows of the workgroup in ascending order.
// Every operation is a single rounding (no contraction): the CPU restatement (tests/rowsort_cases.py) does the same.
__global__ __launch_bounds__(RS_T) void cauchy_rowsort_rows_kernel(CauchyRowSortArgs ra) {
    constexpr int T = RS_T, E = RS_EPT, R = RS_R, NW = T / 64, CPT = RS_MAXN / 2 / T;
    __shared__ __attribute__((aligned(16))) double rowbuf[R][RS_MAXN];
    __shared__ unsigned short sinv[RS_MAXN];                          // rank -> column (0xffff: none); columns are below 4096
    __shared__ double wt[2][R][NW];
    const CauchyArgs& a = ra.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const int nfree = n - a.st->iter;                                  // (cauchy_init_kernel: the variables fixed at the start)
    const int64_t ld = ra.ld, ld2 = ld >> 1;
    const double2* __restrict__ J2 = reinterpret_cast<const double2*>(ra.J);
    const int ngroups = (int)((ra.nrows + R - 1) / R);
    const int NG = (int)gridDim.x;

    bool act[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) act[c] = (int64_t)(tid + c * T) < ld2;
    double2 A[R][CPT], B[R][CPT];
    auto load_group = [&](double2 (&dst)[R][CPT], int grp) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = (int64_t)grp * R + r;
            const bool rv = i < ra.nrows;
            const double2* rp = J2 + (rv ? i : 0) * ld2;
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
    if (g < ngroups) load_group(A, g);                                 // the first row group does not wait for the ranks
    int2 rk[CPT];                                                      // rank of this thread's columns (-1: not staged)
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        rk[c] = make_int2(-1, -1);
        if (act[c]) rk[c] = reinterpret_cast<const int2*>(ra.rank)[tid + c * T];
        if (rk[c].x >= RS_MAXN) rk[c].x = -1;                          // (never: ranks are below nfree <= n <= RS_MAXN)
        if (rk[c].y >= RS_MAXN) rk[c].y = -1;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
        sinv[tid + e * T] = 0xffffu;
#pragma unroll
        for (int r = 0; r < R; ++r) rowbuf[r][tid + e * T] = 0.0;      // positions >= nfree are never staged: they stay +0
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        if (rk[c].x >= 0) sinv[rk[c].x] = (unsigned short)(2 * (tid + c * T));
        if (rk[c].y >= 0) sinv[rk[c].y] = (unsigned short)(2 * (tid + c * T) + 1);
    }
    __syncthreads();
    double dr[E], br[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int r = tid * E + e;
        const int i = r < nfree && sinv[r] != 0xffffu ? (int)sinv[r] : -1;
        dr[e] = i >= 0 ? a.d[i] : 0.0;                                 // d_r = -g_r (cauchy_init_kernel)
        br[e] = i >= 0 ? ra.b[i] : 0.0;                              // b_r: 0 unless T_r is finite
    }
    double accS[E], accX[E];
#pragma unroll
    for (int e = 0; e < E; ++e) accS[e] = accX[e] = 0.0;

    auto process = [&](double2 (&X)[R][CPT], int grp) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < CPT; ++c) {
                if (rk[c].x >= 0) rowbuf[r][rk[c].x] = X[r][c].x;
                if (rk[c].y >= 0) rowbuf[r][rk[c].y] = X[r][c].y;
            }
        __syncthreads();
        double Ss[R][E], Pp[R][E], exS[R], exP[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double v[E];
            const double2* src = reinterpret_cast<const double2*>(&rowbuf[r][tid * E]);
#pragma unroll
            for (int e = 0; e < E / 2; ++e) { const double2 t = src[e]; v[2 * e] = t.x; v[2 * e + 1] = t.y; }
            double ts = 0.0, tp = 0.0;
#pragma unroll
            for (int e = E - 1; e >= 0; --e) { ts = __dadd_rn(__dmul_rn(v[e], dr[e]), ts); Ss[r][e] = ts; }
#pragma unroll
            for (int e = 0; e < E; ++e) { Pp[r][e] = tp; tp = __dadd_rn(tp, __dmul_rn(v[e], br[e])); }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const double us = __shfl_down(ts, off, 64), up = __shfl_up(tp, off, 64);
                if (lane + off < 64) ts = __dadd_rn(ts, us);
                if (lane >= off) tp = __dadd_rn(up, tp);
            }
            const double ns = __shfl_down(ts, 1, 64), np = __shfl_up(tp, 1, 64);
            exS[r] = lane < 63 ? ns : 0.0;
            exP[r] = lane > 0 ? np : 0.0;
            if (lane == 0) wt[0][r][wave] = ts;
            if (lane == 63) wt[1][r][wave] = tp;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = (int64_t)grp * R + r;
            if (i >= ra.nrows) continue;                                // (uniform over the workgroup)
            double bS = 0.0, bP = 0.0;
            for (int w = NW - 1; w > wave; --w) bS = __dadd_rn(wt[0][r][w], bS);
            for (int w = 0; w < wave; ++w) bP = __dadd_rn(bP, wt[1][r][w]);
            const double offS = __dadd_rn(exS[r], bS), offP = __dadd_rn(bP, exP[r]);
            const double w = i < ra.d_rows ? 1.0 : ra.mu;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double S = __dadd_rn(Ss[r][e], offS), P = __dadd_rn(offP, Pp[r][e]);
                accS[e] = __dadd_rn(accS[e], __dmul_rn(__dmul_rn(w, S), S));
                accX[e] = __dadd_rn(accX[e], __dmul_rn(__dmul_rn(w, P), S));
            }
        }
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
    double* out = ra.slab + (int64_t)blockIdx.x * 2 * ld;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int k = tid * E + e;
        if (k < (int)ld) { out[k] = accS[e]; out[ld + k] = accX[e]; }
    }
}

// 3. The slabs over the workgroups of kernel 2 in ascending order from +0; workgroup (x, y): segment 256 x + tid of sum y.
__global__ __launch_bounds__(RS_RED_T) void cauchy_rowsort_reduce_kernel(CauchyRowSortArgs ra) {
    const int64_t ld = ra.ld;
    const int64_t k = (int64_t)blockIdx.x * RS_RED_T + threadIdx.x;
    if (k >= ld) return;
    const double* p = ra.slab + (int64_t)blockIdx.y * ld + k;
    double acc = 0.0;
#pragma unroll 16
    for (int g = 0; g < ra.grid; ++g) acc = __dadd_rn(acc, p[(int64_t)g * 2 * ld]);
    ra.red[(int64_t)blockIdx.y * ld + k] = acc;
}

// 4. Scan, decision, write-back: one workgroup of 1024 threads, the tail of cauchy_sort_scan_kernel (bh_cauchysort.hip.h) called,
// not restated.  Thread t owns the block of E = ceil((n + 1) / 1024) consecutive segments.  sum_{r >= k} g_r d_r in that kernel's
// order: inside a block descending from +0 (W_k = g_k d_k + W_{k+1}); the block totals behind lane l from lane 63 downwards; the
// wave totals behind wave w from wave 15 downwards; the sum is W_k + (A + B).  phi''_k and X_k as kernel 3 left them (segment
// nfree: both +0).
__global__ __launch_bounds__(CS_SCAN_T) void cauchy_rowsort_scan_kernel(CauchyRowSortArgs ra) {
    constexpr int T = CS_SCAN_T, NW = T / 64;
    __shared__ double totG[T];
    __shared__ double wtG[NW];
    __shared__ int kmin, nan_bound;
    const CauchyArgs& a = ra.c;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const int nfix0 = a.st->iter, nfree = n - nfix0;
    const int flag_in = *ra.flag;
    const int E = (n + 1 + T - 1) / T;
    const int lo = min(tid * E, nfree + 1), hi = min(lo + E, nfree + 1);
    if (tid == 0) { kmin = 0x7fffffff; nan_bound = 0; }
    const bool nb = cauchy_sort_invert(ra);
    __syncthreads();
    if (nb) nan_bound = 1;                                             // (every writer stores the same value; read behind two more barriers)
    double wg = 0.0;
    for (int k = hi - 1; k >= lo; --k) {
        double t = 0.0;
        if (k < nfree) { const double gi = a.g[ra.inv[k]]; t = __dmul_rn(gi, -gi); }
        wg = __dadd_rn(t, wg);
        ra.scan[k] = wg;
    }
    totG[tid] = wg;
    __syncthreads();
    double aG[1], bG[1];
    cauchy_carry_behind(totG + 64 * wave, T, 63, lane, aG);
    if (lane == 0) wtG[wave] = __dadd_rn(wg, aG[0]);
    __syncthreads();
    cauchy_carry_behind(wtG, NW, NW - 1, wave, bG);
    const double offG = __dadd_rn(aG[0], bG[0]);
    totG[tid] = offG;                                                  // (every read of the block totals lies before the barrier above)
    auto segment = [&](int k, double oG) {
        return cauchy_sort_stop(ra, k, nfree, nfix0, k < nfree ? ra.red[k] : 0.0, k < nfree ? ra.red[ra.ld + k] : 0.0, __dadd_rn(ra.scan[k], oG));
    };
    for (int k = lo; k < hi; ++k) {
        const CauchySortSeg sg = segment(k, offG);
        if (sg.q.done || sg.bad) { atomicMin(&kmin, k); break; }
    }
    __syncthreads();
    const int ks = kmin;                                               // (segment nfree always ends the search: nfix0 + nfree = n)
    cauchy_sort_finish(ra, segment(ks, totG[ks / E]), ks, nfix0, flag_in != 0 || nan_bound != 0);
}

}  // namespace bh
