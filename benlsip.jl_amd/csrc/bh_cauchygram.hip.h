// bh_cauchygram.hip.h — the whole box-constrained Cauchy search from G = J'J + mu C'C in ONE launch (option "cauchy_gram")
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bh_reduce.hip.h"
#include "bh_cg.hip.h"
#include "bh_cauchy.hip.h"

namespace bh {

// ------------------------------------------------------------------------------------------
// cauchy_step (src/basic_tralcnlss.jl:574-639) on a Gram-form handle with box constraints.  d = P(-g) is -g_i while variable i is
// free and 0 once it is fixed, so fixing variable `ind` changes H*d by one column of G — one contiguous ROW of the image, because
// G is bitwise symmetric:
//     Hd <- Hd - d_ind G[ind, :] ,   d_ind <- 0 ,   phi' = s_c'Hd + g'd (:634) ,   phi'' = d'Hd (:635).
// Every step of a pass is O(n), so ONE workgroup runs the whole while loop (:615-637) on the device: no launch boundary and no
// host between two breakpoints, per breakpoint one dependent read of 8 ld bytes and one barrier.  Hd is the only downdated
// quantity (as t_d = J~ d is in the row-space form); the three dot products are full sums over n in a fixed order in every pass.
//
// Launched after cauchy_init_kernel (active_bounds!, d, d_l, d_u, s_c = 0) and one G d (Hd = H*d, :609).  Loop state and progress
// word are those of cauchy_advance_kernel, written once, when the loop has ended.
//
// Geometry: CA_T = 512 threads; a thread owns the element PAIRS (2 tid, 2 tid + 1) + 1024 j, so its share of a row of G is one
// 16-byte load per 1024 columns.
//   REG = true   n <= 4096: g, d_l, d_u, s_c, Hd (8 elements each) and the free flags stay in registers for the whole search;
//                the four row loads of a thread are issued before any is consumed.
//   REG = false  wider n (up to 16384): the vectors stay in the L2-resident CG workspace and are streamed in tiles of 4096 elements,
//                twice per pass (sums and arg-min, then the update); a thread reads and writes only elements it owns.
// Pad lanes (i >= n) hold g = s_c = Hd = 0 and count as fixed: neutral in every sum and absent from the arg-min.
// ------------------------------------------------------------------------------------------
struct CauchyGramArgs {
    CauchyArgs c;                // st, g, d, Hd, s, dl, du, fixrank, n, nmm, mirror, tag (as left by cauchy_init_kernel)
    const double* G; int64_t ld; // ld x ld row-major, padding rows and columns zero
};

template <bool REG>
__global__ __launch_bounds__(CA_T) void cauchy_gram_kernel(CauchyGramArgs ga) {
    constexpr int NW = CA_T / 64, E = 8, TILE = E * CA_T;
    __shared__ double scratch[2][5 * NW];        // s'Hd, d'Hd, g'd, theta, d of the arg-min — double-buffered: one barrier per pass
    __shared__ int iscratch[2][NW];
    const CauchyArgs& a = ga.c;
    CgState* st = a.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double* __restrict__ Hd = const_cast<double*>(a.Hd);
    int nfix = st->iter;
    int passes = st->n_hmul, bp = st->pad;

    double sv[E], hv[E], gv[E], lv[E], uv[E];
    unsigned freem = 0;                          // bit k: element k of the tile in registers is a free variable
    auto elem = [&](int base, int k) { return base + (k >> 1) * 2 * CA_T + 2 * tid + (k & 1); };
    auto load_tile = [&](int base) {
        freem = 0;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = elem(base, k), ic = min(i, n - 1);
            const double gi = a.g[ic], si = a.s[ic], hi = Hd[ic];
            lv[k] = a.dl[ic]; uv[k] = a.du[ic];
            const int f = a.fixrank[ic];
            const bool in = i < n;
            gv[k] = in ? gi : 0.0; sv[k] = in ? si : 0.0; hv[k] = in ? hi : 0.0;
            if (in && f < 0) freem |= 1u << k;
        }
    };
    if (REG) load_tile(0);
    const int nend = REG ? 1 : n;                // (REG: one tile, so the register arrays never depend on a loop counter)

    int done = 0, min_found = 0, err = 0, last_ind = -1;
    double phi_p = 0.0, phi_pp = 0.0, th_out = 0.0, delta_t = 0.0, d_last = 0.0;
    for (int pass = 0; pass <= n && !done; ++pass) {                  // at most n advances, then the while test (:615) fails
        const int buf = pass & 1;
        // ---- s_c'Hd, d'Hd, g'd and next_breakpoint (:536-562) over all of n --------------------------------------------------
        double x3[3] = {0.0, 0.0, 0.0};
        double th = INF, dbest = 0.0;
        int ind = 0x7fffffff;
        for (int base = 0; base < nend; base += TILE) {
            if (!REG) load_tile(base);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const bool fr = (freem >> k) & 1u;
                const double di = fr ? -gv[k] : 0.0;                  // d = projection(lincons, -g), box constraints (:592 / :632)
                x3[0] = fma(sv[k], hv[k], x3[0]);
                x3[1] = fma(di, hv[k], x3[1]);
                x3[2] = fma(gv[k], di, x3[2]);
                if (fr) {                                             // :547
                    const double t = cauchy_breakpoint_theta(di, sv[k], lv[k], uv[k]);
                    if (t < th) { th = t; ind = elem(base, k); dbest = di; }   // ascending index within a thread: strict < (:555)
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) x3[q] = wave_reduce(x3[q], OpSum());
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double t2 = __shfl_xor(th, off), d2 = __shfl_xor(dbest, off);
            const int i2 = __shfl_xor(ind, off);
            if (cauchy_theta_before(t2, i2, th, ind)) { th = t2; ind = i2; dbest = d2; }
        }
        if (lane == 0) {
            scratch[buf][wave] = x3[0]; scratch[buf][NW + wave] = x3[1]; scratch[buf][2 * NW + wave] = x3[2];
            scratch[buf][3 * NW + wave] = th; scratch[buf][4 * NW + wave] = dbest; iscratch[buf][wave] = ind;
        }
        __syncthreads();
        double shd = 0.0, dhd = 0.0, gd = 0.0;
        for (int w = 0; w < NW; ++w) { shd += scratch[buf][w]; dhd += scratch[buf][NW + w]; gd += scratch[buf][2 * NW + w]; }
        th = scratch[buf][3 * NW]; dbest = scratch[buf][4 * NW]; ind = iscratch[buf][0];
        for (int w = 1; w < NW; ++w) {
            const double t2 = scratch[buf][3 * NW + w];
            const int i2 = iscratch[buf][w];
            if (cauchy_theta_before(t2, i2, th, ind)) { th = t2; ind = i2; dbest = scratch[buf][4 * NW + w]; }
        }
        if (ind == 0x7fffffff) ind = -1;                              // :544
        phi_p = __dadd_rn(shd, gd);                                   // :610 / :634
        phi_pp = dhd;                                                 // :611 / :635
        const CauchyDecision q = cauchy_decide(phi_p, phi_pp, th, ind, nfix, a.nmm);      // :615-636
        done = q.done; min_found = q.min_found; err = q.err; th_out = th; delta_t = q.delta_t;
        passes += 1;
        // ---- s_c += step d (:625 / :628); on "next interval" fix `ind`: Hd -= d_ind G[ind, :], d_ind = 0 (:631-633) -------------
        if (q.step != 0.0 || q.advance) {
            const double* __restrict__ row = ga.G + (int64_t)(q.advance ? ind : 0) * ga.ld;
            for (int base = 0; base < nend; base += TILE) {
                double2 r[E / 2];
#pragma unroll
                for (int j = 0; j < E / 2; ++j) {                     // this thread's share of the row: every load out before any is used
                    const int col = base + j * 2 * CA_T + 2 * tid;
                    r[j] = make_double2(0.0, 0.0);
                    if (q.advance && col < ga.ld) r[j] = *reinterpret_cast<const double2*>(row + col);
                }
                if (!REG) load_tile(base);
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    const int i = elem(base, k);
                    if (i >= n) continue;
                    const bool fr = (freem >> k) & 1u;
                    const double di = fr ? -gv[k] : 0.0;
                    sv[k] = __dadd_rn(sv[k], __dmul_rn(q.step, di));
                    if (q.advance) {
                        hv[k] = __dsub_rn(hv[k], __dmul_rn(dbest, (k & 1) ? r[k >> 1].y : r[k >> 1].x));
                        if (i == ind) {                               // add_active!: fixvars[ind] = true (poly:246), by the thread that owns it
                            freem &= ~(1u << k);
                            a.fixrank[i] = 0; a.d[i] = 0.0;
                        }
                    }
                    if (!REG) { a.s[i] = sv[k]; Hd[i] = hv[k]; }
                }
            }
        }
        if (q.advance) { nfix += 1; bp += 1; last_ind = ind; d_last = dbest; }
    }
    if (REG) {
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = elem(0, k);
            if (i < n) { a.s[i] = sv[k]; Hd[i] = hv[k]; }
        }
    }
    if (tid == 0) {
        st->rtv = phi_p; st->pHp = phi_pp; st->gamma = th_out; st->alpha = delta_t;
        st->n_hmul = passes;
        st->approx_solved = min_found; st->neg_curvature = err;
        st->iter = nfix; st->pad = bp;
        if (last_ind >= 0) { st->status = last_ind; st->beta = d_last; }
        st->done = done; st->need_proj = done ? 0 : 1;
        publish_cauchy_word(a, err, done, bp, passes);
    }
}

}  // namespace bh
