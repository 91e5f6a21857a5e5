// bh_cauchygrameq.hip.h — the Cauchy search with linear equalities from G = J'J + mu C'C (option "cauchy_gram_eq", form 4)
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bh_cg.hip.h"
#include "bh_proj.hip.h"
#include "bh_cauchy.hip.h"

namespace bh {

// The linear-equality form of the row-space search (CauchyImgGenArgs, bh_cauchy.hip.h) restated in the column space of G.  With
// d = P(-g) = -D g - D A'y  (D = mask of the free variables, y = (A_free A_free')^{-1} A_free(-g), left in ProjArgs::tw)
//     Hd = G d = -a - B y ,    a = G D g  (n) ,    B = G D A'  (n x mA, column j at B + j * ld)
// and fixing variable `ind` is  a -= g_ind G[ind, :],  B -= G[ind, :]' A[:, ind]'  — ONE CONTIGUOUS ROW of G (G is bitwise
// symmetric), where the row space needs a strided column of J, and n elements per vector instead of d + q.  phi' and phi'' are then
// dot(s_c, H*d) + g.d and dot(d, H*d) as the reference forms them (src/basic_tralcnlss.jl:610-611, :634-635): Hd goes to the
// advance kernel in its non-image mode.
//
// a and B cost one G v launch and one GEMM over n rows (image_b_mfma_kernel with J := G), microseconds — so every
// kCauchyGramEqRefresh-th pass the host forms them again from the device-side mask instead of carrying thousands of rank-one
// updates; the pass behind a formation runs with fresh = 1 (the mask already holds the variable fixed in between).
struct CauchyGramEqArgs {
    const CgState* st;
    const double* G; int64_t ld;      // ld x ld row-major, zero padded
    int n, mA;
    double* a;                        // ld
    double* B;                        // mA x ld
    const double* A; int64_t ldA;     // row-major mA x ldA image of lineq
    const double* tw;                 // y (mA), written by the factor-and-solve launch of this pass
    const double* g;
    double* Hd;                       // ld (zero on the pad)
    int fresh;                        // a, B have just been formed for the current mask: no rank-one update
};

// A workgroup of 256 threads owns 16 consecutive elements (one 128-byte line of every vector): lane = (element e = lane & 15,
// column slice lane >> 4), so the 16 column groups g = 4 wave + slice hold cpg = ceil(mA / 16) <= 4 columns of B each — n = 4096
// is 256 workgroups, one per CU, and a thread has at most 4 + 4 + 4 + 3 loads.  Two dependent rounds, as in the row-space form:
// (loop state, a, B, y) first, then what needs `ind` (the row of G, the column of A, g_ind).  The 16 partial dot products of an
// element meet in a fixed order: the four slices of a wave by shuffles, (0 + 1) + (2 + 3), the four waves through LDS in
// ascending order.  No atomics; no thread reads what another thread of the launch writes.
__device__ __forceinline__ void cauchy_gram_eq_rows_body(const CauchyGramEqArgs& ga, int block) {
    __shared__ double s_dot[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = lane & 15, grp = 4 * wave + (lane >> 4);
    const int i = block * 16 + e;
    const bool vi = i < ga.n;
    const int ic = vi ? i : ga.n - 1;
    const int cpg = (ga.mA + 15) >> 4, j0 = grp * cpg;
    const bool owner = grp == 0;                                   // this thread keeps a_i and writes Hd_i
    // ---- round 1: everything that does not need `ind` ------------------------------------------------------------------------
    const int ind = ga.st->status;
    double b[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int jj = min(j0 + k, ga.mA - 1);
        b[k] = (k < cpg) ? ga.B[(int64_t)jj * ga.ld + ic] : 0.0;           // (k < cpg is uniform over the launch)
        y[k] = (k < cpg) ? ga.tw[jj] : 0.0;
    }
    double ai = owner ? ga.a[ic] : 0.0;
    // ---- round 2: the row of G, the column of A and g_ind of the variable fixed at the last breakpoint (clamped index: the
    //      loads go out together whether or not the update is applied) ----------------------------------------------------------
    const bool upd = !ga.fresh && ind >= 0;
    const int indc = max(ind, 0);
    const double col = ga.G[(int64_t)indc * ga.ld + ic];
    const double g_ind = ga.g[indc];
    double acol[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acol[k] = (k < cpg) ? ga.A[(int64_t)min(j0 + k, ga.mA - 1) * ga.ldA + indc] : 0.0;
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int jj = j0 + k;
        if (k < cpg && jj < ga.mA) {
            double bij = b[k];
            if (upd) { bij = __dsub_rn(bij, __dmul_rn(col, acol[k])); if (vi) ga.B[(int64_t)jj * ga.ld + i] = bij; }
            dot = fma(bij, y[k], dot);
        }
    }
    if (owner && upd) { ai = __dsub_rn(ai, __dmul_rn(g_ind, col)); if (vi) ga.a[i] = ai; }
    const double p0 = __shfl(dot, e), p1 = __shfl(dot, e + 16), p2 = __shfl(dot, e + 32), p3 = __shfl(dot, e + 48);
    if (lane < 16) s_dot[wave][e] = __dadd_rn(__dadd_rn(p0, p1), __dadd_rn(p2, p3));
    __syncthreads();
    if (owner) {                                                   // wave 0, lanes 0..15: every element of the tile, pad included
        double hd = -ai;                                           // Hd = -a - B y
        hd = __dsub_rn(hd, s_dot[0][e]); hd = __dsub_rn(hd, s_dot[1][e]);
        hd = __dsub_rn(hd, s_dot[2][e]); hd = __dsub_rn(hd, s_dot[3][e]);
        if (i < ga.ld) ga.Hd[i] = vi ? hd : 0.0;
    }
}

// One launch per pass next to the factor-and-solve launch and the decision, mirroring cauchy_gen_rows_and_d_kernel: the first
// `row_blocks` workgroups form Hd (and carry a, B over the last breakpoint), the next `d_blocks` form d = P(-g) = -g_free - A_free'y
// (proj_left_mul_tr_kernel<true, 4>'s arithmetic), the last mA form t_fresh = A_free(-g) for the CURRENT active set: the next
// pass's right-hand side is this value minus the column of the variable the decision in between fixes (cauchy_factor_solve_kernel).
__global__ __launch_bounds__(256) void cauchy_gram_eq_kernel(CauchyGramEqArgs ga, int row_blocks, int d_blocks, ProjArgs pa,
                                                             const double* __restrict__ r, double* __restrict__ d_out,
                                                             double* __restrict__ t_fresh) {
    if (ga.st->done) return;
    const int b = (int)blockIdx.x;
    if (b < row_blocks) {
        cauchy_gram_eq_rows_body(ga, b);
    } else if (b < row_blocks + d_blocks) {
        proj_left_mul_tr_body<true, 4>(pa, r, d_out, b - row_blocks);
    } else {
        ProjArgs pf = pa;
        pf.tw = t_fresh;
        proj_left_mul_body(pf, r, b - row_blocks - d_blocks);
    }
}

}  // namespace bh
