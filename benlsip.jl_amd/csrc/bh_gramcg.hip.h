// bh_gramcg.hip.h — first kernel of the fused CG iteration on a Gram-form handle (option "gram_cg_fused")
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
//
// The Gram counterpart of row_stream_kernel<..., MODE_FUSED, CGP = 1> (bh_matvec.hip.h): launch j forms p_j = -v + beta p_{j-1}
// on the fly from what the update kernel of iteration j-1 left behind, takes the loop's exit test on the way in, and streams
// the ld x ld image of G = J'J + mu C'C once:
//   Hp[row]        stored directly, one whole vector (no slabs: a row of G is dotted with p by ONE workgroup);
//   sqpart[wg]     this workgroup's share of p'Hp = dot(p, H*p) as the reference forms it (src/basic_tralcnlss.jl:723): the sum
//                  over its rows of p_j[row] * Hp[row], in row order.  p_j[row] is recomputed from v[row], p_{j-1}[row] and beta
//                  with the operations of the prologue (same bits as the stored p_j), because the owner of CHUNK row/2 of p_j is
//                  in general another workgroup and nobody may read what this launch writes;
//   gpart[wg]      min of the factor_to_boundary terms of the chunks of p_j this workgroup owns (-> gamma).
// cg_reduce_update_kernel<GEN, false> follows with Hp as its only "slab" (Gs = 1) and sums the partials in workgroup order.
// The ping-pong of p, the r.v partials and the gamma partials, the stop_at gate and the progress word are those of the
// implicit form's two- / three-kernel iteration.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bh_reduce.hip.h"
#include "bh_cg.hip.h"
#include "bh_matvec.hip.h"

namespace bh {

// a: J = G, ld, nrows = ld, nchunks, v / negate / negmask (launch 1: p_1 = -mask(g) on the fly, or p_1 itself with init_done != 0),
// t_out = Hp, cf = the CG prologue's operands (CgFuse: sqpart receives the partials of dot(p, H*p)).
// NOPF = 1: the same code as a separate symbol for the launch the host expects to find the loop finished — no prefetch of G
// before the exit test (as CGP = 2 of the row-stream kernel).  Either symbol does the right thing if the prediction is wrong.
template <int T, int CPT, int R, int NOPF>
__global__ __launch_bounds__(T) void gram_cg_kernel(RowStreamArgs a) {
    const CgFuse& f = a.cf;
    CgState* st = f.st;
    if (f.j > 1 && st->stop_at != 0 && f.j > st->stop_at) return;       // the loop stopped before this iteration
    static_assert(R <= 16, "the R products p[row] * Hp[row] of a row group are summed inside one 16-lane DPP row");
    constexpr int NW = T / 64;
    __shared__ double red[2][R][NW];
    __shared__ double pro[2][NW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ld2 = a.ld >> 1;   // row stride in double2
    const double2* __restrict__ G2 = reinterpret_cast<const double2*>(a.J);
    const int64_t ngroups = (a.nrows + R - 1) / R;
    const int64_t G = gridDim.x;

    bool act[CPT];
    double2 vv[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        act[k] = (tid + k * T) < a.nchunks;
        vv[k] = make_double2(0.0, 0.0);
    }

    double2 A[R][CPT], B[R][CPT];
    double sq_acc = 0.0;
    double beta = 0.0;
    int buf = 0;

    auto load_group = [&](double2 (&dst)[R][CPT], int64_t grp) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = grp * R + r;
            const bool rv = row < a.nrows;
            const double2* rp = G2 + (rv ? row : 0) * ld2;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                dst[r][k] = make_double2(0.0, 0.0);
                if (rv && act[k]) {
                    const dvec2 t = __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(rp + tid + k * T));
                    dst[r][k] = make_double2(t.x, t.y);
                }
            }
        }
    };

    // p_j[grp * R + tid] for the threads tid < R (0 elsewhere and on rows past the image): the operations of the prologue below
    auto row_p = [&](int64_t grp) -> double {
        const int64_t row = grp * R + tid;
        double pr = 0.0;
        if (tid < R && row < a.nrows) {
            if (f.j == 1) {
                pr = a.v[row];
                if (a.negate) {
                    const int fixed = (a.negmask != nullptr) ? a.negmask[row] : -1;
                    pr = (fixed >= 0) ? 0.0 : -pr;
                }
            } else {
                pr = __dadd_rn(-f.vvec[row], __dmul_rn(beta, f.p_old[row]));       // :745
            }
        }
        return pr;
    };

    auto process = [&](double2 (&X)[R][CPT], int64_t grp) {
        const double pr = row_p(grp);                   // asked for first: it arrives while the rows are reduced
        double s[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                acc = fma(X[r][k].x, vv[k].x, acc);
                acc = fma(X[r][k].y, vv[k].y, acc);
            }
            s[r] = wave_sum(acc);
        }
        if (NW > 1) {
            if (lane == 0) {
#pragma unroll
                for (int r = 0; r < R; ++r) red[buf][r][wave] = s[r];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) t += red[buf][r][w];
                s[r] = t;
            }
            buf ^= 1;
        }
        // the R results of the group leave in ONE store instruction (lanes 0..R-1 of wave 0, R*8 contiguous bytes)
        double mine = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (tid == r) mine = s[r];
        const int64_t row = grp * R + tid;
        if (tid < R && row < a.nrows) a.t_out[row] = mine;
        // p'Hp: the group's R products in lane order (DPP row sum; the other lanes hold +0), then onto the workgroup's running sum —
        // only thread 0's copy is stored
        sq_acc = __dadd_rn(sq_acc, row16_sum(__dmul_rn(pr, mine)));
    };

    int64_t g = blockIdx.x;
    if (f.j == 1) {
        // the first row group does not depend on the vector: its loads go out first
        if (g < ngroups) load_group(A, g);
        // (all loads first, the masking afterwards: a compare next to its load makes the compiler wait for each chunk in turn)
        int2 nm[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int c = tid + k * T;
            nm[k] = make_int2(-1, -1);
            if (act[k]) {
                vv[k] = reinterpret_cast<const double2*>(a.v)[c];
                if (a.negate && a.negmask != nullptr) nm[k] = reinterpret_cast<const int2*>(a.negmask)[c];
            }
        }
        if (a.negate) {
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                vv[k].x = (nm[k].x >= 0) ? 0.0 : -vv[k].x;
                vv[k].y = (nm[k].y >= 0) ? 0.0 : -vv[k].y;
            }
        }
        // projected_cg's initialisation (:702-718) belongs to workgroup 0: r = g, v = P(r) = mask(g), p = -v (formed above),
        // rtv = r.v, tol_cg = kappa2*||v||, iter = 1, all flags down
        if (blockIdx.x == 0 && f.init_done != 1) {
            double t = 0.0, vsq = 0.0;
            if (f.init_done == 2) {
                // linear equalities: v = P(g), p_1 = -v are in memory (proj_apply_linv_kernel<INIT>), which also left the
                // partials of r.v and of v.v (every wave gets the same sums)
                t = wave_fixed_sum(f.rvpart, f.nrv);
                vsq = wave_fixed_sum(f.rvpart + f.vv_off, f.nrv);
            } else {
                double rtv0 = 0.0;
#pragma unroll
                for (int k = 0; k < CPT; ++k) {        // vv = -mask(g):  r.v = v.v = sum of squares of the free components
                    rtv0 = fma(vv[k].x, vv[k].x, rtv0); rtv0 = fma(vv[k].y, vv[k].y, rtv0);
                }
                rtv0 = wave_sum(rtv0);
                if (lane == 0) pro[0][wave] = rtv0;
                __syncthreads();
                for (int w2 = 0; w2 < NW; ++w2) t += pro[0][w2];
                vsq = t;
            }
            if (tid == 0) {
                st->rtv = t;                                   // :707  (r.v; box: v = mask(r))
                st->tol_cg = f.kappa2 * sqrt(vsq);             // :710
                st->pHp = 0.0; st->alpha = 0.0; st->gamma = 0.0; st->beta = 0.0;
                st->iter = 1; st->max_iter = f.max_iter;
                st->approx_solved = 0; st->outside_region = 0; st->neg_curvature = 0;
                st->n_hmul = 0; st->need_proj = 0; st->done = 0; st->status = 4; st->stop_at = 0;
                tie_reset(st);
            }
        }
    } else {
        // expected to go on: the first row group of G goes out FIRST — loads return in order, so the prologue's own operands
        // (v, p, the r.v partials: L2 hits) arrive right behind it.  If the loop turns out to have stopped, what this workgroup
        // asked for is simply dropped.
        if (!NOPF && g < ngroups) load_group(A, g);
        // (CPT = 16: v and p_{j-1} pass through the registers in two halves — both whole next to the two row buffers and p_j would
        // not fit the 256 registers a lane has at 8 waves per workgroup; the second half costs one more L2 round trip per launch)
        constexpr int KB = CPT >= 16 ? CPT / 2 : CPT;
        double2 vk[KB], po[KB];
        auto load_vp = [&](int k0) {
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                vk[k] = po[k] = make_double2(0.0, 0.0);
                if (act[k0 + k]) {
                    vk[k] = reinterpret_cast<const double2*>(f.vvec)[tid + (k0 + k) * T];
                    po[k] = reinterpret_cast<const double2*>(f.p_old)[tid + (k0 + k) * T];
                }
            }
        };
        load_vp(0);
        const double rtv = st->rtv, tol_cg = st->tol_cg;
        TieRegs tr;                                                        // (uniform loads, issued with the rest)
        tr.load(st);
        const int outside_prev = st->outside_region, neg_prev = st->neg_curvature;
        const double rtv_next = wave_fixed_sum(f.rvpart, f.nrv);          // :743, same bits in every wave of every workgroup
        const bool solved = fabs(rtv_next) < tol_cg;                       // :747
        const bool stop = solved || f.j > f.max_iter;                      // :720 with iter = j after :748
        beta = __ddiv_rn(rtv_next, rtv);                                   // :744
        if (blockIdx.x == 0 && tid == 0) {
            tr.note(TIE_TOL, rel_margin(fabs(rtv_next), tol_cg), f.j - 1);
            tr.store(st);
            if (f.trace != nullptr && f.j - 1 <= f.trace_cap) f.trace[4 * (int64_t)(f.j - 2) + 3] = rtv_next;
            st->iter = f.j;                        // :748 (nobody reads it back: the kernels count iterations by launch)
            int status = 4;
            if (stop) {
                status = cg_status_of(solved ? 1 : 0, outside_prev, neg_prev, f.j, f.max_iter);
                st->beta = beta; st->rtv = rtv_next; st->approx_solved = solved ? 1 : 0;
                st->done = 1; st->stop_at = f.j - 1;
                st->status = status;
            }
            // "stopped after iteration j-1", or "iter = j: iteration j is streaming" (n_hmul = j - 1 either way)
            publish_word(f.mirror, f.tag, status, stop ? 1 : 0, f.j, f.j - 1, tr);
        }
        if (stop) return;
        if (NOPF && g < ngroups) load_group(A, g);                         // the prediction was wrong: carry on
#pragma unroll
        for (int k0 = 0; k0 < CPT; k0 += KB) {
            if (k0 > 0) load_vp(k0);
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                vv[k0 + k].x = __dadd_rn(-vk[k].x, __dmul_rn(beta, po[k].x));       // :745
                vv[k0 + k].y = __dadd_rn(-vk[k].y, __dmul_rn(beta, po[k].y));
            }
        }
    }
    // the chunks this workgroup owns (runs of CPT consecutive chunks, run r belongs to workgroup r % gridDim.x): store p_j; the
    // workgroup's share of gamma = factor_to_boundary(p, w, w_l, w_u) (:734 / :728)
    {
        OpMinNan opmin;
        double gm = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int c = tid + k * T;
            if (!act[k] || ((c / CPT) % (int)G) != (int)blockIdx.x) continue;
            reinterpret_cast<double2*>(f.p_new)[c] = vv[k];
            double2 wk = make_double2(0.0, 0.0);
            if (f.j > 1) wk = reinterpret_cast<const double2*>(f.w)[c];
            const double2 lo = reinterpret_cast<const double2*>(f.wl)[c], hi = reinterpret_cast<const double2*>(f.wu)[c];
            if (2 * c < f.n) gm = opmin(gm, f2b_term(vv[k].x, wk.x, lo.x, hi.x, f.atol_f2b));
            if (2 * c + 1 < f.n) gm = opmin(gm, f2b_term(vv[k].y, wk.y, lo.y, hi.y, f.atol_f2b));
        }
        gm = wave_min(gm);
        if (NW > 1) {
            if (lane == 0) pro[1][wave] = gm;                  // (pro[0] belongs to workgroup 0's initialisation above)
            __syncthreads();
            gm = pro[1][0];
            for (int w2 = 1; w2 < NW; ++w2) gm = opmin(gm, pro[1][w2]);
        }
        if (tid == 0) f.gpart[blockIdx.x] = gm;
    }

    if (g < ngroups) {
        while (true) {
            int64_t gn = g + G;
            if (gn < ngroups) load_group(B, gn);
            process(A, g);
            if (gn >= ngroups) break;
            g = gn;
            gn = g + G;
            if (gn < ngroups) load_group(A, gn);
            process(B, g);
            if (gn >= ngroups) break;
            g = gn;
        }
    }
    if (tid == 0) f.sqpart[blockIdx.x] = sq_acc;
}

}  // namespace bh
