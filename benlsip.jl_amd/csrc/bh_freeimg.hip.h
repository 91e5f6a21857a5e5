// bh_freeimg.hip.h — the compact image of the free columns (option "free_image"): build, column moves, the gather in front
// of the box-constrained CG loop that runs on it, the line search behind it (option "free_image_minor") and the accumulate of the
// resident inner-step chain behind that (option "free_image_chain")
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
//
// In the box-constrained CG loop every p_j is zero on the fixed variables, and their entries of H*p are used for nothing
// (src/basic_tralcnlss.jl:729-745: w += step p and r.v never see them).  Jf holds one row per row of the image of J and only
// the columns of the free variables, dense, row stride ldf: a sweep over it reads (n - nfix) / n of the bytes.  The policy is in
// bh_free_image_plan.h, the driver in pcg_run (bh_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bh_reduce.hip.h"
#include "bh_cg.hip.h"

namespace bh {

// Jf[row][c'] = J[row][map[c']] for c' < ldf (map[c'] < 0: zero padding).  One workgroup per row at a time, 16-byte stores;
// a pair of slots that maps to an aligned pair of neighbouring columns is read with one 16-byte load.
__global__ __launch_bounds__(256) void free_image_build_kernel(const double* __restrict__ J, int64_t ld, int64_t nrows,
                                                               const int* __restrict__ map, double* __restrict__ Jf, int64_t ldf) {
    const int nch = (int)(ldf >> 1);
    for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
        const double* __restrict__ src = J + row * ld;
        double2* __restrict__ dst = reinterpret_cast<double2*>(Jf + row * ldf);
        for (int c = threadIdx.x; c < nch; c += 256) {
            const int2 m = reinterpret_cast<const int2*>(map)[c];
            double2 x = make_double2(0.0, 0.0);
            if (m.x >= 0 && m.y == m.x + 1 && (m.x & 1) == 0) {
                const dvec2 t = __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(src + m.x));
                x = make_double2(t.x, t.y);
            } else {
                if (m.x >= 0) x.x = __builtin_nontemporal_load(src + m.x);
                if (m.y >= 0) x.y = __builtin_nontemporal_load(src + m.y);
            }
            dst[c] = x;
        }
    }
}

// The moves of one call: the old columns t in [nfree_new, nfree_new + k) leave the image.  dst_of_tail[t - nfree_new] >= 0: column
// t goes to that slot (a slot below nfree_new whose variable became fixed); either way column t is zero afterwards.  One thread
// per (row, t); no slot is both read and written (bh_free_image_plan.h).  Workgroup 0 also carries the slot -> column map along.
__global__ __launch_bounds__(256) void free_image_move_kernel(double* __restrict__ Jf, int64_t ldf, int64_t nrows, int nfree_new, int k,
                                                              const int* __restrict__ dst_of_tail, int* __restrict__ map) {
    const int64_t total = nrows * (int64_t)k;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t row = idx / k;
        const int t = (int)(idx - row * k);
        const int dst = dst_of_tail[t];
        double* __restrict__ rp = Jf + row * ldf;
        const double x = rp[nfree_new + t];
        if (dst >= 0) rp[dst] = x;
        rp[nfree_new + t] = 0.0;
    }
    if (blockIdx.x == 0) {
        for (int t = threadIdx.x; t < k; t += 256) {
            const int dst = dst_of_tail[t];
            const int var = map[nfree_new + t];
            if (dst >= 0) map[dst] = var;
            map[nfree_new + t] = -1;
        }
    }
}

// The one launch in front of the CG loop on the compact image: g, w_l, w_u gathered through the map (zero beyond nfree, up to
// n_pad), the caller's w zeroed on the fixed variables (the loop only ever writes the free ones).  A non-finite g on a FIXED
// variable makes r.v NaN in the loop on the full image (r = g there, NaN * 0); the compact loop never sees that entry, so such a
// call is handed back: `seq` goes into *reroute (every kernel of this call's compact loop then returns at once) and the
// progress word reports done with status kCgReroute, on which the host runs the call on the full image.
constexpr int kCgReroute = 15;
struct FreeGatherArgs {
    const double* g; const double* wl; const double* wu;      // n
    const int* fixrank;                                       // >= 0: fixed
    const int* map;                                           // ldf
    double* gc; double* wlc; double* wuc;                     // n_pad each
    double* wc;                                               // n_pad: the compact w (zeroed here)
    double* w;                                                // n: the caller's w
    int n, n_pad, nfree;
    unsigned long long* reroute; unsigned long long seq;
    unsigned long long* mirror; unsigned tag;
};

__global__ __launch_bounds__(256) void free_image_gather_kernel(FreeGatherArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.n_pad) {
        const int m = (i < a.nfree) ? a.map[i] : -1;
        a.gc[i] = (m >= 0) ? a.g[m] : 0.0;
        a.wlc[i] = (m >= 0) ? a.wl[m] : 0.0;
        a.wuc[i] = (m >= 0) ? a.wu[m] : 0.0;
        a.wc[i] = 0.0;
    }
    if (i < a.n && a.fixrank[i] >= 0) {
        a.w[i] = 0.0;
        const double gi = a.g[i];
        if (!(fabs(gi) <= 1.7976931348623157e308)) {          // NaN or +-Inf
            *a.reroute = a.seq;
            if (a.mirror != nullptr) {
                const unsigned long long wv = ((unsigned long long)(a.tag & 0xffffu) << 48) | ((unsigned long long)kCgReroute << 44) | (1ull << 40);
                __hip_atomic_store(a.mirror, wv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// minor_iterate's line search and scaling (src/basic_tralcnlss.jl:669-672) behind a CG loop that ran on the compact image (option
// "free_image_minor"): the operands are the compact vectors the loop left — g, w_l, w_u as the gather wrote them, w, and hw, the
// FREE part of H*w accumulated by cg_reduce_update_kernel.  w is zero on the fixed variables, so g.w and w.Hw over the nfree
// slots are the sums of linesearch_kernel without its zero terms, and no mask is needed: every live slot is free.  Slot i belongs
// to thread i mod CG_T in both passes, as in linesearch_kernel on n = nfree (linesearch_alpha is the shared arithmetic).
// The scaled w goes into the compact buffer and, from the same thread, into the caller's w at map[i]; alpha into out[0].
// The caller's w keeps the +0 the gather wrote on the fixed variables: with a negative or non-finite alpha linesearch_kernel would
// leave alpha * 0 there (-0 or NaN).  hw is not scaled: nothing reads it after this launch.
template <bool SCALE_HW, typename HW>
__device__ __forceinline__ void free_image_linesearch_body(const double* __restrict__ gc, double* __restrict__ wc, const double* __restrict__ wlc,
                                                           const double* __restrict__ wuc, HW* __restrict__ hwc, const int* __restrict__ map,
                                                           double* __restrict__ w_full, int nfree, double* __restrict__ out, double* scratch) {
    const double alpha = linesearch_alpha(gc, wc, wlc, wuc, nullptr, nullptr, hwc, nfree, scratch);
    for (int i = threadIdx.x; i < nfree; i += CG_T) {
        const double wi = __dmul_rn(alpha, wc[i]);          // :671
        wc[i] = wi;
        if constexpr (SCALE_HW) hwc[i] = __dmul_rn(alpha, hwc[i]);
        const int m = map[i];                                // (i < nfree: a column of the caller's w)
        if (m >= 0) w_full[m] = wi;
    }
    if (threadIdx.x == 0) out[0] = alpha;
}

__global__ __launch_bounds__(CG_T) void free_image_linesearch_kernel(const double* __restrict__ gc, double* __restrict__ wc,
                                                                     const double* __restrict__ wlc, const double* __restrict__ wuc,
                                                                     const double* __restrict__ hwc, const int* __restrict__ map,
                                                                     double* __restrict__ w_full, int nfree, double* __restrict__ out) {
    __shared__ double scratch[2 * (CG_T / 64)];
    free_image_linesearch_body<false>(gc, wc, wlc, wuc, hwc, map, w_full, nfree, out, scratch);
}

// The same behind a compact loop of the resident inner-step chain (option "free_image_chain", step_from_cg = 1): the thread that
// owns slot i also scales hwc[i], as linesearch_kernel does on the full vectors, so that hwc stays the free part of H*w for the
// scaled w — free_image_step_accumulate_kernel adds it to g_minor.  alpha, w and the caller's w are those of the kernel above.
__global__ __launch_bounds__(CG_T) void free_image_linesearch_scale_hw_kernel(const double* __restrict__ gc, double* __restrict__ wc,
                                                                              const double* __restrict__ wlc, const double* __restrict__ wuc,
                                                                              double* __restrict__ hwc, const int* __restrict__ map,
                                                                              double* __restrict__ w_full, int nfree, double* __restrict__ out) {
    __shared__ double scratch[2 * (CG_T / 64)];
    free_image_linesearch_body<true>(gc, wc, wlc, wuc, hwc, map, w_full, nfree, out, scratch);
}

// The model value q(s) = g.s + s'Hs / 2 carried along a chain of steps s += w (options "step_from_cg" and "free_image_chain"):
//   q(s + w) = q(s) + w.(H s + g) + w'Hw / 2 = q(s) + sum w_i gm_i + (sum w_i hw_i) / 2,   gm = H s + g BEFORE it is updated.
// w is zero on the fixed variables, so the sums need the free entries only.  sc: the workspace scalars — sc[4] is q; with
// q_mode = kStepQInit the chain has none yet and q(s) is formed from sc[2] = s.(gm - g), sc[3] = g.s, which
// model_from_gminor_kernel left on the still fully valid gm (the host's g.s + 0.5 s'Hs of bh_model_reduction_dev).
constexpr int kStepQNone = 0, kStepQCarry = 1, kStepQInit = 2;
constexpr int kStepQSlot = 4;
__device__ __forceinline__ void step_q_store(double* __restrict__ sc, int q_mode, double d1, double d2) {
    const double q = (q_mode == kStepQInit) ? __dadd_rn(sc[3], __dmul_rn(0.5, sc[2])) : sc[kStepQSlot];
    sc[kStepQSlot] = __dadd_rn(q, __dadd_rn(d1, __dmul_rn(0.5, d2)));
}

// bh_step_accumulate_dev behind a compact minor iterate of the chain: g_minor[map[c]] += hwc[c] over the nfree slots — the
// per-element arithmetic of vec_add_kernel on the scaled H*w, on the free variables only (the entries of g_minor on the fixed
// variables keep the value they had) — and q carried by the sums above over the slots.  One workgroup; slot c is on thread
// c mod CG_T in both passes, so no thread reads a word another thread writes.
__global__ __launch_bounds__(CG_T) void free_image_step_accumulate_kernel(const double* __restrict__ wc, const double* __restrict__ hwc,
                                                                          const int* __restrict__ map, double* __restrict__ gm, int nfree,
                                                                          double* __restrict__ sc, int q_mode) {
    __shared__ double scratch[2 * (CG_T / 64)];
    if (q_mode != kStepQNone) {
        double acc[2] = {0.0, 0.0};
        for (int c = threadIdx.x; c < nfree; c += CG_T) {
            const int m = map[c];
            if (m < 0) continue;
            const double wi = wc[c];
            acc[0] = fma(wi, gm[m], acc[0]);
            acc[1] = fma(wi, hwc[c], acc[1]);
        }
        block_reduce<CG_T, 2>(acc, scratch, OpSum(), 0.0);
        if (threadIdx.x == 0) step_q_store(sc, q_mode, acc[0], acc[1]);
    }
    for (int c = threadIdx.x; c < nfree; c += CG_T) {
        const int m = map[c];
        if (m >= 0) gm[m] = __dadd_rn(gm[m], hwc[c]);
    }
}

// The same carry in front of an accumulate on the full vectors (a full-image minor iterate inside a chain whose g_minor is already
// stale on the fixed variables): the sums run over all n entries, the terms on the fixed variables are +-0 x.  gm is only read.
__global__ __launch_bounds__(CG_T) void step_carry_q_kernel(const double* __restrict__ w, const double* __restrict__ hw,
                                                            const double* __restrict__ gm, int n, double* __restrict__ sc) {
    __shared__ double scratch[2 * (CG_T / 64)];
    double acc[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += CG_T) {
        const double wi = w[i];
        acc[0] = fma(wi, gm[i], acc[0]);
        acc[1] = fma(wi, hw[i], acc[1]);
    }
    block_reduce<CG_T, 2>(acc, scratch, OpSum(), 0.0);
    if (threadIdx.x == 0) step_q_store(sc, kStepQCarry, acc[0], acc[1]);
}

}  // namespace bh
