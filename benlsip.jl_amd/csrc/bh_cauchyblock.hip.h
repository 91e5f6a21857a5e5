// bh_cauchyblock.hip.h — the one-kernel row-space Cauchy search, K breakpoints per launch (option cauchy_block)
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bh_cauchy.hip.h"

namespace bh {

// With box constraints the row update of a pass does not depend on that pass's sums: in the `advance` branch cauchy_decide sets
// step = theta and fixes ind, both from the n-vectors alone (s_c, g, d_l, d_u, the marks); phi', phi'' only decide whether the search
// stops here instead.  So one launch runs K advances ahead on the vector side, applies all K rank-one updates to its rows from
// registers and leaves K pairs of partial sums; the NEXT launch checks the K decisions in order.  At most K - 1 advances are thrown
// away, once, at the end of a search.  Every row performs cauchy_fused_kernel's operations in its order and every partial sum is
// reduced over the same grid in the same order: the result is bit-identical to the one-breakpoint-per-launch form.
//
// State j = the search after j advances; pass j (0-based) is the decision taken AT state j.  Launch 0 (J v + cauchy_image_kernel,
// first = 1) leaves the sums of state 0.  Block launch b >= 1 has base a_b = (b - 1) K:
//   verify     passes a_{b-1}+1 .. a_{b-1}+K-1 from the records and partial sums block b-1 left, then pass a_b from the last sum slot
//              of block b-1 (launch 0's sums when b = 1) and this launch's own first arg-min — by every workgroup, same operands, same
//              order, same bits.  The first pass that does not advance ends the search: the owners of the 64-element groups write
//              the final s_c (rebuilt from state a_{b-1} with the recorded thetas when the ending pass lies in the recorded range);
//   speculate  K passes from state a_b: arg-min, g'd, s += theta d, d_ind = 0, all from registers (n <= 4096 = 8 x CA_T);
//   rows       t_s, t_d once from memory, the K column entries of a row loaded together, K updates, K pairs of partial sums.
// Nothing a launch writes is read by the same launch:
//   s_c          three buffers: block b reads state a_b from (b-1) mod 3, writes state a_b + K to b mod 3, and on the finishing path
//                alone reads state a_{b-1} from (b-2) mod 3;
//   marks        fixpass[i] = the state from which i counts as fixed (-1: from the start, INT_MAX: free); block b treats i as fixed
//                iff fixpass[i] <= a_b, and the marks workgroup 0 sets in block b are > a_b: they read as free either way;
//   fixrank      written for VERIFIED advances only (block b confirms those of block b-1): no speculative mark reaches the active set;
//   records      two CauchyBlockRec, block b reads [(b+1) & 1], workgroup 0 writes [b & 1];  partial sums ping-pong.
constexpr int kCauchyBlockMaxK = 16;

// The loop state (its first five words are CauchyPass's: cauchy_init_kernel writes them through CauchyArgs::pp0) and what the
// speculation of one block launch leaves for the next: per pass a_b + j the arg-min (theta, ind, d_ind), g'd and — from `valid` —
// how far it got.  valid = V: records 0 .. V-1 are advances; V < K: record V is the pass the speculation stopped at (no candidate
// left, or every variable fixed), which ends the search.
struct CauchyBlockRec {
    int done, nfix, n_hmul, breakpoints, err, valid, pad0, pad1;
    double theta[kCauchyBlockMaxK], dind[kCauchyBlockMaxK], gd[kCauchyBlockMaxK];
    int ind[kCauchyBlockMaxK];
};

struct CauchyBlockArgs {
    CauchyBlockRec* rec; int b;              // block launch b >= 1
    const double* g; const double* dl; const double* du;
    double* sbuf[3];
    int* fixpass; int* fixrank;
    int n, nmm;
    const double* J; int64_t ld; int64_t nrows, d_rows; double mu;
    double* td; double* ts;
    const double* part_in; int Gin;          // b == 1: [2][Gin] from launch 0; b >= 2: [K][2][Gin] from block b - 1
    double* part_out;                        // [K][2][gridDim.x]
    unsigned long long* mirror; unsigned tag;
};

template <int K>
__global__ __launch_bounds__(CA_T) void cauchy_block_kernel(CauchyBlockArgs a) {
    static_assert(K >= 2 && K <= kCauchyBlockMaxK, "K");
    constexpr int NW = CA_T / 64;
    constexpr int E = 8;
    constexpr int SPW = (K + NW - 1) / NW;                     // sum slots a wave folds
    __shared__ double scratch[2][3 * NW];
    __shared__ int iscratch[2][NW];
    __shared__ double s_sum[K][2];
    __shared__ double s_th[K], s_dd[K];
    __shared__ int s_ind[K];
    __shared__ double r_th[K], r_gd[K];                        // the record of block b - 1, one load per thread
    __shared__ int r_ind[K];
    __shared__ double rscratch[2 * K * NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    const int b = a.b;
    const int a_b = (b - 1) * K, a_prev = (b - 2) * K;
    const CauchyBlockRec* in = a.rec + ((b + 1) & 1);
    CauchyBlockRec* out = a.rec + (b & 1);
    const double* __restrict__ s_in = a.sbuf[(b + 2) % 3];
    double* __restrict__ s_out = a.sbuf[b % 3];
    const bool wg0t0 = blockIdx.x == 0 && tid == 0;
    // ---- every load that does not depend on a decision goes out first ------------------------------------------------------------
    const int done_in = in->done, nh_in = in->n_hmul, bp_in = in->breakpoints, err_in = in->err;
    const int nfix_in = in->nfix, valid_in = (b > 1) ? in->valid : K;
    const int jr = min(tid, K - 1);
    const double rth = in->theta[jr], rgd = in->gd[jr];
    const int rind = in->ind[jr];
    // wave w folds the sum slots w, w + NW, ... of block b - 1 (launch 0's single pair stands in the last slot)
    LaneBatch<4> pb[SPW][2];
#pragma unroll
    for (int q = 0; q < SPW; ++q) {
        const int j = wave + q * NW;
        const double* p = (b > 1) ? a.part_in + (int64_t)min(j, K - 1) * 2 * a.Gin : a.part_in;
        pb[q][0].issue(p, a.Gin); pb[q][1].issue(p + a.Gin, a.Gin);
    }
    const int64_t r0 = (int64_t)blockIdx.x * CA_T + tid;
    const int64_t rc = min(r0, a.nrows > 0 ? a.nrows - 1 : (int64_t)0);
    const double td0 = a.td[rc], ts0 = a.ts[rc];
    double sv[E], gv[E], lv[E], uv[E];
    int fv[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = min(tid + k * CA_T, a.n - 1);
        sv[k] = s_in[i]; gv[k] = a.g[i]; lv[k] = a.dl[i]; uv[k] = a.du[i]; fv[k] = a.fixpass[i];
    }
    if (done_in) {                                   // over-launched: hand the final record on, touch nothing else
        if (wg0t0) { out->done = done_in; out->nfix = nfix_in; out->n_hmul = nh_in; out->breakpoints = bp_in; out->err = err_in; out->valid = 0; }
        return;
    }
    // ---- state a_b in registers; arg-min and g'd of one state (cauchy_fused_kernel's arithmetic, element for element) ------------
    double dv[E];
    bool fx[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
        fx[k] = fv[k] <= a_b;
        dv[k] = fx[k] ? 0.0 : -gv[k];                // d = projection(lincons, -g), box constraints (:592 / :632)
    }
    auto arg_min = [&](int buf, double& gd, double& th, int& ind, double& dbest, bool fold) {
        gd = 0.0; th = INF; dbest = 0.0; ind = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = tid + k * CA_T;
            if (i >= a.n) continue;
            gd = fma(gv[k], dv[k], gd);
            if (!fx[k]) {                                             // :547
                const double t = cauchy_breakpoint_theta(dv[k], sv[k], lv[k], uv[k]);
                if (t < th) { th = t; ind = i; dbest = dv[k]; }       // strict <: first minimiser in index order (:555)
            }
        }
        gd = wave_reduce(gd, OpSum());
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double t2 = __shfl_xor(th, off), d2 = __shfl_xor(dbest, off);
            const int i2 = __shfl_xor(ind, off);
            if (cauchy_theta_before(t2, i2, th, ind)) { th = t2; ind = i2; dbest = d2; }
        }
        if (lane == 0) { scratch[buf][wave] = gd; scratch[buf][NW + wave] = th; scratch[buf][2 * NW + wave] = dbest; iscratch[buf][wave] = ind; }
        if (fold) {                                   // (the first arg-min shares its barrier with the sums of block b - 1)
#pragma unroll
            for (int q = 0; q < SPW; ++q) {
                const int j = wave + q * NW;
                const double* p = (b > 1) ? a.part_in + (int64_t)min(j, K - 1) * 2 * a.Gin : a.part_in;
                const double shd = wave_sum(pb[q][0].fold_sum(p, a.Gin)), dhd = wave_sum(pb[q][1].fold_sum(p + a.Gin, a.Gin));
                if (lane == 0 && j < K && (b > 1 || j == 0)) { const int slot = (b > 1) ? j : K - 1; s_sum[slot][0] = shd; s_sum[slot][1] = dhd; }
            }
        }
        __syncthreads();
        gd = 0.0;
        for (int w = 0; w < NW; ++w) gd += scratch[buf][w];
        th = scratch[buf][NW]; dbest = scratch[buf][2 * NW]; ind = iscratch[buf][0];
        for (int w = 1; w < NW; ++w) {
            const double t2 = scratch[buf][NW + w];
            const int i2 = iscratch[buf][w];
            if (cauchy_theta_before(t2, i2, th, ind)) { th = t2; ind = i2; dbest = scratch[buf][2 * NW + w]; }
        }
        if (ind == 0x7fffffff) ind = -1;                              // :544
    };
    if (tid < K) { r_th[tid] = rth; r_gd[tid] = rgd; r_ind[tid] = rind; s_th[tid] = 0.0; s_dd[tid] = 0.0; s_ind[tid] = 0; }
    double gd0, th0, dbest0;
    int ind0;
    arg_min(0, gd0, th0, ind0, dbest0, true);
    // ---- verify: the decisions block b - 1 ran ahead of, in order, then pass a_b — by every workgroup ---------------------------------
    int nfix = nfix_in, nh = nh_in, bp = bp_in, err = err_in, done = 0;
    int fin = -1;                                    // the recorded pass a_{b-1} + fin ended the search (K: pass a_b)
    double step = 0.0;
    if (b > 1) {
#pragma unroll 1
        for (int j = 1; j < K && j <= valid_in && !done; ++j) {
            const double phi_p = __dadd_rn(s_sum[j - 1][0], r_gd[j]);                 // :610 / :634
            const CauchyDecision q = cauchy_decide(phi_p, s_sum[j - 1][1], r_th[j], r_ind[j], nfix, a.nmm);           // :615-636
            nh += 1;
            if (q.advance) {
                nfix += 1; bp += 1;
                if (wg0t0) a.fixrank[r_ind[j]] = 0;                   // add_active!: fixvars[ind] = true (poly:246)
            } else { done = 1; fin = j; step = q.step; err |= q.err; }
        }
    }
    if (!done) {
        const double phi_p = __dadd_rn(s_sum[K - 1][0], gd0);
        const CauchyDecision q = cauchy_decide(phi_p, s_sum[K - 1][1], th0, ind0, nfix, a.nmm);
        nh += 1;
        if (q.advance) {
            nfix += 1; bp += 1;
            if (wg0t0) a.fixrank[ind0] = 0;
        } else { done = 1; fin = K; step = q.step; err |= q.err; }
    }
    if (wg0t0 && a.mirror != nullptr) {              // passes = decisions taken, breakpoints = verified advances
        const unsigned long long wv = ((unsigned long long)(a.tag & 0xffffu) << 48) | ((unsigned long long)(err & 0xf) << 44) |
                                      ((unsigned long long)(done & 0xf) << 40) | ((unsigned long long)(bp & 0xfffff) << 20) |
                                      (unsigned long long)(nh & 0xfffff);
        __hip_atomic_store(a.mirror, wv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (done) {
        // ---- the final s_c (:625): the groups of 64 elements this workgroup owns --------------------------------------------------------
        const bool move = step != 0.0;
        if (fin < K) {
            // the ending pass lies in the recorded range: state a_{b-1}, the recorded thetas with d_i zeroed from its pass on
            const double* __restrict__ s_prev = a.sbuf[(b + 1) % 3];
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const int i = tid + k * CA_T;
                if (i < a.n) sv[k] = s_prev[i];
                dv[k] = (fv[k] <= a_prev) ? 0.0 : -gv[k];
            }
#pragma unroll 1
            for (int j = 0; j < fin; ++j) {
                const double th = r_th[j];
                const int ind = r_ind[j];
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    sv[k] = __dadd_rn(sv[k], __dmul_rn(th, dv[k]));
                    if (tid + k * CA_T == ind) dv[k] = 0.0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const int i = tid + k * CA_T;
            if (i < a.n && ((i >> 6) % (int)gridDim.x) == (int)blockIdx.x)
                s_out[i] = move ? __dadd_rn(sv[k], __dmul_rn(step, dv[k])) : sv[k];
        }
        if (wg0t0) { out->done = 1; out->nfix = nfix; out->n_hmul = nh; out->breakpoints = bp; out->err = err; out->valid = 0; }
        return;
    }
    // ---- speculate K passes from state a_b ------------------------------------------------------------------------------------------
    // (pass a_b has just advanced: nfix - 1 variables are fixed at state a_b)
    int V = 0;
    double gd = gd0, th = th0, dbest = dbest0;
    int ind = ind0;
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
        if (j > 0) arg_min(j & 1, gd, th, ind, dbest, false);
        if (wg0t0) { out->theta[j] = th; out->dind[j] = dbest; out->gd[j] = gd; out->ind[j] = ind; }
        if (ind < 0 || !(nfix - 1 + j < a.nmm)) break;                           // this pass ends the search: nothing to run ahead of
        if (tid == 0) { s_th[j] = th; s_dd[j] = dbest; s_ind[j] = ind; }
#pragma unroll
        for (int k = 0; k < E; ++k) {
            sv[k] = __dadd_rn(sv[k], __dmul_rn(th, dv[k]));                      // s_c += theta d     (:628)
            if (tid + k * CA_T == ind) { dv[k] = 0.0; fx[k] = true; }           // d[ind] = 0         (:632, box)
        }
        if (wg0t0) a.fixpass[ind] = a_b + j + 1;
        V = j + 1;
    }
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int i = tid + k * CA_T;
        if (i < a.n && ((i >> 6) % (int)gridDim.x) == (int)blockIdx.x) s_out[i] = sv[k];
    }
    if (wg0t0) { out->done = 0; out->nfix = nfix; out->n_hmul = nh; out->breakpoints = bp; out->err = err; out->valid = V; }
    __syncthreads();                                                            // s_th, s_dd, s_ind are in place
    // ---- this workgroup's rows: per pass t_s += theta t_d, t_d -= d_ind J~[:, ind], and the partial sums of the state behind it ----
    // (the slots from V on hold theta = 0, d_ind = 0, column 0: V < K means the next launch ends the search, and neither the images
    // nor the sums behind state a_b + V are read again)
    double acc[2 * K];
#pragma unroll
    for (int j = 0; j < 2 * K; ++j) acc[j] = 0.0;
    for (int64_t i = r0; i < a.nrows; i += (int64_t)gridDim.x * CA_T) {
        double td = (i == r0) ? td0 : a.td[i];
        double ts = (i == r0) ? ts0 : a.ts[i];
        double col[K];
#pragma unroll
        for (int j = 0; j < K; ++j) col[j] = a.J[i * a.ld + s_ind[j]];
        const double w = (i < a.d_rows) ? 1.0 : a.mu;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            ts = __dadd_rn(ts, __dmul_rn(s_th[j], td));
            td = __dsub_rn(td, __dmul_rn(s_dd[j], col[j]));
            acc[2 * j] = fma(w * ts, td, acc[2 * j]);
            acc[2 * j + 1] = fma(w * td, td, acc[2 * j + 1]);
        }
        a.td[i] = td;
        a.ts[i] = ts;
    }
    block_reduce<CA_T, 2 * K>(acc, rscratch, OpSum(), 0.0);
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            a.part_out[(int64_t)(2 * j) * gridDim.x + blockIdx.x] = acc[2 * j];
            a.part_out[(int64_t)(2 * j + 1) * gridDim.x + blockIdx.x] = acc[2 * j + 1];
        }
    }
}

}  // namespace bh
