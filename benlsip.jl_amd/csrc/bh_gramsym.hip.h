// bh_gramsym.hip.h — the Gram form read through its lower triangle (bh_hess_set_gram_read): G·v and v'Gv from the elements
// G_ij, j <= i, of the exactly symmetric ld x ld image.  The decision which calls come here is bh_gram_read_plan.h.
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bh_reduce.hip.h"
#include "bh_cg.hip.h"
#include "bh_gram_read_plan.h"

namespace bh {

struct GramSymArgs {
    const double* G;        // row-major ld x ld, bitwise symmetric
    int64_t ld;             // doubles per row (multiple of 16)
    int64_t nrows;          // rows swept: n (the rows beyond are zero, like the columns beyond)
    int nchunks;            // ld / 2
    const double* v;        // ld doubles, zero padded
    double* partials;       // QUAD = 0: gridDim.x x ld, one slab per workgroup (summed by the slab reduction of the row-stream kernels)
    double* sq_partials;    // QUAD = 1: gridDim.x, one partial of v'Gv per workgroup (summed in index order by reduce_scalar_kernel)
    const CgState* state;   // NULL, or skip the launch when state->done
    int negate;             // use -mask(v) instead of v, as row_stream_kernel does
    const int* negmask;     // fixrank (>= 0: fixed -> 0) or NULL, with negate
};

// The row-stream machinery of row_stream_kernel (thread t holds the 16-byte chunks t, t + T, ... of a row; non-temporal loads;
// the next row group on its way before the current one is reduced; butterfly + double-buffered LDS slot; no atomics) over the
// lower triangle:
//   * row i brings its chunks c <= i / 2 only: a load above the diagonal is never issued.  In the diagonal's chunk of an even row
//     the element at column i + 1 is dropped before it is used.
//   * row group g carries ~ g * R chunks, so a workgroup takes its groups in serpentine order, heaviest first (pass p sweeps group
//     ngroups - 1 - gram_read_group(b, p, G), the index running b, 2G-1-b, 2G+b, ...): every two passes give every workgroup the
//     same number of chunks and the incomplete passes fall on the lightest groups; the totals differ by less than one row group.
//   * QUAD = 0: t_i = sum_{j <= i} G_ij v_j is the row's dot product; z_j += v_i G_ij for j < i comes from the registers that
//     still hold the row (v_i is loaded with the row: nothing waits for the dot).  The thread that holds column i adds t_i to its
//     own z slot.  The workgroup's z goes to its slab; reduce_slabs sums the slabs in index order: y = G v, two launches, every
//     sum in a fixed order (rows in the order of the workgroup's passes, then slabs 0 .. gridDim.x - 1).
//   * QUAD = 1: no z, no slab.  Per row q_i = v_i (2 sum_{j < i} G_ij v_j + G_ii v_i); one partial per workgroup.
// VL: each lane parks its slice of v in LDS, lane-private slots as in row_stream_kernel (4096 < n <= 8192, product only: the two
// row buffers and z fill the registers).
template <int T, int CPT, int R, int QUAD, int VL = 0>
__global__ __launch_bounds__(T) void gram_symv_kernel(GramSymArgs a) {
    if (a.state != nullptr && a.state->done) return;
    constexpr int NW = T / 64;
    __shared__ double red[2][R][NW];
    extern __shared__ __attribute__((aligned(16))) double2 v_lds[];     // VL only: [CPT][T]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ld2 = a.ld >> 1;   // row stride in double2
    const double2* __restrict__ G2 = reinterpret_cast<const double2*>(a.G);
    const int64_t ngroups = (a.nrows + R - 1) / R;
    const int64_t NG = gridDim.x, b = blockIdx.x;

    bool act[CPT];
    double2 vv[CPT], zz[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) act[k] = (tid + k * T) < a.nchunks;

    double2 A[R][CPT], B[R][CPT];
    double viA[R], viB[R];           // v_i of the rows in flight
    double sq_acc = 0.0;
    int buf = 0;

    // v_i of row `row` (uniform): what the vector slice below holds at position `row`
    auto row_coef = [&](int64_t row) {
        double x = a.v[row];
        if (a.negate) x = (a.negmask != nullptr && a.negmask[row] >= 0) ? 0.0 : -x;
        return x;
    };

    auto load_group = [&](double2 (&dst)[R][CPT], double (&vi)[R], int64_t grp) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = grp * R + r;
            const bool rv = row < a.nrows;
            const double2* rp = G2 + (rv ? row : 0) * ld2;
            const int diag = rv ? (int)(row >> 1) : -1;                 // chunk of the diagonal: the last one of the row
            vi[r] = rv ? row_coef(row) : 0.0;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                dst[r][k] = make_double2(0.0, 0.0);
                if (tid + k * T <= diag) {
                    const dvec2 t = __builtin_nontemporal_load(reinterpret_cast<const dvec2*>(rp + tid + k * T));
                    dst[r][k] = make_double2(t.x, t.y);
                }
            }
        }
    };

    auto process = [&](double2 (&X)[R][CPT], double (&vi)[R], int64_t grp) {
        double s[R];
        double dg[R];                  // G_ii in the thread that holds it, 0 elsewhere
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = grp * R + r;
            const int diag = (int)(row >> 1);
            const bool odd = (row & 1) != 0;
            double acc = 0.0;
            dg[r] = 0.0;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                if (tid + k * T == diag) {
                    // the diagonal leaves the row buffer for a register of its own: the quadratic form counts it once and the rest
                    // twice, the product owes it no transposed contribution.  Column i + 1 of an even row (above the diagonal)
                    // goes with it: the chunk of an even row is left empty, that of an odd row keeps column i - 1.
                    dg[r] = odd ? X[r][k].y : X[r][k].x;
                    X[r][k].y = 0.0;
                    if (!odd) X[r][k].x = 0.0;
                }
                const double2 vk = VL ? v_lds[k * T + tid] : vv[k];
                acc = fma(X[r][k].x, vk.x, acc);
                acc = fma(X[r][k].y, vk.y, acc);
            }
            acc = fma(dg[r], vi[r], QUAD ? 2.0 * acc : acc);           // (v_i is this thread's own slice element where dg != 0)
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
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = grp * R + r;
            if (row >= a.nrows) continue;
            if (QUAD) {
                sq_acc = fma(vi[r], s[r], sq_acc);
            } else {
                const int diag = (int)(row >> 1);
                const bool odd = (row & 1) != 0;
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    // (the row buffer no longer holds G_ii: it is in t_i already); t_i lands in the slot of column i
                    const bool here = tid + k * T == diag;
                    zz[k].x = fma(vi[r], X[r][k].x, zz[k].x) + ((here && !odd) ? s[r] : 0.0);
                    zz[k].y = fma(vi[r], X[r][k].y, zz[k].y) + ((here && odd) ? s[r] : 0.0);
                }
            }
        }
    };

    int64_t p = 0, g = gram_read_group(b, 0, NG);
    // g, gn: serpentine indices; the row group is ngroups - 1 - index
    if (g < ngroups) load_group(A, viA, ngroups - 1 - g);      // the first row group does not depend on the vector slice: its loads go out first
    int2 nm[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int c = tid + k * T;
        vv[k] = make_double2(0.0, 0.0);
        zz[k] = make_double2(0.0, 0.0);
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
    if (VL) {
#pragma unroll
        for (int k = 0; k < CPT; ++k) v_lds[k * T + tid] = vv[k];     // read back only by this lane
    }

    if (g < ngroups) {
        while (true) {
            int64_t gn = gram_read_group(b, ++p, NG);
            if (gn < ngroups) load_group(B, viB, ngroups - 1 - gn);
            process(A, viA, ngroups - 1 - g);
            if (gn >= ngroups) break;
            g = gn;
            gn = gram_read_group(b, ++p, NG);
            if (gn < ngroups) load_group(A, viA, ngroups - 1 - gn);
            process(B, viB, ngroups - 1 - g);
            if (gn >= ngroups) break;
            g = gn;
        }
    }

    if (QUAD) {
        if (tid == 0) a.sq_partials[blockIdx.x] = sq_acc;
    } else {
        double2* out = reinterpret_cast<double2*>(a.partials) + (int64_t)blockIdx.x * ld2;
#pragma unroll
        for (int k = 0; k < CPT; ++k)
            if (act[k]) out[tid + k * T] = zz[k];
    }
}

}  // namespace bh
