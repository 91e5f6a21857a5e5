// bh_gngram.hip.h — the explicit Gram form of the Gauss-Newton Hessian (bh_hess_set_form, BH_HESS_GRAM):
// G = sum_r w_r J_r' J_r  (w_r = 1 for the rows of J, mu for the rows of C) over the row-major padded image, on fp64 MFMA.
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
// G·v itself is row_stream_kernel<..., MODE_JV, ...> over the G image (bh_api.hip: launch_gram_hmul).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bh_proj.hip.h"   // dvec4

namespace bh {

// One workgroup per (64 x 64 lower block of G, row slab of the image).  A wave owns the whole block as 4 x 4
// v_mfma_f64_16x16x4_f64 tiles: per step of 4 rows, lane l reads the 32 contiguous bytes at columns c0 + 4 (l & 15) .. + 3 of
// row k0 + (l >> 4) for each of the two column blocks (one dwordx4 pair per operand, 512 contiguous bytes per row and block).
// Tile (ta, tb) takes element ta of the A load and element tb of the B load, so its MFMA index i (A's row, l & 15) stands for
// column I0 + 4 i + ta of J, and its index j (B's column, l & 15) for column J0 + 4 j + tb.  Both operands are rows of the same
// image and the same lane reads the same row for both, so the K index (l >> 4) needs no permutation.  C/D of the f64 MFMA:
// col = l & 15, row = (l >> 4) + 4 reg.
// The four waves take interleaved row steps of the slab and are combined through LDS in a fixed order ((w0 + w2) + (w1 + w3)):
// bit-reproducible.  Only entries with row >= col of G are kept; each is stored at (row, col) and (col, row), so G is exactly
// symmetric.  part == NULL: the result goes straight into G (one slab); else into slab blockIdx.y of part (ld x ld each, lower
// entries only), summed in slab order by gn_gram_reduce_kernel.
constexpr int GNG_T = 256;
constexpr int GNG_BS = 64;
__global__ __launch_bounds__(GNG_T) void gn_gram_mfma_kernel(const double* __restrict__ J, int64_t ld, int64_t nrows, int64_t d_rows,
                                                             double mu, int64_t slab_rows, double* __restrict__ G,
                                                             double* __restrict__ part) {
    __shared__ double red[2][64][64];                  // [slot][tile * 4 + reg][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // packed lower block index -> (bi, bj), bi >= bj
    const int e = blockIdx.x;
    int bi = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while ((bi + 1) * (bi + 2) / 2 <= e) ++bi;
    while (bi * (bi + 1) / 2 > e) --bi;
    const int bj = e - bi * (bi + 1) / 2;
    const int64_t ci = (int64_t)bi * GNG_BS + 4 * (lane & 15), cj = (int64_t)bj * GNG_BS + 4 * (lane & 15);
    const bool vi = ci < ld, vj = cj < ld;             // ld is a multiple of 16: a 4-column group is all in or all out
    const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
    const int64_t r1 = r0 + slab_rows < nrows ? r0 + slab_rows : nrows;

    dvec4 acc[4][4];
#pragma unroll
    for (int ta = 0; ta < 4; ++ta)
#pragma unroll
        for (int tb = 0; tb < 4; ++tb) acc[ta][tb] = dvec4{0.0, 0.0, 0.0, 0.0};

    auto fetch = [&](int64_t k0, dvec4& a, dvec4& b) {
        const int64_t row = k0 + (lane >> 4);
        a = b = dvec4{0.0, 0.0, 0.0, 0.0};
        if (row < r1) {
            const double* rp = J + row * ld;
            if (vi) a = *reinterpret_cast<const dvec4*>(rp + ci);
            if (vj) b = *reinterpret_cast<const dvec4*>(rp + cj);
            if (row >= d_rows) b *= mu;
        }
    };
    int64_t k0 = r0 + 4 * wave;
    dvec4 na, nb;
    fetch(k0, na, nb);
    for (; k0 < r1; k0 += 16) {
        const dvec4 a = na, b = nb;
        if (k0 + 16 < r1) fetch(k0 + 16, na, nb);      // next step's rows: in flight during the MFMAs
#pragma unroll
        for (int ta = 0; ta < 4; ++ta)
#pragma unroll
            for (int tb = 0; tb < 4; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
    }

    // fixed-order combination of the four waves
    auto put = [&](int slot) {
#pragma unroll
        for (int t = 0; t < 16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[slot][t * 4 + r][lane] = acc[t >> 2][t & 3][r];
    };
    auto add = [&](int slot) {
#pragma unroll
        for (int t = 0; t < 16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t >> 2][t & 3][r] += red[slot][t * 4 + r][lane];
    };
    if (wave >= 2) put(wave - 2);
    __syncthreads();
    if (wave < 2) add(wave);
    __syncthreads();
    if (wave == 1) put(0);
    __syncthreads();
    if (wave != 0) return;
    add(0);

    double* out = part != nullptr ? part + (int64_t)blockIdx.y * ld * ld : G;
#pragma unroll
    for (int ta = 0; ta < 4; ++ta)
#pragma unroll
        for (int tb = 0; tb < 4; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gr = (int64_t)bi * GNG_BS + 4 * ((lane >> 4) + 4 * r) + ta;
                const int64_t gc = (int64_t)bj * GNG_BS + 4 * (lane & 15) + tb;
                if (gr >= ld || gc > gr) continue;
                const double v = acc[ta][tb][r];
                out[gr * ld + gc] = v;
                if (part == nullptr) out[gc * ld + gr] = v;
            }
}

// Second stage of a build split over row slabs: G[i][j] = sum over slabs, in slab order, of the lower entry (max(i,j), min(i,j)).
__global__ __launch_bounds__(256) void gn_gram_reduce_kernel(const double* __restrict__ part, int nslabs, int64_t ld, double* __restrict__ G) {
    const int64_t total = ld * ld;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx / ld, j = idx - i * ld;
        const int64_t lo = i >= j ? i * ld + j : j * ld + i;
        double s = 0.0;
        for (int k = 0; k < nslabs; ++k) s += part[(int64_t)k * total + lo];
        G[idx] = s;
    }
}

}  // namespace bh
