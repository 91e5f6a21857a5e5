// bh_gngram.hip.h — the explicit Gram form of the Gauss-Newton Hessian (bh_hess_set_form, BH_HESS_GRAM):
// G = sum_r w_r J_r' J_r  (w_r = 1 for the rows of J, mu for the rows of C) over the row-major padded image, on fp64 MFMA.
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
// G·v itself is row_stream_kernel<..., MODE_JV, ...> over the G image (bh_api.hip: launch_gram_hmul), or under bh_hess_set_gram_read
// gram_symv_kernel over its lower triangle (bh_gramsym.hip.h).
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

// packed lower block index -> (bi, bj), bi >= bj
__device__ __forceinline__ void gn_gram_unpack(int e, int& bi, int& bj) {
    bi = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
    while ((bi + 1) * (bi + 2) / 2 <= e) ++bi;
    while (bi * (bi + 1) / 2 > e) --bi;
    bj = e - bi * (bi + 1) / 2;
}

// The body shared by the one-shot build and the panel build of an ingest step: block (bi, bj) over the image rows [r0, r1).
// Every thread of the workgroup calls it; true on wave 0 only, whose acc then holds the sum over the four waves.
__device__ __forceinline__ bool gn_gram_block(const double* __restrict__ J, int64_t ld, int64_t d_rows, double mu, int bi, int bj,
                                              int64_t r0, int64_t r1, double (*red)[64][64], dvec4 (&acc)[4][4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ci = (int64_t)bi * GNG_BS + 4 * (lane & 15), cj = (int64_t)bj * GNG_BS + 4 * (lane & 15);
    const bool vi = ci < ld, vj = cj < ld;             // ld is a multiple of 16: a 4-column group is all in or all out

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
    if (wave != 0) return false;
    add(0);
    return true;
}

__global__ __launch_bounds__(GNG_T) void gn_gram_mfma_kernel(const double* __restrict__ J, int64_t ld, int64_t nrows, int64_t d_rows,
                                                             double mu, int64_t slab_rows, double* __restrict__ G,
                                                             double* __restrict__ part) {
    __shared__ double red[2][64][64];                  // [slot][tile * 4 + reg][lane]
    const int lane = threadIdx.x & 63;
    int bi, bj;
    gn_gram_unpack((int)blockIdx.x, bi, bj);
    const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
    const int64_t r1 = r0 + slab_rows < nrows ? r0 + slab_rows : nrows;

    dvec4 acc[4][4];
    if (!gn_gram_block(J, ld, d_rows, mu, bi, bj, r0, r1, red, acc)) return;

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

// Panel variant for the build that follows an asynchronous upload (option "gram_ingest", bh_gram_ingest_plan.h): the grid is
// (the blocks of one step: packed indices block_lo + blockIdx.x) x (row slabs), so that a step of a few blocks still fills the chip.
// part == NULL (one slab): the block goes straight into G, as above.  Else the whole 64 x 64 block of slab blockIdx.y goes to
// part[(blockIdx.y * gridDim.x + blockIdx.x)][row in block][column in block] — a compact buffer of slabs x blocks x 4096 doubles
// instead of slabs x ld x ld — and gn_gram_panel_reduce_kernel sums the slabs in order.
__global__ __launch_bounds__(GNG_T) void gn_gram_panel_kernel(const double* __restrict__ J, int64_t ld, int64_t nrows, int64_t d_rows,
                                                              double mu, int64_t slab_rows, int block_lo, double* __restrict__ G,
                                                              double* __restrict__ part) {
    __shared__ double red[2][64][64];
    const int lane = threadIdx.x & 63;
    int bi, bj;
    gn_gram_unpack(block_lo + (int)blockIdx.x, bi, bj);
    const int64_t r0 = (int64_t)blockIdx.y * slab_rows;
    const int64_t r1 = r0 + slab_rows < nrows ? r0 + slab_rows : nrows;

    dvec4 acc[4][4];
    if (!gn_gram_block(J, ld, d_rows, mu, bi, bj, r0, r1, red, acc)) return;

    double* pb = part != nullptr ? part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (GNG_BS * GNG_BS) : nullptr;
#pragma unroll
    for (int ta = 0; ta < 4; ++ta)
#pragma unroll
        for (int tb = 0; tb < 4; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = 4 * ((lane >> 4) + 4 * r) + ta, lc = 4 * (lane & 15) + tb;
                const double v = acc[ta][tb][r];
                if (pb != nullptr) { pb[lr * GNG_BS + lc] = v; continue; }
                const int64_t gr = (int64_t)bi * GNG_BS + lr, gc = (int64_t)bj * GNG_BS + lc;
                if (gr >= ld || gc > gr) continue;
                G[gr * ld + gc] = v;
                G[gc * ld + gr] = v;
            }
}

// Second stage of a panel step: entry (row, col) of every block of the step, row >= col, row < ld, is the sum over the slabs in
// slab order; stored at (row, col) and (col, row).  One thread per entry of the nblocks x 64 x 64 panel.
__global__ __launch_bounds__(256) void gn_gram_panel_reduce_kernel(const double* __restrict__ part, int nslabs, int nblocks, int block_lo,
                                                                   int64_t ld, double* __restrict__ G) {
    const int64_t total = (int64_t)nblocks * (GNG_BS * GNG_BS);
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        int bi, bj;
        gn_gram_unpack(block_lo + (int)(idx / (GNG_BS * GNG_BS)), bi, bj);
        const int lr = (int)(idx / GNG_BS) % GNG_BS, lc = (int)(idx % GNG_BS);
        const int64_t gr = (int64_t)bi * GNG_BS + lr, gc = (int64_t)bj * GNG_BS + lc;
        if (gr >= ld || gc > gr) continue;
        double s = 0.0;
        for (int k = 0; k < nslabs; ++k) s += part[(int64_t)k * total + idx];
        G[gr * ld + gc] = s;
        G[gc * ld + gr] = s;
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
