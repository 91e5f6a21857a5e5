// Schedule of a Gram build that runs during the asynchronous upload of J (bh_hess_create_async, option "gram_ingest"): which
// 64 x 64 lower blocks of G = J'J + mu C'C can be computed once column chunk k has been transposed into the image, and the launch
// geometry of each such step.  Plain values only (no HIP type, no library state), so that the host compiler can build it into a
// test program (tests/test_gram_ingest_cpu.py).  The worker that follows it is in bh_api.hip (async_upload_worker), the kernels
// in bh_gngram.hip.h.
#pragma once
#include <algorithm>
#include <cstdint>

namespace bh {

constexpr int64_t kGramBlock = 64;          // block size of the Gram kernels (GNG_BS)

struct GramIngestPlan {
    int64_t ld;                  // leading dimension of the image = order of the padded G (a multiple of 16)
    int64_t chunk_cols;          // columns per upload chunk (a multiple of 32); the last chunk also writes the padding up to ld
    int64_t nchunks;
    int64_t nrows;               // rows of the image (d + q)
    int64_t n_cu;
    int64_t nb;                  // block rows of G
    int64_t part_doubles;        // the compact buffer of per-slab partial blocks: the largest step's need (0: every step has one slab)
};

// What is launched behind chunk k.  Block row b holds the lower blocks (b, 0..b): packed indices [b (b + 1) / 2, (b + 1)(b + 2) / 2),
// so the blocks of the rows [row_lo, row_hi) are the contiguous packed range [block_lo, block_lo + nblocks).
struct GramIngestStep {
    int64_t row_lo, row_hi;      // block rows of G that became complete with this chunk (empty: nothing to launch)
    int64_t block_lo, nblocks;
    int64_t nslabs, slab_rows;   // grid = nblocks x nslabs; slab s covers the image rows [s slab_rows, min(nrows, (s + 1) slab_rows))
    int64_t part_doubles;        // nslabs x nblocks x 64 x 64 when nslabs > 1, else 0 (the step stores straight into G)
};

// Block rows [0, result) are complete once chunks 0..k have been transposed: all 64 columns of each (up to ld in the last one)
// are in the image.  A chunk that is not the last ends before column n <= ld, so a partial last block waits for the last chunk,
// which writes every column up to ld.
inline int64_t gram_ingest_rows_done(const GramIngestPlan& p, int64_t k) {
    if (k < 0) return 0;
    if (k >= p.nchunks - 1) return p.nb;
    const int64_t cols = std::min(p.ld, (k + 1) * p.chunk_cols);
    return cols >= p.ld ? p.nb : cols / kGramBlock;
}

// Row slabs of an ingest step: the rule of the one-shot build (gram_geometry in bh_api.hip) applied to the blocks of the step — one
// slab when they outnumber the CUs (the step stores straight into G), else enough for ~2 workgroups per CU, each slab of at least
// ~256 rows and a multiple of 16.  Where the rows limit the slab count of the step and of the whole matrix alike, the slab
// boundaries are those of the one-shot build and the two G are bit-equal.
// Measured at config 3 (profiles/r11_gram_ingest_timing.txt): the Gram kernels hold one workgroup per CU (384 registers per lane), so
// a grid runs in ceil(workgroups / CUs) rounds of one slab each, and 2 CUs' worth of workgroups rounded up is three rounds for
// the work of two: 55 ms of step kernels against 40 ms for the one-shot build.  A rule that picks the slab count with the least
// rounds x rows per slab is the follow-up.
inline void gram_step_slab_rule(int64_t nblocks, int64_t nrows, int64_t n_cu, int64_t* nslabs, int64_t* slab_rows) {
    int64_t s = 1;
    if (nblocks < n_cu) s = std::max<int64_t>(1, std::min<int64_t>((2 * n_cu + nblocks - 1) / std::max<int64_t>(nblocks, 1), (nrows + 255) / 256));
    const int64_t rows = (std::max<int64_t>((nrows + s - 1) / s, 1) + 15) / 16 * 16;
    *nslabs = std::max<int64_t>(1, (nrows + rows - 1) / rows);
    *slab_rows = rows;
}

inline GramIngestStep gram_ingest_step(const GramIngestPlan& p, int64_t k) {
    GramIngestStep s{};
    s.row_lo = gram_ingest_rows_done(p, k - 1);
    s.row_hi = gram_ingest_rows_done(p, k);
    s.block_lo = s.row_lo * (s.row_lo + 1) / 2;
    s.nblocks = s.row_hi * (s.row_hi + 1) / 2 - s.block_lo;
    s.nslabs = 1;
    s.slab_rows = (std::max<int64_t>(p.nrows, 1) + 15) / 16 * 16;
    if (s.nblocks > 0) gram_step_slab_rule(s.nblocks, p.nrows, p.n_cu, &s.nslabs, &s.slab_rows);
    s.part_doubles = s.nslabs > 1 ? s.nslabs * s.nblocks * kGramBlock * kGramBlock : 0;
    return s;
}

inline GramIngestPlan gram_ingest_plan(int64_t ld, int64_t chunk_cols, int64_t nchunks, int64_t nrows, int64_t n_cu) {
    GramIngestPlan p{};
    p.ld = ld; p.chunk_cols = chunk_cols; p.nchunks = nchunks; p.nrows = nrows; p.n_cu = std::max<int64_t>(n_cu, 1);
    p.nb = (ld + kGramBlock - 1) / kGramBlock;
    for (int64_t k = 0; k < nchunks; ++k) p.part_doubles = std::max(p.part_doubles, gram_ingest_step(p, k).part_doubles);
    return p;
}

}  // namespace bh
