// Policy and bookkeeping of the compact image of the free columns (option "free_image"): when the box-constrained CG loop of a
// handle streams Jf — one row per row of J, only the columns of the free variables, dense — instead of J, when Jf is built, and
// how it follows an active set that grows by a few variables between two calls.  Plain values only (no HIP type, no library
// state), so that the host compiler can build it into a test program (tests/test_free_image_cpu.py).  The driver that follows
// it is pcg_run in bh_api.hip, the kernels are in bh_freeimg.hip.h.
//
// All costs are in SWEEPS: one sweep = one H*p over the full image.  A call with nfix of n variables fixed and n_hmul products
// would have saved n_hmul * nfix / n sweeps on the compact image; that is the credit an eligible call earns while no image
// exists, and the saving the moves of a call are set against.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace bh {

// One build reads J once and writes Jf once.  Measured at config 3 (profiles/r12_free_image_timing.txt): 718 us as the caller sees
// it (a call that builds against calls served from the image, median of five rebuilds) against 303.7 us for one sweep.
constexpr double kFreeImageBuildSweeps = 2.4;
// One launch of free_image_move_kernel moves k columns (one 8-byte read and two 8-byte writes per row and column, strided by the
// row length) behind the upload of the k destinations.  Measured in the same file, as the caller sees it: 51 us for k = 1, 101 us
// for k = 8, 224 us for k = 64, that is 0.167, 0.331 and 0.737 sweeps; the line through the first and the last is used (it is
// 0.1 sweeps short at k = 8).
constexpr double kFreeImageMoveLaunchSweeps = 0.16;
constexpr double kFreeImageMoveColumnSweeps = 0.009;

// The loop on the compact image costs one launch more per call (the gather in front of it): 1.5-2.5 us
// (profiles/r03_grid_sync_probe.txt).  Under the policy a call is only considered when the bytes its sweeps would not read are worth
// about twice that at the streaming rate of 7.1 TB/s (profiles/r03_kernel_stats.csv): 32 MiB.  Small problems, whose CG iteration is
// bound by launch latency and not by the stream, therefore never build an image.
constexpr double kFreeImageMinSavedBytes = 32.0 * 1024.0 * 1024.0;

inline bool free_image_worthwhile(int64_t rows, int64_t nfix, int64_t n_hmul_predicted) {
    return 8.0 * (double)rows * (double)nfix * (double)std::max<int64_t>(n_hmul_predicted, 1) >= kFreeImageMinSavedBytes;
}

enum FreeImageAction {
    FI_FULL = 0,     // this call streams the full image
    FI_USE = 1,      // the compact image describes this call's active set as it is
    FI_BUILD = 2,    // build (or rebuild) the compact image for this call's active set, then use it
    FI_MOVE = 3      // apply the newly fixed variables as column moves, then use it
};
enum FreeImageState { FI_STATE_NONE = 0, FI_STATE_VALID = 1, FI_STATE_STALE = 2 };

// Host record of one handle's compact image.
struct FreeImageBook {
    bool present = false;            // an image exists and describes `mask`
    int64_t n = 0;                   // variables
    int64_t ldf = 0;                 // row stride of the image: the free count at build time rounded up to 16
    int64_t nfree = 0;               // live width (columns [nfree, ldf) are zero)
    std::vector<uint64_t> mask;      // fixvars (BitVector image, ceil(n / 64) words) of the active set the image describes
    std::vector<int32_t> map;        // slot -> original column, ldf entries, -1 from nfree on
    std::vector<int32_t> slot;       // original column -> slot, -1: not in the image
    double credit = 0.0;             // sweeps the calls so far would have saved
    int64_t builds = 0, moves = 0, served = 0;
};

inline bool free_image_bit(const uint64_t* m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1ull; }

inline int64_t free_image_count(const uint64_t* m, int64_t n) {
    int64_t c = 0;
    for (int64_t i = 0; i < n; ++i) c += free_image_bit(m, i) ? 1 : 0;
    return c;
}

// How `want` differs from the active set the image describes: variables fixed since (they can be moved out) and variables
// freed since (the image has lost their columns: it cannot serve).
inline void free_image_diff(const FreeImageBook& b, const uint64_t* want, int64_t* k_new, int64_t* k_freed) {
    int64_t a = 0, f = 0;
    const int64_t nwords = (b.n + 63) / 64;
    for (int64_t w = 0; w < nwords; ++w) {
        uint64_t have = b.mask[(size_t)w], wt = want[w];
        if (w == nwords - 1 && (b.n & 63)) { const uint64_t keep = (1ull << (b.n & 63)) - 1ull; have &= keep; wt &= keep; }
        a += __builtin_popcountll(wt & ~have);
        f += __builtin_popcountll(have & ~wt);
    }
    *k_new = a;
    *k_freed = f;
}

inline double free_image_saving(int64_t n_hmul, int64_t nfix, int64_t n) {
    return n > 0 ? (double)n_hmul * (double)nfix / (double)n : 0.0;
}
inline double free_image_move_cost(int64_t k) { return kFreeImageMoveLaunchSweeps + kFreeImageMoveColumnSweeps * (double)k; }

// The decision of one eligible call.  option: 0 off, 1 the policy, 2 build at the first eligible call and always move.
// rows: rows of the image; nfix: fixed variables of this call; k_new / k_freed: free_image_diff against the image (ignored when
// none exists); last_n_hmul: products of the previous call on the handle (the prediction for this one).
inline FreeImageAction free_image_decide(int option, bool present, int64_t rows, int64_t n, int64_t nfix, int64_t k_new, int64_t k_freed,
                                         double credit, int64_t last_n_hmul) {
    if (option == 0 || nfix <= 0 || nfix >= n) return FI_FULL;
    if (option == 1 && !free_image_worthwhile(rows, nfix, last_n_hmul)) return FI_FULL;
    if (present && k_freed == 0) {
        if (k_new == 0) return FI_USE;
        if (option == 2) return FI_MOVE;
        return free_image_move_cost(k_new) <= free_image_saving(last_n_hmul, nfix, n) ? FI_MOVE : FI_FULL;
    }
    // no image, or one that has lost a column this call needs (it never grows: it is built again)
    if (option == 2) return FI_BUILD;
    return credit >= kFreeImageBuildSweeps ? FI_BUILD : FI_FULL;
}

// Build: the free variables in index order.
inline void free_image_book_build(FreeImageBook& b, const uint64_t* want, int64_t n) {
    const int64_t nwords = (n + 63) / 64;
    b.n = n;
    b.mask.assign(want, want + nwords);
    b.slot.assign((size_t)n, -1);
    b.map.clear();
    for (int64_t i = 0; i < n; ++i)
        if (!free_image_bit(want, i)) { b.slot[(size_t)i] = (int32_t)b.map.size(); b.map.push_back((int32_t)i); }
    b.nfree = (int64_t)b.map.size();
    b.ldf = (std::max<int64_t>(b.nfree, 1) + 15) / 16 * 16;
    b.map.resize((size_t)b.ldf, -1);
    b.present = true;
    b.credit = 0.0;
    b.builds += 1;
}

// Moves (k_freed == 0 only): every newly fixed variable leaves the image; the holes below the new width are filled with the
// live columns of the tail, last live column first.  dst_of_tail[t - nfree_new] for the old columns t in [nfree_new, nfree_old):
// the slot that receives column t, or -1 (column t belonged to a newly fixed variable).  No slot is both read and written.
inline void free_image_book_move(FreeImageBook& b, const uint64_t* want, std::vector<int32_t>& dst_of_tail) {
    const int64_t nwords = (b.n + 63) / 64;
    const int64_t old_nfree = b.nfree;
    std::vector<int32_t> holes;
    for (int64_t s = 0; s < old_nfree; ++s)
        if (free_image_bit(want, b.map[(size_t)s])) holes.push_back((int32_t)s);
    const int64_t k = (int64_t)holes.size(), new_nfree = old_nfree - k;
    dst_of_tail.assign((size_t)k, -1);
    size_t h = 0;
    for (int64_t t = old_nfree - 1; t >= new_nfree; --t) {
        const int32_t var = b.map[(size_t)t];
        if (free_image_bit(want, var)) continue;                 // a hole in the tail: dropped with it
        const int32_t s = holes[h++];                             // (holes is ascending: those below new_nfree come first)
        dst_of_tail[(size_t)(t - new_nfree)] = s;
        b.map[(size_t)s] = var;
        b.slot[(size_t)var] = s;
    }
    for (int64_t i = 0; i < b.n; ++i)
        if (free_image_bit(want, i)) b.slot[(size_t)i] = -1;
    for (int64_t t = new_nfree; t < old_nfree; ++t) b.map[(size_t)t] = -1;
    b.nfree = new_nfree;
    b.mask.assign(want, want + nwords);
    b.moves += k;
}

// The compact image Af of the lineq matrix A (option "free_image_eq") lives beside Jf and shares its slot order.  It is stamped
// with the epoch of the constraint handle's active set (library-wide unique: it names the pair of constraint handle and active
// set).  Af serves a call iff its stamp is the epoch Jf describes and that is the calling constraint handle's; otherwise it is
// formed again through the current map (at most 2 MiB: never moved).  0 is "none" everywhere.
inline bool free_image_af_valid(uint64_t af_epoch, uint64_t fi_epoch, uint64_t mask_epoch) {
    return af_epoch != 0 && af_epoch == fi_epoch && fi_epoch == mask_epoch;
}

inline int free_image_state(const FreeImageBook& b, const uint64_t* current /* NULL: unknown */) {
    if (!b.present) return FI_STATE_NONE;
    if (current == nullptr) return FI_STATE_VALID;
    int64_t a = 0, f = 0;
    free_image_diff(b, current, &a, &f);
    return (a == 0 && f == 0) ? FI_STATE_VALID : FI_STATE_STALE;
}

}  // namespace bh
