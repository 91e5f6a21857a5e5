// How a handle reads G (bh_hess_set_gram_read): the rule alone, as a function of plain values (no HIP type, no library state), so
// that the host compiler can build it into a test program (tests/test_gram_read_cases_cpu.py).  The kernel behind the two lower
// reads is in bh_gramsym.hip.h, the launchers in bh_api.hip (launch_gram_hmul, launch_quad).
#pragma once
#include <cstdint>

namespace bh {

// the values of bh_hess_set_gram_read (BH_GRAM_READ_* of benlsip_hip.h)
enum GramReadMode : int {
    GRAM_READ_FULL = 0,          // every path is what it is without the switch
    GRAM_READ_LOWER = 1,         // products G·v read the lower triangle
    GRAM_READ_LOWER_QUAD = 2,    // ... and the quadratic forms v'Hv come from G
};

enum GramReadCall : int {
    GRAM_CALL_PRODUCT = 0,       // a product through launch_gram_hmul / an H*v of an implicit handle
    GRAM_CALL_QUAD = 1,          // a call that ends in the weighted square sum of launch_jv (vthv)
    GRAM_CALL_WHOLE_ROWS = 2,    // gram_cg_kernel, cauchy_gram_kernel, cauchy_gram_eq_kernel: contiguous whole rows of G
};

enum GramReadPath : int {
    GRAM_PATH_FULL = 0,          // the path of the handle's form as it is without the switch (products: all of G, or the sweep over J)
    GRAM_PATH_LOWER = 1,         // gram_symv_kernel<..., QUAD = 0> + the slab reduction
    GRAM_PATH_QUAD_FROM_G = 2,   // gram_symv_kernel<..., QUAD = 1> + the scalar reduction
    GRAM_PATH_SWEEP_J = 3,       // launch_jv over the image of J
};

struct GramReadIn {
    int mode;                    // GramReadMode, as remembered by the handle
    bool gram_form;              // the handle is in the Gram form now
    bool served;                 // the handle's width has a lower-triangle kernel (gram_read_served)
    int call;                    // GramReadCall
};

inline bool gram_read_mode_ok(int64_t mode) { return mode >= GRAM_READ_FULL && mode <= GRAM_READ_LOWER_QUAD; }

// Widths with a lower-triangle kernel: the register-resident row-stream geometries.  `last_geom_spill_free`: the build's verdict on
// the widest one (8192 < n <= 16384), whose product kernel parks v in LDS.
inline bool gram_read_served(int64_t nchunks, int64_t max_chunks, bool last_geom_spill_free) {
    if (nchunks < 1 || nchunks > max_chunks) return false;
    return nchunks <= max_chunks / 2 || last_geom_spill_free;
}

inline GramReadPath gram_read_path(const GramReadIn& in) {
    const bool lower = in.gram_form && in.served && in.mode >= GRAM_READ_LOWER;
    switch (in.call) {
        case GRAM_CALL_PRODUCT: return lower ? GRAM_PATH_LOWER : GRAM_PATH_FULL;
        case GRAM_CALL_QUAD: return (lower && in.mode == GRAM_READ_LOWER_QUAD) ? GRAM_PATH_QUAD_FROM_G : GRAM_PATH_SWEEP_J;
        default: return GRAM_PATH_FULL;
    }
}

// Bytes of G one lower-triangle launch loads: row i < n brings its 16-byte chunks 0 .. i/2 (the diagonal's chunk included).
inline double gram_read_lower_bytes(int64_t n) {
    const double m = (double)(n / 2);
    return 16.0 * ((n & 1) ? (m + 1.0) * (m + 1.0) : m * (m + 1.0));
}

// Serpentine index of pass p of workgroup b in a grid of G workgroups (b, 2G-1-b, 2G+b, ...): strictly increasing in p.  The pass
// sweeps row group ngroups - 1 - index, the heaviest groups first: two passes give every workgroup the same load, and the passes a
// grid cannot complete fall on the lightest groups, so the totals differ by less than one (the heaviest) row group.
// (constexpr: the kernel calls the same function)
constexpr int64_t gram_read_group(int64_t b, int64_t p, int64_t G) { return (p & 1) ? (p + 1) * G - 1 - b : p * G + b; }

}  // namespace bh
