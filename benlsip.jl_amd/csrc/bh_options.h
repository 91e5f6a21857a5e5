// The options of bh_set_option: the fields with their defaults, and ONE table that says for every key where it is stored, which values
// it admits, what becomes of any other value, and which environment variable sets its initial value at bh_init.  Plain values only (no
// HIP type, no library state: tests/test_options_cpu.py).  A new option is one field, one row, one entry in include/benlsip_hip.h.
#pragma once
#include "../../include/benlsip_hip.h"   // the BH_* codes
#include "bh_cauchy_plan.h"              // cauchy_block_value_ok

#include <array>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

namespace bh {

struct Options {
    int64_t opt_blocks_per_cu = 0;   // 0 = per-config default
    int64_t opt_batch = 0;           // CG iterations launched ahead of the host's done-flag poll; 0 = by problem size (auto_batch)
    // Cauchy search, per breakpoint: 0 = downdate the Gram matrix A_free A_free' and refactor it (O(mA^3), the default: its
    // factor is as accurate as the reference's from-scratch rebuild), 1 = for mA > 64: rank-one downdate of the factor itself
    // (O(mA^2)), refreshed from scratch every kDowndateRefresh breakpoints.  Errors accumulate over the downdates — measured on the
    // 48-parameter NLS (mA = 2, when the one-wave kernel for mA <= 64 still existed): after 29 of them a search direction P(-g)
    // with ||g||/||P(-g)|| = 1.7e7 took one more breakpoint than the oracle; after 40, with A_free A_free' close to singular, the
    // projections had left null(A).  Up to 64 rows the refactoring path costs the same, so it is the only one there.
    int64_t opt_chol_downdate = 0;
    // bh_cauchy_step with box constraints on one rank: 1 = image-space search (J d and J s_c maintained by rank-one column updates:
    // one J v sweep at the start, then no sweep over J per breakpoint), 0 = one H*d sweep per breakpoint as the reference does
    int64_t opt_cauchy_image = 1;
    int64_t opt_cauchy_image_max_ma = 64;   // ... and with up to this many linear equalities (0..64)
    int64_t opt_cauchy_image_refresh = 0;   // row-space search, one rank: R >= 1 forms t_d, t_s (a, B, t_s) again from J every R-th pass (0: never)
    int64_t opt_cauchy_fused = 1;           // box constraints, one rank, row-space form: ONE kernel per breakpoint (cauchy_fused_kernel)
    int64_t opt_cauchy_block = 0;           // ... and K = 2, 4, 8 or 16 breakpoints per launch of it (cauchy_block_kernel<K>; 0, 1: one)
    int64_t opt_cauchy_gram_eq = 0;         // Gram-form handle, 1 <= mA <= 64, one rank: the search with linear equalities from G (cauchy_gram_eq_kernel)
    int64_t opt_cauchy_gram = 0;            // Gram-form handle, box constraints, one rank: the whole search from G in one launch (cauchy_gram_kernel)
    int64_t opt_linv_refine = 1;            // explicit-inverse projection (three-kernel CG iteration): one step of iterative refinement of y
    int64_t opt_cauchy_gemm = 1;            // B = J D A' of that form in one sweep on the matrix cores (0: mA J v sweeps over masked rows of A)
    int64_t opt_gram_cg_fused = 0;          // Gram-form handle: fused CG iteration (gram_cg_kernel + update: two kernels; <= 64 equalities: three)
    int64_t opt_gram_mfma = 1;       // A_free A_free': 1 = matrix cores when mA > 96, 2 = always, 0 = never (one wave per entry, VALU)
    int64_t opt_ls_from_cg = 1;      // minor_iterate: linesearch's w'Hw from the H*w accumulated by the CG loop
    // bh_step_accumulate_dev right behind the bh_minor_iterate_dev that produced its w: g_minor += H*w with the H*w that CG loop
    // accumulated (scaled with w by the line search) instead of a fresh sweep H*s + g over J — one H-product less per minor iterate.
    // Opt-in: it relies on the CALLER'S invariant that g_minor_out holds H*s + g for the current s (true in inner_step,
    // src/basic_tralcnlss.jl:412,:434-437; the library's resident inner-step mirrors switch it on around their loop)
    int64_t opt_step_from_cg = 0;
    int64_t opt_fold_init = 1;       // box CG: fold the initialisation into the first H*p / step launches
    int64_t opt_final_sync = 0;      // *_dev: always drain the stream before returning (1), or only wait for what the host is owed (0)
    int64_t opt_host_copy_kernels = 1;   // host vectors of the host-pointer entry points: copy kernels on the mapped pinned arena (1) or DMA (0)
    int64_t opt_cg_fused = 1;        // box CG: two kernels per iteration (H*p with the p-update folded in + reduce/update) instead of three
    int64_t opt_proj_form = 1;       // 1: reduced mA x mA form (fast), 0: the reference's augmented mpp x mpp form
    int64_t opt_upload_chunk_mb = 64; // bh_hess_create_async: MiB of J per pipelined column chunk
    int64_t opt_free_image = 1;      // box CG loop, one rank: stream the compact image of the free columns (0 off, 1 by the policy of bh_free_image_plan.h, 2 always)
    // bh_minor_iterate* with ls_from_cg = 1 and step_from_cg = 0: the call is considered for the compact image like a bh_pcg* (the
    // loop accumulates the free part of H*w, free_image_linesearch_kernel takes the line search on the compact operands); 0: never
    int64_t opt_free_image_minor = 0;
    // the same with step_from_cg = 1, the resident inner-step chain: the line search keeps cg.hwc scaled with w, bh_step_accumulate_dev
    // adds it to g_minor on the free variables only and carries the model value q(s) in cg.scalars[kStepQSlot], which
    // bh_model_reduction_dev then returns — no sweep over J anywhere in the chain; 0: such calls stay on the full image
    int64_t opt_free_image_chain = 0;
    // the three-kernel equality loop (reduced form, mA <= 64, one rank, implicit form, no H*w) on the compact image too, with a
    // compact image Af of the lineq matrix beside Jf, under the rules of free_image (0 off, 1 on)
    int64_t opt_free_image_eq = 0;
    int64_t opt_gram_ingest = 0;     // bh_hess_create_async, one rank, n <= 16384: the handle is born in the Gram form, G built during the upload
    int64_t opt_ev_stride = 8;       // BH_FLAG_PROFILE: hipEvents around every opt_ev_stride-th H*p launch of a handle
    int64_t opt_image_pool = 2;      // images kept (0: free at once)
};

// What becomes of a value that is not admissible.  OPT_COERCE: any non-zero value is 1 (range 0..1); OPT_CLAMP: the nearest end of the
// range; OPT_REJECT (bh_set_option): BH_ERR_INVALID_ARG with the row's text, OPT_IGNORE (environment): nobody is told, and the option
// keeps its value; OPT_STORE: stored as it is; OPT_CALLER: a known key that is no field of Options, the caller of option_set handles it.
enum OptionOutside : int { OPT_COERCE, OPT_CLAMP, OPT_REJECT, OPT_IGNORE, OPT_STORE, OPT_CALLER };

struct OptionRow {
    const char* key;
    int64_t Options::*field;                 // nullptr with OPT_CALLER
    int64_t lo, hi;                          // the admissible values, both ends included (`ok`, where they are no range)
    OptionOutside outside;                   // ... through bh_set_option
    const char* reject = "";                 // OPT_REJECT: bh_last_error_detail
    const char* env = nullptr;               // the variable bh_init reads, once, for the initial value
    OptionOutside env_outside = OPT_IGNORE;  // ... through it
    bool (*ok)(int64_t) = nullptr;
    bool needs_init = false;                 // a non-zero value is BH_ERR_NOT_INIT before bh_init, whatever the value
};
constexpr int kOptionCount = 31;

// max_blocks_per_cu: the partial-slab capacity of a handle (kMaxBlocksPerCu of bh_api.hip, which sizes the buffers with it).
constexpr std::array<OptionRow, kOptionCount> option_table(int64_t max_blocks_per_cu) {
    return {{
        {"blocks_per_cu", &Options::opt_blocks_per_cu, 0, max_blocks_per_cu, OPT_REJECT, "blocks_per_cu must be 0 (default) .. 8", "BH_BLOCKS_PER_CU", OPT_CLAMP},
        {"pcg_batch", &Options::opt_batch, 0, INT64_MAX, OPT_CLAMP, "", "BH_PCG_BATCH", OPT_CLAMP},
        {"proj_form", &Options::opt_proj_form, 0, 1, OPT_COERCE, "", "BH_PROJ_FORM", OPT_COERCE},
        {"fold_init", &Options::opt_fold_init, 0, 1, OPT_COERCE},
        {"cg_fused", &Options::opt_cg_fused, 0, 2, OPT_REJECT, "cg_fused is 0, 1 (box constraints) or 2 (also linear equalities)", "BH_CG_FUSED", OPT_CLAMP},
        {"final_sync", &Options::opt_final_sync, 0, 1, OPT_COERCE, "", "BH_FINAL_SYNC", OPT_COERCE},
        {"host_copy_kernels", &Options::opt_host_copy_kernels, 0, 1, OPT_COERCE, "", "BH_HOST_COPY_KERNELS", OPT_COERCE},
        {"ls_from_cg", &Options::opt_ls_from_cg, 0, 1, OPT_COERCE},
        {"step_from_cg", &Options::opt_step_from_cg, 0, 1, OPT_COERCE},
        {"gram_mfma", &Options::opt_gram_mfma, 0, 2, OPT_STORE},
        {"chol_downdate", &Options::opt_chol_downdate, 0, 1, OPT_COERCE},
        {"cauchy_image", &Options::opt_cauchy_image, 0, 1, OPT_COERCE},
        {"cauchy_gram", &Options::opt_cauchy_gram, 0, 1, OPT_COERCE},
        {"cauchy_gram_eq", &Options::opt_cauchy_gram_eq, 0, 1, OPT_REJECT, "cauchy_gram_eq is 0 or 1"},
        // selects a device path of the product: like every product-path call it needs bh_init (switching it off never fails)
        {"gram_cg_fused", &Options::opt_gram_cg_fused, 0, 1, OPT_REJECT, "gram_cg_fused is 0 or 1", nullptr, OPT_IGNORE, nullptr, true},
        {"cauchy_image_refresh", &Options::opt_cauchy_image_refresh, 0, INT64_MAX, OPT_REJECT, "cauchy_image_refresh is 0 (never) or the number of passes between two re-formations"},
        {"cauchy_fused", &Options::opt_cauchy_fused, 0, 1, OPT_COERCE},
        {"cauchy_block", &Options::opt_cauchy_block, 0, 16, OPT_REJECT, "cauchy_block is 0, 1, 2, 4, 8 or 16 breakpoints per launch", "BH_CAUCHY_BLOCK", OPT_IGNORE, cauchy_block_value_ok},
        {"linv_refine", &Options::opt_linv_refine, 0, 1, OPT_COERCE},
        {"cauchy_gemm", &Options::opt_cauchy_gemm, 0, 1, OPT_COERCE},
        {"cauchy_image_max_ma", &Options::opt_cauchy_image_max_ma, 0, 64, OPT_CLAMP},
        {"image_pool", &Options::opt_image_pool, 0, 8, OPT_REJECT, "image_pool must be 0..8"},
        {"free_image", &Options::opt_free_image, 0, 2, OPT_REJECT, "free_image is 0 (off), 1 (by the policy) or 2 (build at the first eligible call)", "BH_FREE_IMAGE", OPT_CLAMP},
        {"free_image_minor", &Options::opt_free_image_minor, 0, 1, OPT_REJECT, "free_image_minor is 0 or 1"},
        {"free_image_chain", &Options::opt_free_image_chain, 0, 1, OPT_REJECT, "free_image_chain is 0 or 1"},
        {"free_image_eq", &Options::opt_free_image_eq, 0, 1, OPT_REJECT, "free_image_eq is 0 or 1", "BH_FREE_IMAGE_EQ", OPT_COERCE},
        {"gram_ingest", &Options::opt_gram_ingest, 0, 1, OPT_REJECT, "gram_ingest is 0 or 1"},
        {"upload_chunk_mb", &Options::opt_upload_chunk_mb, 1, 4096, OPT_REJECT, "upload_chunk_mb must be 1..4096"},
        {"profile_stride", &Options::opt_ev_stride, 1, INT64_MAX, OPT_REJECT, "profile_stride must be >= 1"},
        {"comm_path", nullptr, 0, 1, OPT_CALLER},   // communicator state
        {"profile", nullptr, 0, 1, OPT_CALLER},     // the flags of bh_init
    }};
}
static_assert(option_table(0).back().key != nullptr, "kOptionCount is larger than the table");

// Stores `value` by the row's rule; false: the option keeps its value (OPT_REJECT, OPT_IGNORE).
inline bool option_store(Options& o, const OptionRow& r, OptionOutside outside, int64_t value) {
    if (!(r.ok ? r.ok(value) : (value >= r.lo && value <= r.hi))) {
        if (outside == OPT_REJECT || outside == OPT_IGNORE) return false;
        if (outside != OPT_STORE) value = outside == OPT_COERCE ? 1 : (value < r.lo ? r.lo : r.hi);
    }
    o.*r.field = value;
    return true;
}

// bh_set_option on the fields.  initialised: bh_init has been called.  *why: bh_last_error_detail of a code below BH_OK.
// kOptionForCaller: nothing was stored, the key is one the caller has to finish itself (OPT_CALLER).
constexpr int32_t kOptionForCaller = 1;
inline int32_t option_set(Options& o, const char* key, int64_t value, bool initialised, std::string* why, int64_t max_blocks_per_cu) {
    if (!key) { *why = "NULL key"; return BH_ERR_INVALID_ARG; }
    for (const OptionRow& r : option_table(max_blocks_per_cu)) {
        if (std::strcmp(key, r.key) != 0) continue;
        if (r.outside == OPT_CALLER) return kOptionForCaller;
        if (r.needs_init && value != 0 && !initialised) { *why = "bh_init has not been called"; return BH_ERR_NOT_INIT; }
        if (!option_store(o, r, r.outside, value)) { *why = r.reject; return BH_ERR_INVALID_ARG; }
        return BH_OK;
    }
    *why = std::string("unknown option ") + key;
    return BH_ERR_INVALID_ARG;
}

// The initial values bh_init takes from the environment: read(name) is the variable's text as atoll takes it, nullptr when it is not set.
template <class Getenv>
void options_from_env(Options& o, Getenv&& read, int64_t max_blocks_per_cu) {
    for (const OptionRow& r : option_table(max_blocks_per_cu)) {
        const char* s = r.env ? read(r.env) : nullptr;
        if (s) option_store(o, r, r.env_outside, std::atoll(s));
    }
}

}  // namespace bh
