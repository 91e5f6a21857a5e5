// Which form of the Cauchy search bh_cauchy_step runs: the rule alone, as a function of plain values (no HIP type, no library
// state), so that the host compiler can build it into a test program (tests/test_cauchy_plan_cpu.py).  The launchers behind each
// form are in bh_api.hip (cauchy_make_plan, cauchy_launch_pass).
#pragma once
#include <algorithm>
#include <cstdint>

namespace bh {

// The numbers bh_cauchy_info reports.
enum CauchyForm : int {
    CAUCHY_SWEEP = 0,         // one H*d sweep per breakpoint, as the reference does
    CAUCHY_ROWSPACE_BOX = 1,  // row space of J, box constraints (bh_cauchy.hip.h)
    CAUCHY_ROWSPACE_EQ = 2,   // row space of J with linear equalities
    CAUCHY_GRAM = 3,          // Gram-form handle: the whole box-constrained search in one launch (bh_cauchygram.hip.h)
    CAUCHY_GRAM_EQ = 4,       // Gram-form handle with linear equalities (bh_cauchygrameq.hip.h)
    CAUCHY_GRAM_SORTED = 5,   // Gram-form handle, box constraints: one sorted sweep over G (bh_hess_set_cauchy_search, bh_cauchysort.hip.h)
    CAUCHY_ROWS_SORTED = 6,   // implicit handle, box constraints: one sorted sweep over J (bh_hess_set_cauchy_rows, bh_cauchy_rows_plan.h)
};

struct CauchySelectIn {
    bool gram_handle;             // the handle is in the Gram form (BH_HESS_GRAM)
    int mA;                       // linear equalities
    bool comm;                    // a communicator is active (several ranks)
    bool lda_is_ld;               // the lineq image has the handle's leading dimension
    bool multi_panel;             // J is wider than the register-resident kernels hold (n > 16384)
    int last_cauchy_passes;       // passes of the previous search on this bh_proj (-1: none yet)
    int64_t cauchy_image, cauchy_image_max_ma, cauchy_fused, cauchy_gram, cauchy_gram_eq, cauchy_image_refresh;   // the options
    int64_t n;                    // columns of J (the blocked search keeps the whole vector side in registers: n <= 4096)
    int64_t cauchy_block;         // option cauchy_block = K: breakpoints per launch of the one-kernel row-space search (0, 1: one)
    bool gram_sorted;             // the handle's switch bh_hess_set_cauchy_search is at BH_CAUCHY_SORTED (no option: a per-handle mode)
};

struct CauchySelection {
    CauchyForm form;
    bool fused;                   // row space, box: ONE kernel per breakpoint (cauchy_fused_kernel)
    int refresh;                  // effective cauchy_image_refresh: 0, or the interval R clamped to the 20-bit pass counter
    int block;                    // effective cauchy_block: 0, or K >= 2 breakpoints per launch (cauchy_block_kernel<K>)
};

// The vector side of cauchy_block_kernel lives in registers: 8 elements in each of 512 threads.
constexpr int64_t kCauchyBlockMaxN = 4096;

inline CauchySelection cauchy_select(const CauchySelectIn& in) {
    const int mA = in.mA;
    CauchySelection o{CAUCHY_SWEEP, false, 0, 0};
    // Gram-form handle, box constraints, one rank, the handle's switch at BH_CAUCHY_SORTED: init -> ranks -> row sums of G -> scan, the
    // same three launches for every search length (bh_cauchysort.hip.h).  Ahead of "cauchy_gram" and independent of every Cauchy
    // option; any other handle or constraint set takes the path it takes without the switch.
    if (in.gram_sorted && in.gram_handle && mA == 0 && !in.comm) o.form = CAUCHY_GRAM_SORTED;
    // Gram-form handle, box constraints, one rank, option "cauchy_gram": init -> G d -> cauchy_gram_kernel, the whole search in one
    // launch (bh_cauchygram.hip.h).  Any other case takes the path it takes without the option.
    else if (in.cauchy_gram != 0 && in.gram_handle && mA == 0 && !in.comm) o.form = CAUCHY_GRAM;
    // Gram-form handle, 1 <= mA <= 64, one rank, option "cauchy_gram_eq": the linear-equality form in the column space of G
    // (bh_cauchygrameq.hip.h) — a = G D g, B = G D A' from one G v launch and one GEMM over n rows, re-formed every
    // kCauchyGramEqRefresh-th pass; per pass [factor + solves: y] -> [Hd = -a - B y | d = P(-g) | t_fresh] -> [decision from Hd].
    else if (in.cauchy_gram_eq != 0 && in.gram_handle && mA >= 1 && mA <= 64 && !in.comm && in.lda_is_ld) o.form = CAUCHY_GRAM_EQ;
    // Box constraints: the image-space search (bh_cauchy.hip.h) — t_d = J~ d once by the J v kernel, then per breakpoint
    // a rank-one update of t_d, t_s over the rows (one column of J) + the single-workgroup advance kernel; no sweep over J.
    // (several ranks: every rank keeps t_d, t_s for ITS rows; the two sums are all-reduced before the replicated advance kernel)
    // With linear equalities the form costs 1 + mA J v sweeps up front: always used up to cauchy_image_max_ma rows; up to 64 rows when
    // the previous search on this handle took more than 4 (1 + mA) passes (consecutive searches of a solve behave alike).
    else if (in.cauchy_image != 0 && (mA == 0 || mA <= in.cauchy_image_max_ma || (mA <= 64 && in.last_cauchy_passes > 4 * (1 + mA))))
        o.form = mA > 0 ? CAUCHY_ROWSPACE_EQ : CAUCHY_ROWSPACE_BOX;
    const bool image = o.form == CAUCHY_ROWSPACE_BOX || o.form == CAUCHY_ROWSPACE_EQ;
    // ... and there ONE kernel per breakpoint: the decision of pass k-1 in the prologue of the row kernel of pass k (cauchy_fused_kernel)
    o.fused = o.form == CAUCHY_ROWSPACE_BOX && !in.comm && in.cauchy_fused != 0;
    // Option cauchy_image_refresh = R >= 1 (one rank): at every pass index that is a positive multiple of R the images are formed again
    // from J and the device-side state, behind the `done` gate; the other passes are unchanged.  Several ranks: ignored.
    //   one kernel per breakpoint: launch k -> [cauchy_fused_kernel, decide_only: decision k-1] [cauchy_reform_kernel: t_d, t_s, sums];
    //                              a J wider than the register-resident kernels hold (n > 16384) keeps its carried images
    //   two-kernel box form:       [J v of d] [J v of s_c] before cauchy_image_kernel(fresh = 1)
    //   with equalities:           [mask g, J v: a] [B: the GEMM or mA masked sweeps] [J v of s_c] before the row kernel (fresh = 1)
    if (image && !in.comm && !(o.fused && in.multi_panel)) o.refresh = (int)std::min<int64_t>(in.cauchy_image_refresh, 0xfffff);
    // Option cauchy_block = K >= 2: the one-kernel form takes K breakpoints per launch (bh_cauchyblock.hip.h) — box constraints, one
    // rank, no re-formation of the images, the whole vector in the registers of one workgroup.  Any other case: the path of K = 0.
    if (o.form == CAUCHY_ROWSPACE_BOX && o.fused && !in.comm && o.refresh == 0 && in.n <= kCauchyBlockMaxN && in.cauchy_block >= 2)
        o.block = (int)in.cauchy_block;
    return o;
}

// The values option cauchy_block accepts (0 and 1: the one-breakpoint-per-launch path).
inline bool cauchy_block_value_ok(int64_t v) { return v == 0 || v == 1 || v == 2 || v == 4 || v == 8 || v == 16; }

// The blocked search on the launch-ahead schedule (off = 1: unit 0 is launch 0, unit b >= 1 is block launch b).  Block launch 1
// takes decision 0, every later one the K decisions behind it: once `unit_target` units have spoken, this many passes are decided.
inline int cauchy_block_pass_target(int unit_target, int K) { return unit_target <= 0 ? 0 : 1 + (unit_target - 1) * K; }
// The block launch that took the last of `passes` decisions — it wrote the final s_c into buffer (launch mod 3).
inline int cauchy_block_final_launch(int passes, int K) { return 1 + (std::max(passes, 1) - 1 + K - 1) / K; }

}  // namespace bh
