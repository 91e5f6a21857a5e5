// bh_cauchy_rows_plan.h — where the per-handle switch bh_hess_set_cauchy_rows changes the form of the Cauchy search (plain values:
// the host compiler builds it, tests/test_rowsort_plan_cpu.py runs it).  Applied by cauchy_make_plan AFTER cauchy_select, whose
// input and rule are untouched.  A second switch, bh_hess_set_cauchy_rows_ranks (the field `ranks`, tests/test_rowsort_ranks_plan_cpu.py),
// lets a row-sharded handle take the form as well.
#pragma once
#include <stdint.h>
#include "bh_cauchy_plan.h"

namespace bh {

// The widest row the one geometry of cauchy_rowsort_rows_kernel holds without spilling (bh_cauchyrowsort.hip.h: 512 threads x
// 8 ranks, the whole row of the image in LDS once per row).  ld is the padded width of the handle (n rounded up to 16).
constexpr int64_t kCauchyRowsMaxN = 4096;

inline bool cauchy_rows_served(int64_t n, int64_t ld) { return n >= 1 && ld <= kCauchyRowsMaxN; }

struct CauchyRowsIn {
    bool rows_sorted;             // the handle's switch bh_hess_set_cauchy_rows is at BH_CAUCHY_ROWS_SORTED (and this is no re-run)
    bool gram_handle;
    int mA;
    bool comm;
    int64_t n, ld;
    bool ranks;                   // the handle's switch bh_hess_set_cauchy_rows_ranks is on: a communicator does not rule the form out
};

// Implicit handle, box constraints, a served width, the switch on, and either one rank or the ranks switch on: form 6 — the same
// launches for every search length, ahead of and independent of every Cauchy option (cauchy_image, cauchy_fused, cauchy_block,
// cauchy_image_refresh: the selection loses its fused / refresh / block parts).  Every other case keeps what cauchy_select chose.
// With a communicator the form sums phi'' and X over the ranks in ONE all-reduce (bh_api.hip: cauchy_launch_rows_sorted); every
// input of the rule is replicated, so all ranks choose alike.
inline CauchySelection cauchy_rows_apply(const CauchyRowsIn& in, CauchySelection sel) {
    if (in.rows_sorted && !in.gram_handle && in.mA == 0 && (!in.comm || in.ranks) && cauchy_rows_served(in.n, in.ld))
        return CauchySelection{CAUCHY_ROWS_SORTED, false, 0, 0};
    return sel;
}

}  // namespace bh
