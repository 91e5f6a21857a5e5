// bh_cauchy_sort_layout.h — the workspace of the two sorted forms of the Cauchy search (bh_cauchysort.hip.h: form 5, H->csort;
// bh_cauchyrowsort.hip.h: form 6, H->crows), stated once (plain values: the host compiler builds it,
// tests/test_sorted_layout_cpu.py runs it).  The allocation, the memset of the hand-back flag and the launcher of bh_api.hip all
// take their offsets from here.
#pragma once
#include <stdint.h>
#include "bh_cauchy_plan.h"

namespace bh {

// bh_cauchysort.hip.h: CS_MAX_PANELS (a static_assert there ties the two).  A change of the panel count is three edits: this constant,
// CS_MAX_PANELS, and the 8 ld doubles of UL written out in tests/test_sorted_layout_cpu.py.
constexpr int kCauchySortMaxPanels = 4;

// Offsets in doubles from the base (-1: the form has no such region), in the order of the layout.  ld is the padded width (a
// multiple of 16): every offset is even — b and rank are read as 16- and 8-byte vectors.
struct CauchySortLayout {
    int64_t T, b;                // ld doubles each, by index
    int64_t UL;                  // form 5: 2 * kCauchySortMaxPanels * ld doubles, the per-panel parts of U, then of L
    int64_t red;                 // form 6: 2 ld doubles, phi'' then X by segment
    int64_t scan;                // form 5: three arrays of ld + 16 doubles, form 6: one
    int64_t rank, inv;           // ld ints each
    int64_t flag;                // the hand-back flag (first int of 16 doubles)
    int64_t head;                // end of the regions above: all of form 5
    int64_t slab;                // form 6: one slab of 2 ld doubles per workgroup of the row scan
    int64_t total;
};

inline CauchySortLayout cauchy_sort_layout(int64_t ld, CauchyForm form, int grid) {
    const bool gram = form == CAUCHY_GRAM_SORTED;
    CauchySortLayout o{};
    o.T = 0;
    o.b = ld;
    o.UL = gram ? 2 * ld : -1;
    o.red = gram ? -1 : 2 * ld;
    o.scan = 2 * ld + (gram ? 2 * kCauchySortMaxPanels : 2) * ld;
    o.rank = o.scan + (gram ? 3 : 1) * (ld + 16);
    o.inv = o.rank + ld / 2;
    o.flag = o.rank + ld;
    o.head = o.flag + 16;
    o.slab = gram ? -1 : o.head;
    o.total = o.head + (gram ? 0 : (int64_t)grid * 2 * ld);
    return o;
}

}  // namespace bh
