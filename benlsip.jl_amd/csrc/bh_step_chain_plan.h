// What bh_step_accumulate_dev and bh_model_reduction_dev do under options "step_from_cg" and "free_image_chain": the rule alone, as
// a function of plain values (no HIP type, no library state), so that the host compiler can build it into a test program
// (tests/test_free_image_chain_cpu.py).  The launches behind each path are in bh_api.hip.
//
// Two notes describe the bh_minor_iterate_dev that has just produced w: the FULL note (cg.hw holds H*w on all n variables) and the
// COMPACT note (cg.hwc holds its free part in slot order, beside the compact w and the handle's slot -> column map).  gm_note says
// that the library itself wrote g_minor for exactly (H, s, g), and carries two flags:
//   fixed_part_stale   a compact accumulate has updated g_minor on the free variables only; its entries on the fixed variables
//                      are those of an earlier s
//   q_valid            the model value q(s) = g.s + s'Hs / 2 of this chain is carried in a device scalar of the workspace
// model_from_gminor_kernel takes s'Hs = s.(g_minor - g) over ALL variables: it is never selected for a stale g_minor.
#pragma once
#include <cstdint>

namespace bh {

enum StepAccPath : int {
    STEP_ACC_SWEEP = 0,           // s += w, then g_minor = H*s + g by a sweep over J (rewrites all of g_minor: both flags fall)
    STEP_ACC_FULL = 1,            // s += w, g_minor += hw on all n variables (two launches, as ever)
    STEP_ACC_FULL_CARRY = 2,      // ... with q carried by a one-workgroup kernel in front of them
    STEP_ACC_COMPACT = 3,         // s += w, g_minor[map[c]] += hwc[c] on the free variables
    STEP_ACC_COMPACT_CARRY = 4,   // ... with q carried by the same launch
};

struct StepAccIn {
    int64_t step_from_cg, free_image_chain;   // the options
    bool full_note, compact_note;             // which note names this (H, w, g_minor)
    bool gm_note_match;                       // gm_note names this (H, s, g, g_minor)
    bool fixed_part_stale, q_valid;           // its flags (read only when it matches)
};

struct StepAccPlan {
    StepAccPath path;
    bool q_init;                  // STEP_ACC_COMPACT_CARRY: the chain has no q yet — q0 from the still fully valid g_minor first
    bool gm_note_set;             // gm_note names (H, s, g, g_minor) afterwards ...
    bool fixed_part_stale, q_valid;   // ... with these flags
};

inline StepAccPlan step_acc_select(const StepAccIn& in) {
    StepAccPlan o{};
    const bool stale = in.gm_note_match && in.fixed_part_stale;
    const bool q = in.gm_note_match && in.q_valid;
    o.path = STEP_ACC_SWEEP;
    o.gm_note_set = true;                     // (the sweep writes g_minor = H*s + g itself)
    if (in.step_from_cg == 0) return o;
    if (in.compact_note && in.free_image_chain == 1) {
        // q can be carried when the chain has one, or when g_minor is still H*s + g on every variable by the library's own hand
        // (q0 from it).  Otherwise only the free part is kept up: the model value then costs its J v sweep.
        const bool carry = in.gm_note_match && (q || !stale);
        o.path = carry ? STEP_ACC_COMPACT_CARRY : STEP_ACC_COMPACT;
        o.q_init = carry && !q;
        o.fixed_part_stale = true;
        o.q_valid = carry;
        return o;
    }
    if (in.full_note) {
        // (q is carried here too: the fixed part of g_minor is already stale, the sums over all n have terms +-0 x there)
        const bool carry = q && in.free_image_chain == 1;
        o.path = carry ? STEP_ACC_FULL_CARRY : STEP_ACC_FULL;
        o.fixed_part_stale = stale;
        o.q_valid = carry;
        return o;
    }
    return o;
}

enum ModelPath : int {
    MODEL_JV = 0,                 // g.s + |J s|^2 / 2 by a sweep over J
    MODEL_FROM_GMINOR = 1,        // s'Hs = s.(g_minor - g): model_from_gminor_kernel, no sweep
    MODEL_CARRIED = 2,            // the carried q through the mailbox: no launch over J, none over the vectors
};

inline ModelPath model_select(int64_t step_from_cg, bool gm_note_match, bool fixed_part_stale, bool q_valid) {
    if (step_from_cg == 0 || !gm_note_match) return MODEL_JV;
    if (q_valid) return MODEL_CARRIED;
    if (fixed_part_stale) return MODEL_JV;
    return MODEL_FROM_GMINOR;
}

}  // namespace bh
