// What bh_step_accumulate_dev and bh_model_reduction_dev do under options "step_from_cg" and "free_image_chain": the rule alone, as
// a function of plain values (no HIP type, no library state), so that the host compiler can build it into a test program
// (tests/test_free_image_chain_cpu.py).  The launches behind each path are in bh_api.hip.  The notes themselves, with every event
// that sets, uses up or clears one, are StepNotes at the end of this file (tests/test_step_notes_cpu.py).
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

// The three notes and everything that keeps them true.  The host code (bh_api.hip) says WHAT HAPPENED through one of the events
// below, at the place where it happens; which note falls with it is decided here and nowhere else.  Pointers are identities: they
// are compared and never dereferenced.  A note whose H is null is empty.
struct ModelQuery {
    bool match;                       // gm names this (H, s, g) with a g_minor
    bool fixed_part_stale, q_valid;   // its flags, as model_select takes them
    const void* gm;                   // the noted g_minor
};

struct StepNotes {
    struct Full { const void *H = nullptr, *w = nullptr, *gm = nullptr; } full;   // cg.hw is H*w of the call that delivered w for g_minor = gm
    // cg.hwc, the compact w (cg.s) and the handle's slot -> column map (nfree slots) describe that call
    struct Compact { const void *H = nullptr, *w = nullptr, *gm = nullptr; int64_t nfree = 0; } compact;
    // the library itself wrote g_minor = H*s + g for exactly these vectors (flags: the head of this file)
    struct Gm { const void *H = nullptr, *s = nullptr, *g = nullptr, *gm = nullptr; bool fixed_part_stale = false, q_valid = false; } gm;

    // ---- events that invalidate
    // cg.hw, cg.hwc and cg.scalars (the carried q) go with the workspace slab; g_minor is the caller's vector and stays noted.
    // (bh_shutdown used to leave the full note standing: unobservable, a match needs cg.hw != nullptr and the next workspace starts
    // from n_pad = 0, which comes through here.)
    void workspace_gone() { full = {}; compact = {}; gm.q_valid = false; }
    // H is another operator now (mu, form) or no operator at all (destroyed): cg.hw, cg.hwc, the carried q and the caller's g_minor
    // all hold products with the old one.  A null H names nothing.
    void handle_changed(const void* H) {
        if (H == nullptr) return;
        if (full.H == H) full = {};
        if (compact.H == H) compact = {};
        if (gm.H == H) gm = {};
    }
    // the compact image of H was released, built again or had columns moved: cg.hwc and the compact w are in the old slot order
    void compact_slots_changed(const void* H) { if (compact.H == H) compact = {}; }
    // a CG loop starts: it overwrites cg.hw when it accumulates H*w, and any loop may run on the compact image, whose gather
    // rewrites cg.hwc's companions (the compact operands)
    void cg_loop_begins(bool writes_hw) { if (writes_hw) full = {}; compact = {}; }
    // a host-pointer entry point stages its vectors into the workspace vectors that hold the compact operands beside cg.hwc
    void compact_operands_overwritten() { compact = {}; }

    // ---- events that record
    // bh_minor_iterate* has delivered w_out: cg.hw (hw_kept, loop on the full image) or, in the chain, cg.hwc (loop on the compact
    // image) is H*w, scaled with w by the line search.  A host-pointer call (dev false) notes nothing.
    void minor_iterate_done(const void* H, const void* w, const void* g_model, bool dev, bool hw_kept, bool on_compact, bool chain, int64_t nfree) {
        if (dev && hw_kept && !on_compact) { full.H = H; full.w = w; full.gm = g_model; }
        if (dev && hw_kept && on_compact && chain) compact = {H, w, g_model, nfree};
    }
    // a sweep has written all of g_minor = H*s + g: both flags fall.  Into a host vector (dev false) nothing is noted.
    void gminor_written(const void* H, const void* s, const void* g, const void* g_minor, bool dev) {
        gm = {};
        if (dev) gm = {H, s, g, g_minor};
    }
    // bh_step_accumulate_dev looks the notes up and uses up the full and the compact one: s changes next, a second call with the
    // same w is a different step.  hw_live, compact_live, nfree_now: cg.hw exists; cg.hwc, the image and its map exist; the image's
    // width now.  The caller adds the two options to the result.
    StepAccIn accumulate_begins(const void* H, const void* w, const void* gm_out, const void* s, const void* g, bool ok, bool hw_live,
                                bool compact_live, int64_t nfree_now) {
        StepAccIn in{};
        in.full_note = ok && full.H == H && full.w == w && full.gm == gm_out && hw_live;
        in.compact_note = ok && compact.H == H && compact.w == w && compact.gm == gm_out && compact_live && nfree_now == compact.nfree;
        in.gm_note_match = ok && gm.H == H && gm.s == s && gm.g == g && gm.gm == gm_out;
        in.fixed_part_stale = gm.fixed_part_stale; in.q_valid = gm.q_valid;
        full = {}; compact = {};
        return in;
    }
    // the vector launches of a path other than STEP_ACC_SWEEP (that one ends in gminor_written) have updated g_minor for s + w
    void accumulate_done(const void* H, const void* s, const void* g, const void* g_minor, const StepAccPlan& plan) {
        gm = {H, s, g, g_minor, plan.fixed_part_stale, plan.q_valid};
    }
    // bh_model_reduction_dev: read only
    ModelQuery model_query(const void* H, const void* s, const void* g) const {
        return {gm.H == H && gm.s == s && gm.g == g && gm.gm != nullptr, gm.fixed_part_stale, gm.q_valid, gm.gm};
    }
};

}  // namespace bh
