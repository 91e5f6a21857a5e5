// Which iteration shape a projected_cg call takes (bh_pcg*, bh_minor_iterate*): the rule alone, as a function of plain values (no HIP
// type, no library state), so that the host compiler can build it into a test program (tests/test_pcg_plan_cpu.py).  The geometry and
// the launchers behind each shape are in bh_api.hip (pcg_make_plan, pcg_launch_first, pcg_launch_unit).
#pragma once
#include <cstdint>

namespace bh {

enum PcgShape : int {
    PCG_SEPARATE = 0,     // one H*p launch + the step kernels (three kernels with box constraints, seven with equalities)
    PCG_FUSED = 1,        // two, three or four kernels per iteration: S(1) | U(1) S(2) | U(2) S(3) | ...   (bh_cgfuse.hip.h, bh_gramcg.hip.h)
    PCG_RCCL_BOX = 2,     // box constraints over RCCL, the update in the prologue of the next H*p:  S(1) | R(1) AR(1) S(2) | ...
};

struct PcgSelectIn {
    int64_t mA;                   // linear equalities (0: box constraints)
    bool gram_handle;             // the handle is in the Gram form (BH_HESS_GRAM)
    int64_t cg_fused, gram_cg_fused, linv_refine, fold_init;   // the options
    bool comm, peer_path;         // a communicator is active (several ranks); the peer-buffer transport carries the exchanges
    bool reduced;                 // the reduced mA x mA projection form
    bool tpart, W, M_valid;       // bh_proj holds the partials of A_free r, the explicit inverse of the factor, a valid Gram matrix of A_free
    bool lda_is_ld;               // the lineq image has the handle's leading dimension
    bool rs_cfg_ok;               // a register-resident row-stream geometry exists (n <= 16384)
    bool cgp3_ok;                 // ... and it has the CGP = 3 variant
    bool peer_blocks_fit;         // the update kernel's workgroups fit the flags of the peer buffers (kPeerBlkCap)
    bool iterates;                // max_iter >= 1
    bool g_padded;                // g is readable up to the padded length (workspace copy, or n == ld)
    bool vectors_in_regs;         // (n + 1) / 2 <= 4 * CG_T: the single-workgroup step kernels hold the vectors in registers
    bool hw_wanted;               // the caller wants H*w accumulated (bh_minor_iterate)
    bool atol_f2b_positive;
    bool allow_free_image;        // false: the compact loop handed this call back
    bool hw_free_part_ok;         // the free part of the accumulated H*w is enough: hw is wanted, option free_image_minor is on and
                                  // step_from_cg is off (the only consumer left is the line search's w'Hw, and w is zero where fixed),
                                  // or option free_image_chain is on and step_from_cg is on (bh_step_accumulate_dev takes the free
                                  // part too: bh_step_chain_plan.h)
    int64_t free_image_eq;        // option free_image_eq: the three-kernel equality loop may run on the compact image too
};

struct PcgSelection {
    PcgShape shape;
    // PCG_FUSED only (false elsewhere):
    bool fuse_gen;                // linear equalities in the fused shape
    bool gen_linv;                // ... in three kernels, through the explicit inverse of the factor (else four: triangular solves)
    bool linv_refine;             // ... with the step of iterative refinement
    bool peer_fused;              // the exchange between the ranks sits inside the update kernel
    bool rccl_gen;                // equalities over RCCL: slab reduction, collective, update (one kernel more)
    bool free_image_eligible;     // the call may be considered for the compact image of the free columns
    // PCG_SEPARATE only:
    bool fold_init;               // the first H*p / step launches do the initialisation
    int cg_kernels;               // stats.cg_kernels
};

inline PcgSelection pcg_select(const PcgSelectIn& in) {
    PcgSelection o{};
    const bool box = in.mA == 0;
    // Box constraints, J rows register-resident: TWO kernels per iteration instead of three (bh_cgfuse.hip.h) — the H*p launch forms
    // p on the fly and takes the exit test, one 128-workgroup kernel reduces the slabs and updates w, r, v.
    // (g doubles as the first H*p input, so it must be readable up to the padded length.)
    // General constraints in the reduced projection form with mA <= 64 get the same treatment.
    // cg_fused = 1: THREE kernels instead of seven — H*p (p formed on the fly), reduce/update leaving partials of A_free r, and
    // proj_apply_linv_kernel, whose every workgroup sums those partials and applies the explicit inverse of the factor.
    // cg_fused = 2: FOUR kernels — the triangular solves in a launch of their own, then left_mul_tr.  Both change pHp's rounding like
    // the box form does (cg_fused = 0 keeps dot(p, H*p)).
    // Gram form: the fused shapes are opt-in through an option of their own (gram_cg_fused, independent of cg_fused; a Gram handle is
    // single-rank by construction) and exist in the two- and the three-kernel form only; everything else takes the separate-kernel
    // shape, as every Gram handle does without the option.
    const int64_t cg_fused = !in.gram_handle ? in.cg_fused : (in.gram_cg_fused != 0 && !in.comm) ? 1 : 0;
    const bool fuse_gen = !box && cg_fused >= 1 && in.reduced && in.mA <= 64 && in.tpart && in.lda_is_ld && (!in.gram_handle || in.W);
    const bool gen_linv = fuse_gen && cg_fused == 1 && in.W;
    // Several ranks: the exchange rides inside the update kernel when the peer-buffer transport is the active one; an RCCL
    // all-reduce cannot sit inside a kernel.  Equalities over RCCL: the host enqueues the collective between the slab reduction and
    // the update kernel — four kernels + the collective instead of seven.
    const bool peer_fused = in.comm && in.peer_path && (box || fuse_gen) && in.peer_blocks_fit;
    const bool rccl_gen = in.comm && !in.peer_path && fuse_gen;
    const bool feasible = in.rs_cfg_ok && in.iterates && in.g_padded;
    if ((box || fuse_gen) && cg_fused != 0 && feasible && (!in.comm || peer_fused || rccl_gen)) {
        o.shape = PCG_FUSED;
        o.fuse_gen = fuse_gen; o.gen_linv = gen_linv; o.peer_fused = peer_fused; o.rccl_gen = rccl_gen;
        // (one equality: the "factor" is a scalar, y = t / l^2 has no conditioning to repair)
        o.linv_refine = gen_linv && in.linv_refine != 0 && in.M_valid && in.mA >= 2;
        o.cg_kernels = (box ? 2 : gen_linv ? 3 : 4) + (rccl_gen ? 1 : 0);
        // Box constraints, one rank, implicit form, no H*w wanted or only its free part: the loop may run on the compact image of
        // the free columns
        o.free_image_eligible = in.allow_free_image && box && !in.gram_handle && !in.comm && (!in.hw_wanted || in.hw_free_part_ok) &&
                                in.atol_f2b_positive;
        // Linear equalities (option free_image_eq): the three-kernel shape only, whose operands besides A (W, M, the partials of
        // A_free r) depend on the free set alone; A gets the same compaction.  No H*w at all here, whatever hw_free_part_ok says.
        if (in.free_image_eq != 0 && gen_linv && !in.gram_handle && !in.comm && !in.hw_wanted && in.atol_f2b_positive && in.allow_free_image)
            o.free_image_eligible = true;
        return o;
    }
    // Several ranks over RCCL, box constraints: TWO kernels and the collective per iteration — the update of iteration j-1 moves
    // into the prologue of the H*p launch of iteration j (row_stream_kernel<..., CGP = 3>).
    if (!in.gram_handle && in.comm && !in.peer_path && box && in.cg_fused != 0 && feasible && in.cgp3_ok) {
        o.shape = PCG_RCCL_BOX;
        o.cg_kernels = 2;
        return o;
    }
    // Box constraints with register-resident vectors: no init kernel — the first H*p forms p_1 = -mask(g) on the fly and the first
    // step kernel does the initialisation of :702-718 itself.
    o.shape = PCG_SEPARATE;
    o.fold_init = box && in.vectors_in_regs && in.fold_init != 0 && feasible;
    return o;
}

}  // namespace bh
