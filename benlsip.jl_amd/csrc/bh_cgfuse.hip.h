// bh_cgfuse.hip.h — second kernel of the two-kernel box-constrained CG iteration
// Part of the single translation unit of bh_api.hip (see bh_kernels.hip.h for the layout and design notes).
//
// One iteration of projected_cg (src/basic_tralcnlss.jl:722-750) used to be three launches: H*p stream, slab reduction,
// single-workgroup step kernel.  For box constraints (projection = mask) it is two:
//   row_stream_kernel<..., CGP = 1>(j)   forms p_j = -v + beta p_{j-1} on the fly (beta and the exit test |r.v| < tol_cg come
//                                         from the partial sums the update kernel of iteration j-1 left), streams J once,
//                                         leaves the per-workgroup slabs of J'(W.(J p)), the partial sums of p'Hp = sum_i
//                                         w_i (Jp)_i^2 and the factor_to_boundary terms of p_j;
//   cg_reduce_update_kernel(j)            128 workgroups: each recomputes the iteration's scalars (pHp, gamma, r.v, alpha and the
//                                         branch of :725-739 — identical bits everywhere: shape-independent wave reductions),
//                                         sums ITS 32 columns of the slabs and updates ITS 32 entries of w, H*w, r, v at once,
//                                         leaving its partial of the next r.v.
// No workgroup ever reads a word its own launch writes: scalars that change are either recomputed from partials or read
// from CgState fields that only the PREVIOUS launch wrote; the exit is signalled through CgState::stop_at (iteration
// number), which gates launches of later iterations only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bh_reduce.hip.h"
#include "bh_cg.hip.h"
#include "bh_comm.hip.h"

namespace bh {

struct CgUpdArgs {
    CgState* st;
    int j;                          // iteration (1-based) = number of the H*p product being consumed
    const double* partials; int64_t ld; int nchunks; int G;      // slabs of the preceding row_stream launch
    int Gs, Gq;                     // how many slabs / p'Hp partials to sum: G, or 1 when an all-reduced H*p with its p'Hp slot takes their place (RCCL)
    const double* sqpart;           // [Gq]
    const double* gpart;            // [G]
    const double* rvpart_in;        // [nrv] partials of r.v from iteration j-1   (j >= 2)
    double* rvpart_out;             // [gridDim.x]
    int nrv;
    const double* p;                // p_j
    double* w; double* hw;          // hw may be NULL
    double* r; const double* g;     // j == 1: r = g_minor (:705), w = 0 (:702)
    double* v;
    const int* fixrank;             // NULL: nothing fixed
    int n;
    double atol_neg;
    double* trace; int trace_cap;
    unsigned long long* mirror; unsigned tag;
    // GEN (linear equalities, reduced projection form): no v / r.v here — this kernel leaves the per-workgroup partials of
    // A_free r, trsv_small_kernel sums and solves, proj_left_mul_tr_kernel forms v = P(r) and the partials of r.v
    const double* A; int64_t ldA; int mA;
    double* tpart;                  // [gridDim.x][mA]
    int init_in_memory;             // j == 1: r = g and w = 0 are already in memory (init kernels), not taken from g
    // Loop on the compact image of the free columns (bh_freeimg.hip.h): every vector above is compact; w also reaches the caller's
    // buffer through the slot -> column map, from the same thread that updates it (NULL: the vectors are the caller's own)
    const int* map; double* w_full;
    const unsigned long long* reroute; unsigned long long reroute_seq;      // as CgFuse::reroute
};

// grid = ceil(nchunks / 16) workgroups of 256 threads = 16 chunks x 16 slab lanes (as reduce_partials_kernel).
// PEER: several ranks over the peer-buffer transport (bh_comm.hip.h) — the workgroup's 32 columns of this rank's slab sum and
// this rank's share of pHp are pushed into every inbox, and the sums over ranks (rank order: identical bits everywhere) take
// their place before the update.  The exchange is inside the stop_at gate by construction.
// The body is in bh_cgfuse_body.hip.h, shared as TEXT with cg_reduce_update_compact_kernel below: the four instantiations of this
// template then compile from exactly the statements they always had (an inlined __device__ body changed their SGPR counts).
// SCAT: w also goes through a.map into a.w_full (the loop on the compact image); the box kernels take the map as a run-time
// argument.
template <bool GEN, bool PEER>
__global__ __launch_bounds__(256) void cg_reduce_update_kernel(CgUpdArgs a, PeerArgs pa) {
    constexpr bool SCAT = !GEN;
#include "bh_cgfuse_body.hip.h"
}

// The three-kernel equality iteration on the compact image of the free columns (option "free_image_eq"): the GEN kernel of one
// rank on compact operands — A is its compact image Af with row stride ldA = ldf, fixrank is NULL (every live slot is free; the
// slots beyond the live width hold zeros in Af and in every vector) — and w reaches the caller's buffer through the map, as in the
// box loop.  In bounds: chunk c < nchunks = round_up(nfree, 16) / 2 <= ldf / 2, row min(., mA - 1) of the mA x ldf image.
__global__ __launch_bounds__(256) void cg_reduce_update_compact_kernel(CgUpdArgs a) {
    constexpr bool GEN = true, PEER = false, SCAT = true;
    const PeerArgs pa{};
#include "bh_cgfuse_body.hip.h"
}

}  // namespace bh
