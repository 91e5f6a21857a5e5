// bh_api.hip — C ABI (include/benlsip_hip.h) over the gfx950 kernels of bh_kernels.hip.h.
// One process drives one GPU; all launches go to one stream; exports that move host data are synchronous, device-pointer
// exports return once the host has what it is owed (option final_sync).
#include "../../include/benlsip_hip.h"
#include "bh_cauchy_plan.h"
#include "bh_cauchy_rows_plan.h"
#include "bh_cauchy_sort_layout.h"
#include "bh_free_image_plan.h"
#include "bh_gram_ingest_plan.h"
#include "bh_kernels.hip.h"
#include "bh_launch_ahead.h"
#include "bh_options.h"
#include "bh_pcg_plan.h"
#include "bh_gram_read_plan.h"
#include "bh_step_chain_plan.h"

#include <dlfcn.h>
#include <fcntl.h>
#include <rccl/rccl.h>   // types only: librccl is dlopen'ed in bh_comm_init (never needed on one GPU)
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <initializer_list>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

using namespace bh;

// Every kernel launch of the library goes through hipLaunchKernelGGL in this translation unit: count them (bh_cauchy_info reports
// how many a search enqueued).
static uint64_t g_kernel_launches = 0;
// bh_proj::mask_epoch: bumped wherever fixrank of any handle is written (bh_proj_create, bh_proj_set_active,
// bh_proj_update_active_dev, bh_cauchy_step and the renumbering behind the last two), so equal epochs name the same active set
static uint64_t g_mask_epoch = 0;
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, ...) do { ++g_kernel_launches; hipLaunchKernelGGLInternal((kernelName), __VA_ARGS__); } while (0)

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
namespace {

struct CgWorkspace {
    int64_t n_pad = 0;
    double *w = nullptr, *r = nullptr, *v = nullptr, *p = nullptr, *Hp = nullptr, *g = nullptr, *wl = nullptr, *wu = nullptr;
    double *x = nullptr, *s = nullptr, *xlow = nullptr, *xupp = nullptr;   // minor_iterate staging
    double* hw = nullptr;          // H*w accumulated by the CG loop for minor_iterate's linesearch
    double* hwc = nullptr;         // ... its free part in slot order, when that loop ran on the compact image (options free_image_minor, free_image_chain)
    double *p2 = nullptr, *gpart = nullptr, *rvpart = nullptr;   // two-kernel box iteration: p ping-pong, (spare), r.v partials (2 x n_pad/2)
    double *r2 = nullptr, *hpx = nullptr, *hpx_tail = nullptr;   // RCCL form of it: r ping-pong; H*p with the p'Hp slot right behind it (hpx[n_pad] = hpx_tail[0])
    double* slab = nullptr;
    double* scalars = nullptr;     // 8 doubles (linesearch alpha, ...)
    CgState* d_state = nullptr;
    volatile unsigned long long* h_mirror = nullptr;   // host-mapped progress word written by the CG kernels
    unsigned long long* d_mirror = nullptr;            // its device address
    unsigned tag = 0;
    unsigned long long* d_reroute = nullptr;           // the CG loop on the compact image of the free columns: "run this call on the full image" (bh_freeimg.hip.h)
    unsigned long long reroute_seq = 0;                // one value per such call: the word never needs a reset
    double* d_trace = nullptr;
    int64_t trace_cap = 0;
};

// Host side of the peer-buffer exchange: this rank's inbox, the peers' inboxes mapped through hipIpc, and the POSIX
// shared-memory page the ranks of one node meet on to swap handles (named after the communicator's unique id).
struct PeerShm {
    std::atomic<int> arrive;
    std::atomic<int> generation;
    int failed;
    hipIpcMemHandle_t handle[kMaxPeers];
};
struct PeerComm {
    bool active = false;
    bool broken = false;                     // an exchange timed out: the path may not be selected again
    void* inbox = nullptr;                   // slots | flags | seq, arrive   (one allocation: one IPC handle)
    size_t inbox_bytes = 0;
    void* peer_base[kMaxPeers] = {};         // mapped inboxes (own rank: inbox)
    volatile unsigned long long* h_err = nullptr;   // host-mapped error word
    PeerShm* shm = nullptr;
    PeerArgs args{};
};
constexpr int64_t kPeerCap = 1 << 16;                                   // doubles per slot (512 KiB): larger vectors go in pieces
constexpr int kPeerBlkCap = (int)(kPeerCap / (2 * kPeerBlockChunks));   // 2048 flags per (parity, rank)
constexpr size_t kPeerSlotBytes = (size_t)2 * kMaxPeers * kPeerCap * sizeof(double);
constexpr size_t kPeerFlagBytes = (size_t)2 * kMaxPeers * kPeerBlkCap * sizeof(unsigned long long);
constexpr size_t kPeerScalBytes = kPeerFlagBytes;                         // one double per (parity, rank, block): scalars that ride along

// An upload in flight (bh_hess_create_async): a worker thread feeds column chunks of the caller's J through two device
// staging buffers — copy of chunk k+1 on one stream while chunk k is transposed into the row-major image on another.
struct AsyncUpload {
    std::thread worker;
    int32_t rc = BH_OK;              // written by the worker, read after join
    std::string detail;
    hipStream_t s_copy = nullptr, s_xpose = nullptr;
    double* staging[2] = {nullptr, nullptr};
    hipEvent_t copied[2] = {nullptr, nullptr}, freed[2] = {nullptr, nullptr};
    size_t staging_bytes = 0;        // capacity of each staging buffer
    int64_t chunk_cols = 0;
    // option gram_ingest: G is built behind the transposes, on a stream of its own (bh_gram_ingest_plan.h)
    bool gram = false;               // this upload builds G of its handle
    double gram_mu = 0.0;            // ... with this mu (the handle's at creation)
    GramIngestPlan gram_plan{};
    hipStream_t s_gram = nullptr;
    double* gram_part = nullptr;     // per-slab partial blocks of one step (kept with the other resources)
    int64_t gram_part_doubles = 0;
    bool resources() const { return s_copy != nullptr; }
};

struct Ctx : Options {   // the opt_* fields of bh_set_option: bh_options.h
    bool init = false;
    int device = -1;
    int flags = 0;
    int n_cu = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string detail;
    // what cg.hw, cg.hwc and the caller's g_minor currently are products of, for the options ls_from_cg, step_from_cg and free_image_chain:
    // written and read only through the events of bh_step_chain_plan.h
    StepNotes notes;
    // RCCL
    void* rccl_lib = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    ncclResult_t (*p_ncclGetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*p_ncclCommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*p_ncclCommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*p_ncclAllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*p_ncclGetErrorString)(ncclResult_t) = nullptr;
    // one-shot all-reduce over peer-mapped inboxes (bh_comm.hip.h); comm_path selects it (1) or RCCL (0) when both exist
    PeerComm peer;
    int comm_path = 0;
    CgWorkspace cg;
    double* scratch_dev = nullptr;   // small device scratch (selftest, f2b)
    // Jacobian images of destroyed handles, kept for the next bh_hess_create* of a similar size: the reference builds a new
    // AlHessian for every accepted step (src/basic_tralcnlss.jl:361-362) and drops the old one — a 2 GiB hipFree makes the
    // driver scrub the memory in the background (-5 % HBM bandwidth for ~60 ms) and the next hipMalloc costs ~4 ms
    struct PooledImage { double* ptr; int64_t doubles; };
    std::vector<PooledImage> image_pool;
    int64_t image_pool_hits = 0;
    AsyncUpload* upload_cache = nullptr;   // streams, events and staging buffers of the last finished asynchronous upload, kept for the next
    // host <-> device traffic issued by the library since bh_init (bh_stats: the device-resident entry points are checked against it)
    int64_t h2d_bytes = 0, d2h_bytes = 0, h2d_calls = 0, d2h_calls = 0;
    // Mailbox: a host-mapped page the kernels write the few host-visible results of a device-pointer call into (counts, norms,
    // alpha, the BitVector image), sealed by a sequence number: the host polls one word instead of paying for a DMA per
    // scalar (~10 us each) and a hipStreamSynchronize (~10 us) per call.
    volatile unsigned long long* mbox_h = nullptr;   // [0] = sequence number, payload from byte 64
    unsigned long long* mbox_d = nullptr;
    unsigned long long mbox_seq = 0;
    double* rbuf = nullptr;          // residual staging of bh_resid_sqnorm (grown on demand)
    int64_t rbuf_cap = 0;
    int live_hess = 0;               // bh_hess handles alive (a handle bakes in this rank's share of C: see bh_comm_init)
    // dynamic-LDS ceilings already raised on this device (hipFuncSetAttribute); reset by bh_shutdown
    bool reform_vlds_attr_set = false;   // cauchy_reform_kernel<512,16,1,VL>
    bool vlds_attr_set = false;      // row_stream_kernel<512,16,1,FUSED,...,VL>
    bool cgp_vlds_attr_set = false;  // ... and its two CG-prologue symbols
    bool gramsym_vlds_attr_set = false;  // gram_symv_kernel<512,8,2,0,VL>
    bool trsm_lds_granted = false;   // chol_trsm_kernel
    size_t trsv_lds_granted = 0;     // trsv_pair_kernel
};

Ctx g_ctx;

void pin_arena_abandon(bool drained);   // drops results parked for a call that is about to fail
bool pin_arena_busy();

// drain: DMAs queued by stage_vec / fetch_vec may still be reading or writing the pinned arena; wait for them before the
// arena is handed to the next call.  A caller that is failing BECAUSE the stream makes no progress passes drain = false
// (the arena is then retired instead of reused).
int32_t fail(int32_t code, const std::string& what, bool drain = true) {
    g_ctx.detail = what;
    // the runtime keeps the last error until somebody reads it: a failed hipMalloc (out of memory) would otherwise surface
    // again in the next call's hipGetLastError() check and fail a perfectly good launch
    (void)hipGetLastError();
    bool drained = true;
    if (pin_arena_busy()) drained = drain && g_ctx.stream != nullptr && hipStreamSynchronize(g_ctx.stream) == hipSuccess;
    pin_arena_abandon(drained);
    return code;
}

#define BH_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess)                                                                         \
            return fail(BH_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__));               \
    } while (0)

#define BH_NCCL(call)                                                                                  \
    do {                                                                                               \
        ncclResult_t r__ = (call);                                                                     \
        if (r__ != ncclSuccess)                                                                        \
            return fail(BH_ERR_RCCL, std::string(#call) + ": " +                                      \
                                         (g_ctx.p_ncclGetErrorString ? g_ctx.p_ncclGetErrorString(r__) : "?")); \
    } while (0)

#define BH_REQUIRE_INIT() \
    do { if (!g_ctx.init) return fail(BH_ERR_NOT_INIT, "bh_init has not been called"); } while (0)

#define BH_TRY(expr) do { int32_t rc__ = (expr); if (rc__ != BH_OK) return rc__; } while (0)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline void count_h2d(size_t bytes) { g_ctx.h2d_bytes += (int64_t)bytes; g_ctx.h2d_calls += 1; }
inline void count_d2h(size_t bytes) { g_ctx.d2h_bytes += (int64_t)bytes; g_ctx.d2h_calls += 1; }

template <class T>
int32_t dev_alloc(T** out, int64_t count) {
    *out = nullptr;
    if (count <= 0) count = 1;
    BH_HIP(hipMalloc(reinterpret_cast<void**>(out), (size_t)count * sizeof(T)));
    return BH_OK;
}

void dev_free(void* p) { if (p) (void)hipFree(p); }

// ------------------------------------------------------------------------------------------
// row-stream kernel geometry
// ------------------------------------------------------------------------------------------
struct RsConfig { int T, CPT, R, blocks_per_cu; };

// One geometry as a type: T threads, CPT 16-byte chunks of the vector per thread, R rows per step; blocks_per_cu is its default grid.
template <int T_, int CPT_, int R_, int BPC_>
struct RsGeom {
    static constexpr int T = T_, CPT = CPT_, R = R_, blocks_per_cu = BPC_;
    static constexpr size_t vec_bytes = (size_t)T_ * CPT_ * sizeof(double2);   // one workgroup's slice of a vector
    // n <= 16384 (the last geometry): a kernel that needs a second vector slice next to the row buffers parks it in LDS (VL = 1:
    // T * CPT * 16 bytes = 128 KiB, above the 64 KiB a kernel may use without asking); the others keep everything in registers
    static constexpr bool vec_in_lds = vec_bytes > 64 * 1024;
};

// index -> geometry.  The only place the triples are written: kRsConfigs and every launcher (with_rs_geom) take them from here.
using RsGeoms = std::tuple<
    RsGeom<64, 1, 8, 8>,     // 0: nchunks <= 64    (n <= 128)
    RsGeom<256, 1, 8, 4>,    // 1: nchunks <= 256   (n <= 512)
    RsGeom<256, 2, 8, 2>,    // 2: nchunks <= 512   (n <= 1024)   2 WGs/CU measured best (6.5 vs 6.0 TB/s at 4)
    RsGeom<256, 4, 4, 2>,    // 3: nchunks <= 1024  (n <= 2048)   2 WGs/CU measured best (6.6 vs 6.0 TB/s at 4)
    RsGeom<256, 8, 4, 1>,    // 4: nchunks <= 2048  (n <= 4096)   measured best of nine geometries: 1 WG/CU, 128 KiB in flight
    RsGeom<512, 8, 2, 1>,    // 5: nchunks <= 4096  (n <= 8192)
    RsGeom<512, 16, 1, 1>    // 6: nchunks <= 8192  (n <= 16384): one row per step; the fused mode parks v in LDS (VL)
    >;
constexpr int kNumRsConfigs = (int)std::tuple_size<RsGeoms>::value;
static_assert(kNumRsConfigs == 7, "with_rs_geom and pick_config enumerate seven geometries");

template <class... G>
constexpr std::array<RsConfig, sizeof...(G)> rs_config_table(std::tuple<G...>) { return {{RsConfig{G::T, G::CPT, G::R, G::blocks_per_cu}...}}; }
constexpr auto kRsConfigs = rs_config_table(RsGeoms{});
constexpr int64_t kMaxChunks = 8192;
constexpr int64_t kMaxBlocksPerCu = 8;   // partial-slab capacity per handle: n_cu * kMaxBlocksPerCu workgroups (alloc_hess_common)

int pick_config(int nchunks) {
    if (nchunks <= 64) return 0;
    if (nchunks <= 256) return 1;
    if (nchunks <= 512) return 2;
    if (nchunks <= 1024) return 3;
    if (nchunks <= 2048) return 4;
    if (nchunks <= 4096) return 5;
    return 6;
}

// The only switch over a geometry index: f(RsGeom<...>{}) for the geometry of `cfg`.  f is instantiated for all seven; what exists
// for some of them only sits behind `if constexpr` in f.
template <class F>
void with_rs_geom(int cfg, F&& f) {
    switch (cfg) {
        case 0: f(std::tuple_element_t<0, RsGeoms>{}); break;
        case 1: f(std::tuple_element_t<1, RsGeoms>{}); break;
        case 2: f(std::tuple_element_t<2, RsGeoms>{}); break;
        case 3: f(std::tuple_element_t<3, RsGeoms>{}); break;
        case 4: f(std::tuple_element_t<4, RsGeoms>{}); break;
        case 5: f(std::tuple_element_t<5, RsGeoms>{}); break;
        default: f(std::tuple_element_t<6, RsGeoms>{}); break;
    }
}

// Raise the dynamic-LDS ceiling of the kernels that park a vector slice in LDS, once per device (`granted`: a flag of Ctx).
void grant_lds_once(bool& granted, size_t lds, std::initializer_list<const void*> kernels) {
    if (granted) return;
    for (const void* k : kernels) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    granted = true;
}

template <class G>
void launch_rs_mode(int mode, const RowStreamArgs& a, int grid, hipStream_t s) {
    constexpr int T = G::T, CPT = G::CPT, R = G::R;
    switch (mode) {
        case MODE_JV: hipLaunchKernelGGL((row_stream_kernel<T, CPT, R, MODE_JV>), dim3(grid), dim3(T), 0, s, a); break;
        case MODE_JTV: hipLaunchKernelGGL((row_stream_kernel<T, CPT, R, MODE_JTV>), dim3(grid), dim3(T), 0, s, a); break;
        default: hipLaunchKernelGGL((row_stream_kernel<T, CPT, R, MODE_FUSED>), dim3(grid), dim3(T), 0, s, a); break;
    }
}

// J v and J'u keep everything in registers in every geometry; the fused mode of a vec_in_lds geometry needs the v slice in LDS.
void launch_row_stream(int cfg, int mode, const RowStreamArgs& a, int grid, hipStream_t s) {
    with_rs_geom(cfg, [&](auto geom) {
        using G = decltype(geom);
        if constexpr (G::vec_in_lds) {
            if (mode == MODE_FUSED) {
                auto* kernel = &row_stream_kernel<G::T, G::CPT, G::R, MODE_FUSED, 1, 1, 1>;
                grant_lds_once(g_ctx.vlds_attr_set, G::vec_bytes, {reinterpret_cast<const void*>(kernel)});
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(G::T), G::vec_bytes, s, a);
                return;
            }
        }
        launch_rs_mode<G>(mode, a, grid, s);
    });
}

// CGP = 3: the RCCL form (update of the previous iteration folded into the prologue); register-resident geometries only.
bool cgp3_supported(int cfg) {
    bool ok = false;
    with_rs_geom(cfg, [&](auto geom) { ok = !decltype(geom)::vec_in_lds; });
    return ok;
}
void launch_row_stream_cgp3(int cfg, const RowStreamArgs& a, int grid, hipStream_t s) {
    with_rs_geom(cfg, [&](auto geom) {
        using G = decltype(geom);
        if constexpr (!G::vec_in_lds)
            hipLaunchKernelGGL((row_stream_kernel<G::T, G::CPT, G::R, MODE_FUSED, 1, 1, 0, 3>), dim3(grid), dim3(G::T), 0, s, a);
    });
}

// MODE_FUSED with the CG prologue (two-kernel box iteration).  CGP = 2: the launch expected to stop.
void launch_row_stream_cgp(int cfg, const RowStreamArgs& a, int grid, hipStream_t s, bool expect_stop) {
    with_rs_geom(cfg, [&](auto geom) {
        using G = decltype(geom);
        constexpr int VL = G::vec_in_lds ? 1 : 0;
        constexpr size_t lds = VL ? G::vec_bytes : 0;
        auto* go_on = &row_stream_kernel<G::T, G::CPT, G::R, MODE_FUSED, 1, 1, VL, 1>;
        auto* stop = &row_stream_kernel<G::T, G::CPT, G::R, MODE_FUSED, 1, 1, VL, 2>;
        if constexpr (VL != 0)
            grant_lds_once(g_ctx.cgp_vlds_attr_set, lds, {reinterpret_cast<const void*>(go_on), reinterpret_cast<const void*>(stop)});
        if (expect_stop) hipLaunchKernelGGL(stop, dim3(grid), dim3(G::T), lds, s, a);
        else hipLaunchKernelGGL(go_on, dim3(grid), dim3(G::T), lds, s, a);
    });
}

// Option cauchy_image_refresh, one-kernel-per-breakpoint form: t_d = J~ d, t_s = J~ s_c and their sums in one sweep (cauchy_reform_kernel),
// every geometry.  n <= 8192: both vector slices in registers; above, the slice of d in LDS (128 KiB, asked for once).
void launch_cauchy_reform(int cfg, const CauchyReformArgs& a, int grid, hipStream_t s) {
    with_rs_geom(cfg, [&](auto geom) {
        using G = decltype(geom);
        constexpr int VL = G::vec_in_lds ? 1 : 0;
        constexpr size_t lds = VL ? G::vec_bytes : 0;
        auto* kernel = &cauchy_reform_kernel<G::T, G::CPT, G::R, VL>;
        if constexpr (VL != 0) grant_lds_once(g_ctx.reform_vlds_attr_set, lds, {reinterpret_cast<const void*>(kernel)});
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(G::T), lds, s, a);
    });
}

// Gram form, option gram_cg_fused: G·v with the CG prologue (bh_gramcg.hip.h), every geometry over the ld rows of G.
// Every instantiation holds its slice of p and both row buffers in registers (no z accumulators: nothing is parked in LDS).
void launch_gram_cg(int cfg, const RowStreamArgs& a, int grid, hipStream_t s, bool expect_stop) {
    with_rs_geom(cfg, [&](auto geom) {
        using G = decltype(geom);
        if (expect_stop) hipLaunchKernelGGL((gram_cg_kernel<G::T, G::CPT, G::R, 1>), dim3(grid), dim3(G::T), 0, s, a);
        else hipLaunchKernelGGL((gram_cg_kernel<G::T, G::CPT, G::R, 0>), dim3(grid), dim3(G::T), 0, s, a);
    });
}

// Gram form read through the lower triangle (bh_gramsym.hip.h): the register-resident geometries over the n rows of G, n <= 8192.
// The product keeps its slice of v next to z and both row buffers: in registers up to n = 4096, in LDS (VL, 64 KiB, asked for once)
// for 4096 < n <= 8192, where the registers alone spill; the quadratic form has no z and needs no LDS.
// kGramSymLastGeomOk: whether the widest geometry (8192 < n <= 16384) is served.  Its product kernel spills even with v in LDS
// (profiles/r23_gram_read_resources.txt), so it is not instantiated and such handles keep the full read.
constexpr bool kGramSymLastGeomOk = false;
void launch_gram_symv(int cfg, bool quad, const GramSymArgs& a, int grid, hipStream_t s) {
    with_rs_geom(cfg, [&](auto geom) {
        using G = decltype(geom);
        if constexpr (!G::vec_in_lds || kGramSymLastGeomOk) {
            if (quad) {
                hipLaunchKernelGGL((gram_symv_kernel<G::T, G::CPT, G::R, 1>), dim3(grid), dim3(G::T), 0, s, a);
                return;
            }
            constexpr int VL = G::vec_bytes >= 64 * 1024 ? 1 : 0;
            constexpr size_t lds = VL ? G::vec_bytes : 0;
            auto* kernel = &gram_symv_kernel<G::T, G::CPT, G::R, 0, VL>;
            if constexpr (VL != 0) grant_lds_once(g_ctx.gramsym_vlds_attr_set, lds, {reinterpret_cast<const void*>(kernel)});
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(G::T), lds, s, a);
        }
    });
}

int grid_for(int cfg, int64_t nrows) {
    const RsConfig& c = kRsConfigs[cfg];
    const int64_t ngroups = (nrows + c.R - 1) / c.R;
    const int64_t bpc = g_ctx.opt_blocks_per_cu > 0 ? g_ctx.opt_blocks_per_cu : c.blocks_per_cu;
    int64_t g = (int64_t)g_ctx.n_cu * std::min<int64_t>(bpc, kMaxBlocksPerCu);   // the slab buffers hold n_cu * kMaxBlocksPerCu rows
    g = std::min<int64_t>(g, std::max<int64_t>(ngroups, 1));
    return (int)g;
}

constexpr int kEvCap = 512;
constexpr int kCauchyFusedGrid = 256;    // workgroups of cauchy_fused_kernel (512 rows each per sweep); its partial sums are 2 x [2][256]
constexpr int kCauchyImgGrid = 512;      // workgroups of cauchy_image_kernel (256 rows each per sweep of the row space)

}  // namespace

// ------------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------------
struct bh_hess {
    int64_t d = 0, n = 0, q = 0, q_eff = 0, ld = 0;
    AsyncUpload* up = nullptr;     // non-NULL while bh_hess_create_async's upload may still be running (hess_ready joins it)
    int64_t d_total = 0;           // rows of J over all ranks (= d on one rank): sizes the launch-ahead batch identically everywhere
    int nchunks = 0;
    double mu = 0.0;
    double* Jd = nullptr;          // (d + q) x ld row-major
    int64_t Jd_doubles = 0;        // capacity of the allocation behind Jd (it may come from the image pool)
    double* vpad = nullptr;        // ld
    double* zpad = nullptr;        // ld
    double* upad = nullptr;        // d + q   (J'u input staging / J v output staging)
    double* tbuf = nullptr;        // d + q   (t = J v between the two passes of a column-panel H*p; NULL for n <= 16384)
    double* timg = nullptr;        // 2 x (d + q) + 2 x kCauchyImgGrid: t_d = J~ d, t_s = J~ s_c and the partial sums of the image-space Cauchy search (lazy)
    double* timg_gen = nullptr;    // (1 + mA) x (d + q): a = J~ D g and B = J~ D A' of its linear-equality form (lazy, grown on demand)
    int64_t timg_gen_doubles = 0;
    double* cblk = nullptr;        // option cauchy_block: third s_c buffer (ld), two CauchyBlockRec, 2 x [16][2][kCauchyFusedGrid] partial sums (lazy)
    double* partials = nullptr;    // g_cap x ld
    double* sq_partials = nullptr; // 2 x g_cap (second half: per-workgroup minima of the two-kernel CG iteration)
    double* scalar = nullptr;      // 2
    int g_cap = 0;
    int last_n_hmul = 0;           // H*p count of the previous bh_pcg on this handle (launch schedule hint)
    // tie log of the previous projected_cg on this handle (bh_pcg_tie_info)
    int tie_flags = 0, tie_first = 0, margin_kind = 0, margin_at = 0;
    double min_margin = 0.0;
    unsigned tie_tag = 0;          // tag of the call the log belongs to
    bool tie_read = true;          // false: the words have not been fetched from the host-mapped page yet
    bh_stats_t stats{};
    std::vector<hipEvent_t> ev;    // 2*kEvCap, created lazily
    std::vector<int> ev_pending;   // launch index (within the running bh_pcg) of each recorded pair
    uint64_t hmul_seq = 0;         // H*p launches of bh_pcg calls on this handle (profile sampling)
    bool counted = false;          // included in g_ctx.live_hess (false while a create is failing)
    bool pending_finish = false;   // bh_hess_create_async on a rank without rows: the d_total collective runs at wait / first use, as on its peers
    // explicit Gram form (bh_hess_set_form): G = J'J + mu C'C as an ld x ld row-major image, built on first use after it went stale
    int form = BH_HESS_IMPLICIT;
    double* G = nullptr;           // ld x ld (allocated while form == BH_HESS_GRAM)
    double* gpart = nullptr;       // gram_slabs x ld x ld: per-slab partial sums of a build split over row slabs (small n only)
    int gram_slabs = 1;
    int64_t gram_slab_rows = 0;
    bool G_valid = false;          // G belongs to the current J and to G_mu
    double G_mu = 0.0;             // the mu G was built with
    int64_t gram_builds = 0;
    double* geq = nullptr;         // (1 + mA) x ld: a = G D g and B = G D A' of the Cauchy search with equalities from G (lazy, grown on demand)
    int64_t geq_doubles = 0;
    // how the Gram form reads G (bh_hess_set_gram_read, bh_gram_read_plan.h): remembered in either form, never rebuilds G
    int gram_read = GRAM_READ_FULL;
    int64_t products_lower = 0;    // launches of gram_symv_kernel<..., QUAD = 0> since the handle was created
    int64_t quads_from_g = 0;      // launches of gram_symv_kernel<..., QUAD = 1>
    // which box-constrained Cauchy search the Gram form runs (bh_hess_set_cauchy_search): remembered in either form, never rebuilds G
    int cauchy_search = BH_CAUCHY_STEPWISE;
    int64_t searches_sorted = 0;   // searches the sorted form (bh_cauchysort.hip.h) completed; a handed-back call is not one
    double* csort = nullptr;       // T, b, U / L parts, the scan arrays, rank, inv and the hand-back flag of the sorted form (lazy)
    // which box-constrained Cauchy search the implicit form runs (bh_hess_set_cauchy_rows): remembered in either form, rebuilds nothing
    int cauchy_rows = BH_CAUCHY_ROWS_STEPWISE;
    int cauchy_rows_ranks = 0;     // bh_hess_set_cauchy_rows_ranks: that form also with a communicator, phi'' and X summed in one all-reduce
    int64_t searches_rows_sorted = 0;  // searches the sorted rows form (bh_cauchyrowsort.hip.h) completed; a handed-back call is not one
    double* crows = nullptr;       // T, b, phi'' / X, the scan array, rank, inv, the hand-back flag and the slabs of that form (lazy)
    int crows_grid = 0;            // slabs crows holds: the grid of cauchy_rowsort_rows_kernel on this handle
    // compact image of the free columns (option free_image; bh_free_image_plan.h, bh_freeimg.hip.h)
    double* Jf = nullptr;          // (d + q_eff) x fi.ldf row-major, from the image pool
    int64_t Jf_doubles = 0;        // capacity of the allocation behind Jf
    int* fi_map = nullptr;         // ld ints: slot -> original column (-1 beyond the live width)
    int* fi_ops = nullptr;         // ld ints: the moves of one call (free_image_move_kernel)
    std::vector<int32_t> fi_ops_h; // ... as the host planned them (kept until the next call: the upload may still be reading it)
    FreeImageBook fi;              // host record: active set, map, width, credit, counters
    uint64_t fi_epoch = 0;         // bh_proj::mask_epoch of the active set Jf describes (0: none)
    double* Af = nullptr;          // mA x fi.ldf row-major: the lineq matrix through fi_map (option free_image_eq), zero where the map is -1
    int64_t Af_doubles = 0;        // capacity of the allocation behind Af
    uint64_t af_epoch = 0;         // the epoch Af was formed for: it serves iff this is fi_epoch and the caller's mask_epoch (0: none)
    double call_bytes = 0.0;       // bytes of the image the H*p launches of the running bh_pcg stream
    double timed_bytes = 0.0;      // ... summed over the timed_n sampled launches since the last reset or change of form:
    int64_t timed_n = 0;           //     stats.bytes_per_hmul is their mean, the bytes the sampled launches really streamed
};

struct bh_proj {
    int64_t mA = 0, n = 0, ldA = 0;
    double* Ad = nullptr;          // mA x ldA row-major
    int nfix = 0, mpp = 0;
    bool active_set = false;
    int* fixrank = nullptr;        // ldA ints
    int* fixidx = nullptr;         // n ints
    double* L = nullptr;           // mpp x mpp: the caller's augmented factor (reference form)
    int64_t L_cap = 0;
    bool have_L = false;
    double* M = nullptr;           // mA x mA: A_free A_free' (lower triangle), kept for rank-one downdates (bh_cauchy_step)
    double* Lr = nullptr;          // mA x mA + mA: chol(M) and its reciprocal diagonal (reduced form)
    int* info = nullptr;           // device flag of the Cholesky kernels (= counts + 4)
    double* tpart = nullptr;       // (ldA/32 + 1) x mA: per-workgroup partials of A_free r (three- / four-kernel CG iteration)
    double* W = nullptr;           // 2 x 64 x 64: [Linv | Linv'] of the reduced factor, mA <= 64 (tri_inv_small_kernel)
    bool linv_valid = false;       // W belongs to the current Lr
    int last_cauchy_form = -1;     // bh_cauchy_info: form of the previous bh_cauchy_step on this handle (-1: none yet) ...
    int last_cauchy_launches = 0;  // ... and the kernels it enqueued
    int last_cauchy_passes = 0;    // passes of the previous bh_cauchy_step on this handle (decides whether 1 + mA set-up sweeps pay off)
    bool reduced = false;          // form used by bh_project / bh_pcg for the current active set
    bool M_valid = false;          // M = A_free A_free' for the CURRENT active set (false after factor-only downdates)
    std::vector<uint64_t> last_chunks;   // fixvars of the last successful bh_proj_set_active (reduced form: skip identical pushes)
    int* newidx = nullptr;         // n ints: variables fixed by the last bh_proj_update_active_dev, index order
    int* counts = nullptr;         // 8 ints (AU_*)
    unsigned long long* chunks_dev = nullptr;   // ceil(n/64) + 1 words: BitVector image of the device-side mask
    double* tw = nullptr;          // n + 16
    double* rpad = nullptr;        // ldA
    double* vtmp = nullptr;        // ldA
    uint64_t mask_epoch = 0;       // a library-wide counter's value at the last write of fixrank: equal epochs mean the same active set
};

namespace {

int32_t ensure_cg_workspace(int64_t n_pad, int64_t trace_cap) {
    CgWorkspace& c = g_ctx.cg;
    if (c.n_pad < n_pad) {
        // order matters: the host-pointer entry points stage (g, wl, wu), (s, x, xlow, xupp, g) or (x, xlow, xupp, g) with ONE DMA
        double** vecs[] = {&c.w, &c.r, &c.v, &c.p, &c.Hp, &c.s, &c.x, &c.xlow, &c.xupp, &c.g, &c.wl, &c.wu, &c.hw, &c.hwc, &c.p2, &c.gpart, &c.rvpart,
                           &c.r2, &c.hpx, &c.hpx_tail};
        constexpr int NV = 20;
        dev_free(c.slab);
        c.slab = nullptr;
        g_ctx.notes.workspace_gone();
        BH_TRY(dev_alloc(&c.slab, NV * n_pad + 8));
        BH_HIP(hipMemsetAsync(c.slab, 0, (size_t)(NV * n_pad + 8) * sizeof(double), g_ctx.stream));
        for (int i = 0; i < NV; ++i) *vecs[i] = c.slab + (int64_t)i * n_pad;
        c.scalars = c.slab + NV * n_pad;
        c.n_pad = n_pad;
    }
    if (!c.d_state) {
        BH_TRY(dev_alloc(&c.d_state, 1));
        BH_HIP(hipMemsetAsync(c.d_state, 0, sizeof(CgState), g_ctx.stream));
        void* hp = nullptr;
        BH_HIP(hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent));
        memset(hp, 0, 64);
        c.h_mirror = reinterpret_cast<volatile unsigned long long*>(hp);
        void* dp = nullptr;
        BH_HIP(hipHostGetDevicePointer(&dp, hp, 0));
        c.d_mirror = reinterpret_cast<unsigned long long*>(dp);
    }
    if (!c.d_reroute) {
        BH_TRY(dev_alloc(&c.d_reroute, 1));
        BH_HIP(hipMemsetAsync(c.d_reroute, 0, sizeof(unsigned long long), g_ctx.stream));
    }
    if (trace_cap > c.trace_cap) {
        dev_free(c.d_trace);
        c.d_trace = nullptr;
        BH_TRY(dev_alloc(&c.d_trace, 4 * trace_cap));
        c.trace_cap = trace_cap;
    }
    return BH_OK;
}

int32_t check_peer_error();
int32_t hess_ready(bh_hess* H);

// Spin on the host-mapped progress word until this call's tag shows `done` or at least `target` H*p products.
// iter_target > 0: also return once the reference's `iter` has reached it (two-kernel box iteration: the H*p launch of
// iteration j publishes iter = j when its prologue has decided that the loop goes on).
int32_t wait_mirror(CgWorkspace& c, unsigned tag, int target, MirrorWord* out, int iter_target = 0) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long spins = 0;
    auto reached = [&](unsigned long long w, MirrorWord* m) {
        if (((w >> 48) & 0xffffu) != (tag & 0xffffu)) return false;
        m->status = (int)((w >> 44) & 0xf);
        m->done = (int)((w >> 40) & 0xf);
        m->iter = (int)((w >> 20) & 0xfffff);
        m->n_hmul = (int)(w & 0xfffff);
        return m->done != 0 || m->n_hmul >= target || (iter_target > 0 && m->iter >= iter_target);
    };
    while (true) {
        if (reached(*c.h_mirror, out)) return BH_OK;
        __builtin_ia32_pause();
        if ((++spins & 0xffff) == 0) {
            if (g_ctx.peer.active && *g_ctx.peer.h_err != 0ull) return check_peer_error();
            hipError_t q = hipStreamQuery(g_ctx.stream);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(BH_ERR_HIP, std::string("CG loop: ") + hipGetErrorString(q));
            if (q == hipSuccess) {
                // everything enqueued has run: the word is final.  Not reaching the target now is a logic error, not a wait.
                MirrorWord m2{};
                if (!reached(*c.h_mirror, &m2)) return fail(BH_ERR_HIP, "internal: stream drained but the loop state did not reach the launch target");
                continue;
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
                return fail(BH_ERR_HIP, "CG loop: no progress for 120 s", /*drain=*/false);
        }
    }
}

bool comm_active() { return g_ctx.comm != nullptr || g_ctx.peer.active; }
// the peer-buffer exchange is used when it is the only communicator, or when option "comm_path" = 1 selects it
bool use_peer_path() { return g_ctx.peer.active && (g_ctx.comm_path == 1 || g_ctx.comm == nullptr); }

// buf[0, count) <- sum over ranks, in place, on the library stream.  `buf` must be addressable in whole 16-byte chunks
// (every caller passes a padded workspace vector).  state: the device-side gate of a CG / Cauchy loop — honoured by the
// peer-buffer path; an RCCL call cannot be gated from the device, so over-launched iterations still pay for it there.
int32_t allreduce_inplace(double* buf, int64_t count, bh_hess* H, const CgState* state = nullptr) {
    if (!comm_active() || count <= 0) return BH_OK;
    if (use_peer_path()) {
        for (int64_t off = 0; off < count; off += kPeerCap) {
            const int nch = (int)((std::min(kPeerCap, count - off) + 1) / 2);
            hipLaunchKernelGGL(reduce_exchange_kernel, dim3((nch + kPeerBlockChunks - 1) / kPeerBlockChunks), dim3(256), 0, g_ctx.stream,
                               (const double*)nullptr, (int64_t)0, nch, 0, buf + off, state, g_ctx.peer.args);
        }
        BH_HIP(hipGetLastError());
    } else {
        BH_NCCL(g_ctx.p_ncclAllReduce(buf, buf, (size_t)count, ncclDouble, ncclSum, g_ctx.comm, g_ctx.stream));
    }
    if (H) H->stats.n_allreduce += 1;
    return BH_OK;
}

int32_t check_peer_error() {
    if (g_ctx.peer.active && g_ctx.peer.h_err != nullptr && *g_ctx.peer.h_err != 0ull)
        return fail(BH_ERR_RCCL, "peer-buffer all-reduce: a rank did not arrive within the timeout (exchange #" +
                                     std::to_string(*g_ctx.peer.h_err) + "); results are invalid", /*drain=*/false);
    return BH_OK;
}

// z_out (ld doubles) = sum over ranks of the fixed-order sum of the `grid` slab rows a row-stream launch left in
// H->partials.  One launch either way on one rank; with the peer-buffer communicator the exchange is fused into the slab
// reduction (reduce_exchange_kernel), with RCCL it is a separate collective behind reduce_partials_kernel.
int32_t reduce_slabs(bh_hess* H, int grid, double* z_out, const CgState* state) {
    const int nblk = (H->nchunks + kPeerBlockChunks - 1) / kPeerBlockChunks;
    if (use_peer_path() && nblk <= kPeerBlkCap) {
        hipLaunchKernelGGL(reduce_exchange_kernel, dim3(nblk), dim3(256), 0, g_ctx.stream, (const double*)H->partials, H->ld, H->nchunks,
                           grid, z_out, state, g_ctx.peer.args);
        BH_HIP(hipGetLastError());
        H->stats.n_allreduce += 1;
        return BH_OK;
    }
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(nblk), dim3(256), 0, g_ctx.stream, H->partials, H->ld, H->nchunks, grid, z_out, state);
    BH_HIP(hipGetLastError());
    return allreduce_inplace(z_out, H->n, H, state);
}

// Column panels: a row wider than the register-resident kernels can hold (ld/2 > kMaxChunks) is swept in panels of
// kPanelChunks 16-byte chunks, one launch per panel; H*p then costs two passes over J (J v accumulated over panels into
// tbuf, then J' (W .* t) per panel) instead of the fused single pass.
constexpr int kPanelChunks = 2048;
constexpr int kPanelCfg = 4;          // <256,8,4>: handles any panel up to 2048 chunks, same grid for every panel

bool multi_panel(const bh_hess* H) { return H->nchunks > kMaxChunks; }

RowStreamArgs rs_args(bh_hess* H, int64_t nrows, const CgState* state) {
    RowStreamArgs a{};
    a.J = H->Jd; a.ld = H->ld; a.nrows = nrows; a.d_rows = H->d; a.nchunks = H->nchunks;
    a.mu = H->mu; a.state = state;
    return a;
}

// t (nrows) = J[:, all panels] v
int32_t launch_jv_panels(bh_hess* H, const double* v_pad, double* t, int64_t nrows, const CgState* state) {
    const int grid = grid_for(kPanelCfg, nrows);
    for (int c0 = 0, p = 0; c0 < H->nchunks; c0 += kPanelChunks, ++p) {
        RowStreamArgs a = rs_args(H, nrows, state);
        a.J = H->Jd + 2 * (int64_t)c0; a.v = v_pad + 2 * (int64_t)c0;
        a.nchunks = std::min(kPanelChunks, H->nchunks - c0);
        a.t_out = t; a.accumulate = p > 0 ? 1 : 0;
        launch_row_stream(kPanelCfg, MODE_JV, a, grid, g_ctx.stream);
    }
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// z_out (ld) = J[:, all panels]' (u or W.*u), reduced over workgroups
int32_t launch_jtv_panels(bh_hess* H, const double* u, double* z_out, int64_t nrows, bool weighted, const CgState* state) {
    const int grid = grid_for(kPanelCfg, nrows);
    for (int c0 = 0; c0 < H->nchunks; c0 += kPanelChunks) {
        RowStreamArgs a = rs_args(H, nrows, state);
        a.J = H->Jd + 2 * (int64_t)c0; a.partials = H->partials + 2 * (int64_t)c0;
        a.nchunks = std::min(kPanelChunks, H->nchunks - c0);
        a.u = u; a.weighted_u = weighted ? 1 : 0;
        launch_row_stream(kPanelCfg, MODE_JTV, a, grid, g_ctx.stream);
    }
    BH_HIP(hipGetLastError());
    return reduce_slabs(H, grid, z_out, state);       // includes the all-reduce over ranks
}

// BH_FLAG_PROFILE: records the start event of an H*p launch when this launch is sampled; *slot >= 0 then names the pair.
int32_t profile_begin(bh_hess* H, int ev_index, int* slot) {
    *slot = -1;
    if (!(g_ctx.flags & BH_FLAG_PROFILE) || ev_index < 0) return BH_OK;
    if ((H->hmul_seq++ % (uint64_t)g_ctx.opt_ev_stride) != 0 || (int)H->ev_pending.size() >= kEvCap) return BH_OK;
    if (H->ev.empty()) {
        H->ev.resize(2 * kEvCap, nullptr);
        for (auto& e : H->ev) BH_HIP(hipEventCreate(&e));
    }
    *slot = (int)H->ev_pending.size();
    H->ev_pending.push_back(ev_index);
    BH_HIP(hipEventRecord(H->ev[2 * *slot], g_ctx.stream));
    return BH_OK;
}

// Which path a call of kind `call` (GramReadCall) takes on this handle now (bh_gram_read_plan.h).
bool gram_served(const bh_hess* H) { return gram_read_served(H->nchunks, kMaxChunks, kGramSymLastGeomOk); }
GramReadPath gram_path(const bh_hess* H, int call) {
    GramReadIn in{};
    in.mode = H->gram_read; in.gram_form = H->form == BH_HESS_GRAM; in.served = gram_served(H); in.call = call;
    return gram_read_path(in);
}

// Algorithmic bytes of one H*p launch in the handle's current form (bh_stats_t.bytes_per_hmul).
double hmul_bytes(const bh_hess* H) {
    if (gram_path(H, GRAM_CALL_PRODUCT) == GRAM_PATH_LOWER) return gram_read_lower_bytes(H->n) + 16.0 * (double)H->n;
    if (H->form == BH_HESS_GRAM) return 8.0 * (double)H->n * (double)H->ld + 16.0 * (double)H->n;
    return (multi_panel(H) ? 16.0 : 8.0) * (double)(H->d + H->q_eff) * (double)H->n + 16.0 * (double)H->n;
}

// ---- explicit Gram form --------------------------------------------------------------------------------------------------
// Row slabs of a build: one when the 64 x 64 lower blocks of G already outnumber the CUs, else enough slabs for ~2 workgroups
// per CU, each of at least 256 rows.
void gram_geometry(const bh_hess* H, int* nslabs, int64_t* slab_rows) {
    const int64_t nrows = H->d + H->q_eff;
    const int64_t nb = (H->ld + GNG_BS - 1) / GNG_BS, nlb = nb * (nb + 1) / 2;
    int64_t s = 1;
    if (nlb < g_ctx.n_cu) s = std::max<int64_t>(1, std::min<int64_t>((2 * g_ctx.n_cu + nlb - 1) / nlb, (nrows + 255) / 256));
    int64_t rows = round_up(std::max<int64_t>((nrows + s - 1) / s, 1), 16);
    s = std::max<int64_t>(1, (nrows + rows - 1) / rows);
    *nslabs = (int)s;
    *slab_rows = rows;
}

// G = J'J + mu C'C on the library stream (after the image is complete).  No host synchronisation.
int32_t launch_gram_build(bh_hess* H) {
    BH_TRY(hess_ready(H));
    const int64_t nb = (H->ld + GNG_BS - 1) / GNG_BS;
    const unsigned nlb = (unsigned)(nb * (nb + 1) / 2);
    const int64_t nrows = H->d + H->q_eff;
    const bool split = H->gram_slabs > 1;
    hipLaunchKernelGGL(gn_gram_mfma_kernel, dim3(nlb, (unsigned)H->gram_slabs), dim3(GNG_T), 0, g_ctx.stream, (const double*)H->Jd, H->ld,
                       nrows, H->d, H->mu, H->gram_slab_rows, H->G, split ? H->gpart : nullptr);
    if (split) {
        const int64_t blocks = std::min<int64_t>((H->ld * H->ld + 255) / 256, (int64_t)g_ctx.n_cu * 8);
        hipLaunchKernelGGL(gn_gram_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, g_ctx.stream, (const double*)H->gpart, H->gram_slabs,
                           H->ld, H->G);
    }
    BH_HIP(hipGetLastError());
    H->G_valid = true;
    H->G_mu = H->mu;
    H->gram_builds += 1;
    return BH_OK;
}

int32_t ensure_gram(bh_hess* H) {
    if (H->up) BH_TRY(hess_ready(H));        // an upload that builds G itself (option gram_ingest) leaves it valid
    if (H->G_valid) return BH_OK;
    return launch_gram_build(H);
}

// G·v: row_stream_kernel in J·v mode over the G image (ld rows, every weight 1; the padding rows of G are zero, so z_out's
// padding comes out zero).  Its non-temporal loads are faster than plain ones although G is re-read by every product
// (config 3: 21.9 against 22.4 us; n = 8192: 78.3 against 86.5 us; profiles/r04_gn_gram_timing.txt).
void launch_gram_gv(bh_hess* H, const double* v_pad, double* z_out, const CgState* state, bool negate, const int* negmask) {
    RowStreamArgs a{};
    a.J = H->G; a.ld = H->ld; a.nrows = H->ld; a.d_rows = H->ld; a.nchunks = H->nchunks; a.mu = 1.0; a.state = state;
    a.v = v_pad; a.t_out = z_out;
    a.negate = negate ? 1 : 0; a.negmask = negmask;
    const int cfg = pick_config(H->nchunks);
    launch_row_stream(cfg, MODE_JV, a, grid_for(cfg, a.nrows), g_ctx.stream);
}

// G·v from the lower triangle (bh_hess_set_gram_read): gram_symv_kernel leaves one slab per workgroup in H->partials, the slab
// reduction of the row-stream kernels sums them in index order.  A Gram handle lives on one rank: no exchange behind the reduction.
void launch_gram_gv_lower(bh_hess* H, const double* v_pad, double* z_out, const CgState* state, bool negate, const int* negmask) {
    GramSymArgs a{};
    a.G = H->G; a.ld = H->ld; a.nrows = H->n; a.nchunks = H->nchunks; a.v = v_pad; a.partials = H->partials; a.state = state;
    a.negate = negate ? 1 : 0; a.negmask = negmask;
    const int cfg = pick_config(H->nchunks);
    const int grid = grid_for(cfg, a.nrows);
    launch_gram_symv(cfg, false, a, grid, g_ctx.stream);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((H->nchunks + kPeerBlockChunks - 1) / kPeerBlockChunks), dim3(256), 0, g_ctx.stream,
                       H->partials, H->ld, H->nchunks, grid, z_out, state);
    H->products_lower += 1;
}

// v'Gv from the lower triangle -> sq_out_scalar, where launch_jv would have left sum_i w_i (J v)_i^2: one launch over G and the
// index-order fold of the per-workgroup partials.
void launch_gram_quad(bh_hess* H, const double* v_pad, double* sq_out_scalar) {
    GramSymArgs a{};
    a.G = H->G; a.ld = H->ld; a.nrows = H->n; a.nchunks = H->nchunks; a.v = v_pad; a.sq_partials = H->sq_partials;
    const int cfg = pick_config(H->nchunks);
    const int grid = grid_for(cfg, a.nrows);
    launch_gram_symv(cfg, true, a, grid, g_ctx.stream);
    hipLaunchKernelGGL(reduce_scalar_kernel, dim3(1), dim3(256), 0, g_ctx.stream, H->sq_partials, grid, sq_out_scalar);
    H->quads_from_g += 1;
}

// Gram form of launch_hmul: G rebuilt first when stale, then ONE launch — no slab reduction, no all-reduce.
// (BH_GRAM_READ_LOWER on a served width: the lower triangle and the slab reduction, two launches.)
int32_t launch_gram_hmul(bh_hess* H, const double* v_pad, double* z_out, const CgState* state, int ev_index, bool negate,
                         const int* negmask) {
    BH_TRY(ensure_gram(H));
    int slot = -1;
    BH_TRY(profile_begin(H, ev_index, &slot));
    if (gram_path(H, GRAM_CALL_PRODUCT) == GRAM_PATH_LOWER) launch_gram_gv_lower(H, v_pad, z_out, state, negate, negmask);
    else launch_gram_gv(H, v_pad, z_out, state, negate, negmask);
    if (slot >= 0) BH_HIP(hipEventRecord(H->ev[2 * slot + 1], g_ctx.stream));
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// z_out (ld doubles, device) = sum over ranks of J_k'(W .* (J_k v)), v = v_pad (ld doubles, zero padded).
// Gram form: z_out = G v (launch_gram_hmul).
int32_t launch_hmul(bh_hess* H, const double* v_pad, double* z_out, const CgState* state, int ev_index, bool negate = false,
                    const int* negmask = nullptr) {
    BH_TRY(hess_ready(H));
    if (H->form == BH_HESS_GRAM) return launch_gram_hmul(H, v_pad, z_out, state, ev_index, negate, negmask);
    const int64_t nrows = H->d + H->q_eff;
    if (multi_panel(H)) {
        BH_TRY(launch_jv_panels(H, v_pad, H->tbuf, nrows, state));
        BH_TRY(launch_jtv_panels(H, H->tbuf, z_out, nrows, true, state));
        return BH_OK;
    }
    const int cfg = pick_config(H->nchunks);
    const int grid = grid_for(cfg, nrows);
    RowStreamArgs a = rs_args(H, nrows, state);
    a.v = v_pad; a.partials = H->partials;
    a.negate = negate ? 1 : 0; a.negmask = negmask;
    // BH_FLAG_PROFILE: hipEvents around every opt_ev_stride-th (default 8th) H*p launch of this handle, counted ACROSS calls
    // (an event pair costs ~10 us of stream time; timing every launch would slow the loop it measures by 3 %).
    int slot = -1;
    BH_TRY(profile_begin(H, ev_index, &slot));
    launch_row_stream(cfg, MODE_FUSED, a, grid, g_ctx.stream);
    if (slot >= 0) BH_HIP(hipEventRecord(H->ev[2 * slot + 1], g_ctx.stream));
    return reduce_slabs(H, grid, z_out, state);
}

// (state: NULL, or the launches are skipped when state->done — a sweep enqueued behind the end of the loop it belongs to)
int32_t launch_jv(bh_hess* H, const double* v_pad, double* t_out, bool with_c_rows, double* sq_out_scalar, const CgState* state = nullptr) {
    BH_TRY(hess_ready(H));
    const int64_t nrows = H->d + (with_c_rows ? H->q_eff : 0);
    if (multi_panel(H)) {
        double* t = t_out ? t_out : H->tbuf;
        BH_TRY(launch_jv_panels(H, v_pad, t, nrows, state));
        if (sq_out_scalar)
            hipLaunchKernelGGL(weighted_sqsum_kernel, dim3(1), dim3(1024), 0, g_ctx.stream, (const double*)t, nrows, H->d, H->mu, sq_out_scalar);
        BH_HIP(hipGetLastError());
        return BH_OK;
    }
    const int cfg = pick_config(H->nchunks);
    const int grid = grid_for(cfg, nrows);
    RowStreamArgs a = rs_args(H, nrows, state);
    a.v = v_pad; a.t_out = t_out;
    a.sq_partials = sq_out_scalar ? H->sq_partials : nullptr;
    launch_row_stream(cfg, MODE_JV, a, grid, g_ctx.stream);
    if (sq_out_scalar) {
        hipLaunchKernelGGL(reduce_scalar_kernel, dim3(1), dim3(256), 0, g_ctx.stream, H->sq_partials, grid, sq_out_scalar);
    }
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// v'Hv -> H->scalar (vthv): the weighted square sum of a sweep over J (stats.n_jv) or, under BH_GRAM_READ_LOWER_QUAD on a Gram
// handle, v'Gv from one launch over the lower triangle (quads_from_g).  The value is used exactly where the sweep's was.
int32_t launch_quad(bh_hess* H, const double* v_pad) {
    if (gram_path(H, GRAM_CALL_QUAD) == GRAM_PATH_QUAD_FROM_G) {
        BH_TRY(hess_ready(H));
        BH_TRY(ensure_gram(H));
        launch_gram_quad(H, v_pad, H->scalar);
        BH_HIP(hipGetLastError());
        return BH_OK;
    }
    BH_TRY(launch_jv(H, v_pad, nullptr, true, H->scalar));
    BH_TRY(allreduce_inplace(H->scalar, 1, H));
    H->stats.n_jv += 1;
    return BH_OK;
}

int32_t launch_jtv(bh_hess* H, const double* u_dev, double* z_out, bool with_c_rows = false) {
    BH_TRY(hess_ready(H));
    const int64_t nrows = H->d + (with_c_rows ? H->q_eff : 0);
    if (multi_panel(H)) {
        BH_TRY(launch_jtv_panels(H, u_dev, z_out, nrows, false, nullptr));
        return BH_OK;
    }
    const int cfg = pick_config(H->nchunks);
    const int grid = grid_for(cfg, nrows);
    RowStreamArgs a = rs_args(H, nrows, nullptr);
    a.u = u_dev; a.partials = H->partials;
    launch_row_stream(cfg, MODE_JTV, a, grid, g_ctx.stream);
    return reduce_slabs(H, grid, z_out, nullptr);
}

// An image of `need` doubles: from the pool when a retired one fits (>= the size needed, <= twice), else a fresh allocation.
bool image_from_pool(int64_t need, double** ptr, int64_t* doubles) {
    int best = -1;
    for (int i = 0; i < (int)g_ctx.image_pool.size(); ++i) {
        const int64_t have = g_ctx.image_pool[(size_t)i].doubles;
        if (have >= need && have <= 2 * need && (best < 0 || have < g_ctx.image_pool[(size_t)best].doubles)) best = i;
    }
    if (best >= 0) {
        *ptr = g_ctx.image_pool[(size_t)best].ptr;
        *doubles = g_ctx.image_pool[(size_t)best].doubles;
        g_ctx.image_pool.erase(g_ctx.image_pool.begin() + best);
        g_ctx.image_pool_hits += 1;
        return true;
    }
    return false;
}
int32_t image_acquire(int64_t need, double** ptr, int64_t* doubles) {
    if (image_from_pool(need, ptr, doubles)) return BH_OK;
    BH_TRY(dev_alloc(ptr, need));
    *doubles = need;
    return BH_OK;
}
// ... and back (the caller has drained the stream): kept for the next image when the pool has room, >= 1 MiB images only (small
// ones are not worth a pool slot)
void image_release(double* ptr, int64_t doubles) {
    if (ptr && g_ctx.init && (int64_t)g_ctx.image_pool.size() < g_ctx.opt_image_pool && doubles >= (1 << 17)) g_ctx.image_pool.push_back({ptr, doubles});
    else dev_free(ptr);
}

int32_t alloc_hess_common(bh_hess* H) {
    const int64_t rows = H->d + H->q;
    H->ld = round_up(std::max<int64_t>(H->n, 1), 16);
    H->nchunks = (int)(H->ld / 2);
    H->q_eff = (g_ctx.rank == 0) ? H->q : 0;   // C is replicated: only rank 0 contributes C'(mu C v)
    BH_TRY(image_acquire(std::max<int64_t>(rows, 1) * H->ld, &H->Jd, &H->Jd_doubles));
    BH_TRY(dev_alloc(&H->vpad, H->ld));
    BH_TRY(dev_alloc(&H->zpad, H->ld));
    BH_TRY(dev_alloc(&H->upad, std::max<int64_t>(rows, 1)));
    if (multi_panel(H)) BH_TRY(dev_alloc(&H->tbuf, std::max<int64_t>(rows, 1)));
    BH_HIP(hipMemsetAsync(H->vpad, 0, H->ld * sizeof(double), g_ctx.stream));
    BH_HIP(hipMemsetAsync(H->zpad, 0, H->ld * sizeof(double), g_ctx.stream));
    // partial slabs: enough for the largest grid the option blocks_per_cu may ask for
    int64_t gmax = (int64_t)g_ctx.n_cu * kMaxBlocksPerCu;
    H->g_cap = (int)gmax;
    BH_TRY(dev_alloc(&H->partials, gmax * H->ld));
    // [0, gmax): sum w (Jp)^2 per workgroup; [gmax, 2 gmax): its factor_to_boundary minimum; [2 gmax, 3 gmax): the same, ping-pong
    // partner for the RCCL form of the two-kernel iteration (there the H*p launch reads the previous launch's minima itself)
    BH_TRY(dev_alloc(&H->sq_partials, 3 * gmax));
    BH_TRY(dev_alloc(&H->scalar, 2));
    H->stats.bytes_per_hmul = hmul_bytes(H);
    return BH_OK;
}

int32_t finish_hess_create(bh_hess* H);

static void async_upload_destroy(AsyncUpload* u) {
    if (!u) return;
    for (int i = 0; i < 2; ++i) {
        if (u->copied[i]) (void)hipEventDestroy(u->copied[i]);
        if (u->freed[i]) (void)hipEventDestroy(u->freed[i]);
        dev_free(u->staging[i]);
    }
    dev_free(u->gram_part);
    if (u->s_copy) (void)hipStreamDestroy(u->s_copy);
    if (u->s_xpose) (void)hipStreamDestroy(u->s_xpose);
    if (u->s_gram) (void)hipStreamDestroy(u->s_gram);
    delete u;
}
// A finished upload hands its streams / events / staging buffers to the next one (creating them costs ~3 ms, hipFree of the
// staging buffers another ~3 ms: more than a 64 MiB upload itself).
static void async_upload_cleanup(AsyncUpload* u) {
    if (g_ctx.init && g_ctx.upload_cache == nullptr && u->resources() && u->rc == BH_OK) {
        u->detail.clear();
        g_ctx.upload_cache = u;
        return;
    }
    async_upload_destroy(u);
}

// Worker of bh_hess_create_async.  Never touches g_ctx.detail (the caller's thread owns it): errors travel in u.rc / u.detail.
static void async_upload_worker(bh_hess* H, const double* J, int64_t d, int64_t n, int64_t ldJ, int device) {
    AsyncUpload& u = *H->up;
    auto bad = [&](const char* what, hipError_t e) { u.rc = BH_ERR_HIP; u.detail = std::string(what) + ": " + hipGetErrorString(e); };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { bad("hipSetDevice (upload thread)", e); return; }
    const int64_t cc = u.chunk_cols;
    // option gram_ingest: behind the transpose of chunk k, the blocks of G whose columns are all in the image by then
    // (gram_ingest_step), on s_gram — never on s_xpose, where a Gram kernel of several milliseconds ahead of a transpose would hold
    // that transpose's staging slot and with it the copy.  No launch reads a column that has not landed: a recycled image may hold
    // stale data there.
    auto gram_step = [&](int k, hipEvent_t xposed) -> bool {
        const GramIngestStep st = gram_ingest_step(u.gram_plan, k);
        if (st.nblocks == 0) return true;
        if ((e = hipStreamWaitEvent(u.s_gram, xposed, 0)) != hipSuccess) { bad("hipStreamWaitEvent (Gram step)", e); return false; }
        double* part = st.nslabs > 1 ? u.gram_part : nullptr;
        hipLaunchKernelGGL(gn_gram_panel_kernel, dim3((unsigned)st.nblocks, (unsigned)st.nslabs), dim3(GNG_T), 0, u.s_gram,
                           (const double*)H->Jd, H->ld, H->d + H->q_eff, H->d, u.gram_mu, st.slab_rows, (int)st.block_lo, H->G, part);
        if (part != nullptr) {
            const int64_t blocks = std::min<int64_t>(st.nblocks * (GNG_BS * GNG_BS / 256), (int64_t)u.gram_plan.n_cu * 8);
            hipLaunchKernelGGL(gn_gram_panel_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, u.s_gram, (const double*)part,
                               (int)st.nslabs, (int)st.nblocks, (int)st.block_lo, H->ld, H->G);
        }
        if ((e = hipGetLastError()) != hipSuccess) { bad("Gram step launch", e); return false; }
        return true;
    };
    int k = 0;
    for (int64_t c0 = 0; c0 < n; c0 += cc, ++k) {
        const int slot = k & 1;
        const int64_t cols = std::min(cc, n - c0);
        const bool last = c0 + cols >= n;
        // the staging slot is free once the transpose that read it (two chunks ago) has finished
        if (k >= 2 && (e = hipEventSynchronize(u.freed[slot])) != hipSuccess) { bad("hipEventSynchronize", e); break; }
        if (ldJ == d) e = hipMemcpyAsync(u.staging[slot], J + c0 * ldJ, (size_t)d * cols * sizeof(double), hipMemcpyHostToDevice, u.s_copy);
        else e = hipMemcpy2DAsync(u.staging[slot], (size_t)d * sizeof(double), J + c0 * ldJ, (size_t)ldJ * sizeof(double),
                                  (size_t)d * sizeof(double), (size_t)cols, hipMemcpyHostToDevice, u.s_copy);
        if (e != hipSuccess) { bad("hipMemcpyAsync (J chunk)", e); break; }
        if ((e = hipEventRecord(u.copied[slot], u.s_copy)) != hipSuccess) { bad("hipEventRecord", e); break; }
        if ((e = hipStreamWaitEvent(u.s_xpose, u.copied[slot], 0)) != hipSuccess) { bad("hipStreamWaitEvent", e); break; }
        const int64_t wcols = last ? H->ld - c0 : cols;          // the last chunk also writes the zero padding of every row
        dim3 grid((unsigned)((d + 31) / 32), (unsigned)((wcols + 31) / 32));
        hipLaunchKernelGGL(transpose_cm_to_rm_kernel, grid, dim3(256), 0, u.s_xpose, (const double*)u.staging[slot], d, d, cols,
                           H->Jd + c0, H->ld, wcols);
        if ((e = hipGetLastError()) != hipSuccess) { bad("transpose launch", e); break; }
        if ((e = hipEventRecord(u.freed[slot], u.s_xpose)) != hipSuccess) { bad("hipEventRecord", e); break; }
        if (u.gram && !gram_step(k, u.freed[slot])) break;     // freed[slot]: recorded right behind the transpose of this chunk
    }
    // also after an error: nothing of this upload may still be queued when the handle's buffers go
    if ((e = hipStreamSynchronize(u.s_xpose)) != hipSuccess && u.rc == BH_OK) bad("hipStreamSynchronize (upload)", e);
    if (u.gram && (e = hipStreamSynchronize(u.s_gram)) != hipSuccess && u.rc == BH_OK) bad("hipStreamSynchronize (Gram steps)", e);
}

// Every entry point that reads the image calls this first: joins a pending asynchronous upload (bh_hess_wait does the same).
int32_t hess_ready(bh_hess* H) {
    if (H && !H->up && H->pending_finish) { H->pending_finish = false; return finish_hess_create(H); }
    if (!H || !H->up) return BH_OK;
    AsyncUpload* u = H->up;
    if (u->worker.joinable()) u->worker.join();
    const int32_t rc = u->rc;
    const std::string detail = u->detail;
    if (u->gram && rc == BH_OK) {              // option gram_ingest: the worker has built G (its last synchronisation covered the Gram stream)
        H->gram_builds += 1;
        H->G_mu = u->gram_mu;
        H->G_valid = H->mu == u->gram_mu;      // a bh_hess_set_mu during the upload: rebuilt at the next use, as ever
    }
    u->gram = false;
    async_upload_cleanup(u);
    H->up = nullptr;
    if (rc != BH_OK) return fail(rc, "asynchronous J upload: " + detail);
    return finish_hess_create(H);
}

// Last step of every bh_hess constructor.  With a communicator the ranks' row counts are summed once: everything that
// shapes the launch schedule (launch_batch_size) must be computed from data that is identical on all ranks, or ranks would
// enqueue different numbers of iterations — and of collectives (q_eff and the +-1 row of row_shard differ between ranks).
int32_t finish_hess_create(bh_hess* H) {
    H->d_total = H->d;
    if (comm_active()) {
        double v[2] = {(double)H->d, 0.0};
        BH_HIP(hipMemcpyAsync(H->scalar, v, sizeof(v), hipMemcpyHostToDevice, g_ctx.stream));
        BH_TRY(allreduce_inplace(H->scalar, 1, nullptr));
        BH_HIP(hipMemcpyAsync(v, H->scalar, sizeof(double), hipMemcpyDeviceToHost, g_ctx.stream));
        BH_HIP(hipStreamSynchronize(g_ctx.stream));
        BH_TRY(check_peer_error());
        H->d_total = (int64_t)std::llround(v[0]);
    }
    return BH_OK;
}

// Upload a column-major host matrix (rows x cols, leading dimension ldh) into rows [row0, row0+rows) of a
// row-major padded device image with leading dimension ldd.
// The same from a column-major matrix that already lives in HBM (a device-side jac_res): transpose only, no PCIe.
int32_t transpose_from_device(const double* src_dev, int64_t rows, int64_t cols, int64_t lds, double* dst_image, int64_t row0, int64_t ldd) {
    if (rows == 0) return BH_OK;
    dim3 grid((unsigned)((rows + 31) / 32), (unsigned)((ldd + 31) / 32));
    hipLaunchKernelGGL(transpose_cm_to_rm_kernel, grid, dim3(256), 0, g_ctx.stream, src_dev, lds, rows, cols, dst_image + row0 * ldd, ldd, ldd);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

int32_t upload_transposed(const double* host, int64_t rows, int64_t cols, int64_t ldh, double* dst_image, int64_t row0,
                          int64_t ldd) {
    if (rows == 0) return BH_OK;
    double* staging = nullptr;
    BH_TRY(dev_alloc(&staging, rows * std::max<int64_t>(cols, 1)));
    if (cols > 0) {
        count_h2d((size_t)rows * cols * sizeof(double));
        hipError_t e = hipMemcpy2DAsync(staging, (size_t)rows * sizeof(double), host, (size_t)ldh * sizeof(double),
                                        (size_t)rows * sizeof(double), (size_t)cols, hipMemcpyHostToDevice, g_ctx.stream);
        if (e != hipSuccess) { dev_free(staging); return fail(BH_ERR_HIP, std::string("hipMemcpy2DAsync: ") + hipGetErrorString(e)); }
    }
    dim3 grid((unsigned)((rows + 31) / 32), (unsigned)((ldd + 31) / 32));
    hipLaunchKernelGGL(transpose_cm_to_rm_kernel, grid, dim3(256), 0, g_ctx.stream, staging, rows, rows, cols,
                       dst_image + row0 * ldd, ldd, ldd);
    hipError_t e = hipStreamSynchronize(g_ctx.stream);
    dev_free(staging);
    if (e != hipSuccess) return fail(BH_ERR_HIP, std::string("transpose: ") + hipGetErrorString(e));
    return BH_OK;
}

// Host <-> device vector traffic goes through a pinned arena: the caller's arrays are pageable (Julia / NumPy heap), and a
// pageable hipMemcpyAsync costs 20-25 us per 32 KiB vector; memcpy into pinned memory + a truly asynchronous DMA costs ~4.
// The arena is a bump allocator reset by sync_flush(), which every export calls before returning (host pointers are only
// borrowed for the duration of the call); results are copied out of the arena after the stream has drained.
struct PendingOut { double* dst; const double* pin; int64_t n; };
struct PinArena {
    char* base = nullptr;
    char* dev_base = nullptr;      // the same pages as the GPU sees them (pinned host memory is mapped into the device's address space)
    size_t cap = 0, used = 0;
    std::vector<PendingOut> outs;
    bool dma = false;              // a DMA engine transfer has been enqueued since the last flush (then the flush must be a real drain)
};
PinArena g_pin;
inline void note_dma() { g_pin.dma = true; }
// Small host <-> device vector copies done by a KERNEL on the mapped arena instead of a DMA engine: a 32 KiB hipMemcpyAsync costs
// ~10 us of stream time and a kernel behind it another cross-engine dependency; a copy kernel reads / writes the pinned pages
// over PCIe in ~3 us and keeps everything on the compute queue, so that the call can end with a mailbox seal + poll instead
// of a hipStreamSynchronize.
__global__ __launch_bounds__(256) void arena_copy_kernel(double* __restrict__ dst, const double* __restrict__ src, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
}
inline double* pin_dev_view(const double* pin) { return reinterpret_cast<double*>(g_pin.dev_base + (reinterpret_cast<const char*>(pin) - g_pin.base)); }
inline bool arena_kernels() { return g_ctx.opt_host_copy_kernels != 0 && g_pin.dev_base != nullptr; }
inline void launch_arena_copy(double* dst, const double* src, int64_t n) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 256));
    hipLaunchKernelGGL(arena_copy_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, dst, src, n);
}
bool pin_arena_busy() { return g_pin.used > 0; }
void pin_arena_abandon(bool drained) {
    g_pin.outs.clear();
    g_pin.used = 0;
    // transfers may still be in flight (the stream could not be drained): retire this arena — it is leaked on purpose,
    // a later pin_alloc maps a fresh one — rather than let the next call's vectors share memory with a stale DMA
    if (!drained) { g_pin.base = nullptr; g_pin.dev_base = nullptr; g_pin.cap = 0; }
    g_pin.dma = false;
}
constexpr size_t kPinArenaBytes = 32u << 20;
constexpr int64_t kPinMaxVec = 1 << 20;     // doubles; larger transfers go directly (bandwidth-, not latency-bound)

double* pin_alloc(int64_t n) {
    if (n > kPinMaxVec) return nullptr;
    if (!g_pin.base) {
        void* p = nullptr;
        if (hipHostMalloc(&p, kPinArenaBytes, hipHostMallocDefault) != hipSuccess) return nullptr;
        g_pin.base = static_cast<char*>(p);
        g_pin.cap = kPinArenaBytes;
        void* dp = nullptr;
        g_pin.dev_base = (hipHostGetDevicePointer(&dp, p, 0) == hipSuccess) ? static_cast<char*>(dp) : nullptr;
        if (g_pin.dev_base == nullptr) (void)hipGetLastError();
    }
    const size_t bytes = ((size_t)n * sizeof(double) + 255) & ~(size_t)255;
    if (g_pin.used + bytes > g_pin.cap) return nullptr;
    double* r = reinterpret_cast<double*>(g_pin.base + g_pin.used);
    g_pin.used += bytes;
    return r;
}

int32_t stage_vec(double* dst_pad, const double* src, int64_t n, bool src_is_device) {
    if (n == 0) return BH_OK;
    if (!src_is_device) count_h2d((size_t)n * sizeof(double));
    if (!src_is_device) {
        if (double* pin = pin_alloc(n)) {
            memcpy(pin, src, (size_t)n * sizeof(double));
            if (arena_kernels()) { launch_arena_copy(dst_pad, pin_dev_view(pin), n); BH_HIP(hipGetLastError()); return BH_OK; }
            note_dma();
            BH_HIP(hipMemcpyAsync(dst_pad, pin, (size_t)n * sizeof(double), hipMemcpyHostToDevice, g_ctx.stream));
            return BH_OK;
        }
        note_dma();
    }
    BH_HIP(hipMemcpyAsync(dst_pad, src, (size_t)n * sizeof(double), src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                          g_ctx.stream));
    return BH_OK;
}

// A device vector the kernels may read in whole 16-byte chunks up to the padded length: the caller's own buffer when it needs no
// padding (n == n_pad) and is 16-byte aligned, else a zero-padded staging copy (pad must be zero beyond n already).
int32_t device_operand(const double** out, double* pad, const double* v_dev, int64_t n, int64_t n_pad) {
    if (n == n_pad && (reinterpret_cast<uintptr_t>(v_dev) & 15u) == 0) { *out = v_dev; return BH_OK; }
    BH_TRY(stage_vec(pad, v_dev, n, true));
    *out = pad;
    return BH_OK;
}

// Several host vectors into CONSECUTIVE workspace vectors (stride n_pad) with one DMA instead of one each: a 32 KiB
// hipMemcpyAsync costs ~10 us of stream time whatever its size, and the host-pointer entry points stage 3-5 of them.
int32_t stage_vecs(double* dst_first, std::initializer_list<const double*> srcs, int64_t n, int64_t n_pad) {
    const int64_t k = (int64_t)srcs.size();
    double* pin = (n > 0) ? pin_alloc(k * n_pad) : nullptr;
    if (pin == nullptr) {
        int64_t i = 0;
        for (const double* src : srcs) {       // too large for the arena: one copy each; the padding is zeroed as the batched path does
            BH_TRY(stage_vec(dst_first + i * n_pad, src, n, false));
            if (n_pad > n) BH_HIP(hipMemsetAsync(dst_first + i * n_pad + n, 0, (size_t)(n_pad - n) * sizeof(double), g_ctx.stream));
            ++i;
        }
        return BH_OK;
    }
    int64_t i = 0;
    for (const double* src : srcs) {
        memcpy(pin + i * n_pad, src, (size_t)n * sizeof(double));
        if (n_pad > n) memset(pin + i * n_pad + n, 0, (size_t)(n_pad - n) * sizeof(double));
        ++i;
    }
    count_h2d((size_t)k * n * sizeof(double));
    if (arena_kernels()) { launch_arena_copy(dst_first, pin_dev_view(pin), k * n_pad); BH_HIP(hipGetLastError()); return BH_OK; }
    note_dma();
    BH_HIP(hipMemcpyAsync(dst_first, pin, (size_t)(k * n_pad) * sizeof(double), hipMemcpyHostToDevice, g_ctx.stream));
    return BH_OK;
}

int32_t fetch_vec(double* dst, const double* src_dev, int64_t n, bool dst_is_device) {
    if (n == 0) return BH_OK;
    if (!dst_is_device) count_d2h((size_t)n * sizeof(double));
    if (!dst_is_device) {
        if (double* pin = pin_alloc(n)) {
            if (arena_kernels()) { launch_arena_copy(pin_dev_view(pin), src_dev, n); BH_HIP(hipGetLastError()); }
            else { note_dma(); BH_HIP(hipMemcpyAsync(pin, src_dev, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, g_ctx.stream)); }
            g_pin.outs.push_back({dst, pin, n});
            return BH_OK;
        }
        note_dma();
    }
    BH_HIP(hipMemcpyAsync(dst, src_dev, (size_t)n * sizeof(double), dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                          g_ctx.stream));
    return BH_OK;
}

// ---- mailbox ------------------------------------------------------------------------------
constexpr size_t kMboxBytes = 64 * 1024;
constexpr size_t kMboxPayloadOff = 64;
constexpr size_t kMbScal = 0, kMbInts = 16, kMbChunks = 64;          // payload layout: 2 doubles | 8 ints | BitVector image
// Optional riders: up to two doubles and `icount` ints that live in device memory (results an all-reduce or a later kernel
// also needs there) are copied into the page by the sealing thread itself.
__global__ void mbox_seal_kernel(unsigned long long* seq_word, unsigned long long seq, const double* a, const double* b, double* ddst,
                                 const int* isrc, int icount, int* idst) {
    // runs after the producers (same stream): their stores to the page were performed before they completed
    if (a != nullptr) ddst[0] = a[0];
    if (b != nullptr) ddst[1] = b[0];
    for (int i = 0; i < icount; ++i) idst[i] = isrc[i];
    __threadfence_system();
    __hip_atomic_store(seq_word, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
int32_t mbox_ensure() {
    if (g_ctx.mbox_h) return BH_OK;
    void* hp = nullptr;
    BH_HIP(hipHostMalloc(&hp, kMboxBytes, hipHostMallocMapped | hipHostMallocCoherent));
    memset(hp, 0, kMboxBytes);
    void* dp = nullptr;
    BH_HIP(hipHostGetDevicePointer(&dp, hp, 0));
    g_ctx.mbox_h = static_cast<volatile unsigned long long*>(hp);
    g_ctx.mbox_d = static_cast<unsigned long long*>(dp);
    g_ctx.mbox_seq = 0;
    return BH_OK;
}
// device / host views of the payload (byte offset `off`, a multiple of 8)
template <class T> T* mbox_dev(size_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(g_ctx.mbox_d) + kMboxPayloadOff + off); }
template <class T> const volatile T* mbox_host(size_t off) {
    return reinterpret_cast<const volatile T*>(reinterpret_cast<const volatile char*>(g_ctx.mbox_h) + kMboxPayloadOff + off);
}
// Enqueue the seal; returns its sequence number through *seq_out.
int32_t mbox_seal(unsigned long long* seq_out, const double* a = nullptr, const double* b = nullptr, double* ddst = nullptr,
                  const int* isrc = nullptr, int icount = 0, int* idst = nullptr) {
    const unsigned long long seq = ++g_ctx.mbox_seq;
    hipLaunchKernelGGL(mbox_seal_kernel, dim3(1), dim3(1), 0, g_ctx.stream, g_ctx.mbox_d, seq, a, b, ddst, isrc, icount, idst);
    BH_HIP(hipGetLastError());
    *seq_out = seq;
    return BH_OK;
}
// Spin until the seal `seq` has been observed: the stream executes in order, so EVERYTHING enqueued before the seal — kernels,
// DMAs into and out of the pinned arena — has completed by then.
int32_t mbox_poll(unsigned long long seq) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long spins = 0;
    while (g_ctx.mbox_h[0] != seq) {
        __builtin_ia32_pause();
        if ((++spins & 0xffff) == 0) {
            if (g_ctx.peer.active && *g_ctx.peer.h_err != 0ull) return check_peer_error();
            const hipError_t q = hipStreamQuery(g_ctx.stream);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(BH_ERR_HIP, std::string("mailbox wait: ") + hipGetErrorString(q));
            if (q == hipSuccess && g_ctx.mbox_h[0] != seq) return fail(BH_ERR_HIP, "internal: stream drained but the mailbox was not sealed");
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
                return fail(BH_ERR_HIP, "mailbox wait: no progress for 120 s", /*drain=*/false);
        }
    }
    // what the device wrote before the seal (mailbox payload, results parked in the pinned arena) is read after it: keep the
    // compiler from hoisting those plain loads above the poll (the hardware keeps load order on its own)
    std::atomic_thread_fence(std::memory_order_acquire);
    return BH_OK;
}
void pin_arena_deliver() {
    for (const PendingOut& o : g_pin.outs) memcpy(o.dst, o.pin, (size_t)o.n * sizeof(double));
    g_pin.outs.clear();
    g_pin.used = 0;
}

// Wait until everything enqueued has completed, deliver the results parked in the pinned arena, reset the arena:
// hipStreamSynchronize, or a seal in the mailbox + a poll where no DMA precedes it (the device-pointer entry points use that
// through mbox_seal_and_wait).  Behind a D2H DMA the seal kernel waits for a cross-engine dependency that costs more than the
// synchronize it replaces (A/B'd: bh_pcg 0.667 -> 0.72 ms, bh_project 34 -> 45-50 us), so there it stays a synchronize.
int32_t sync_flush() {
    // No DMA engine involved since the last flush (the host vectors travelled through arena_copy_kernel): a seal + poll ends
    // the call without a hipStreamSynchronize.
    const bool kernels_only = arena_kernels() && !g_pin.dma;
    g_pin.dma = false;
    if (!g_ctx.opt_final_sync && kernels_only && g_ctx.mbox_h != nullptr) {
        unsigned long long seq = 0;
        BH_TRY(mbox_seal(&seq));
        BH_TRY(mbox_poll(seq));
        pin_arena_deliver();
        return check_peer_error();
    }
    hipError_t e = hipStreamSynchronize(g_ctx.stream);
    if (e == hipSuccess) pin_arena_deliver();
    g_pin.outs.clear();
    g_pin.used = 0;
    if (e != hipSuccess) return fail(BH_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return check_peer_error();
}

// Seal what the kernels enqueued so far have written into the mailbox (plus the riders) and wait for it.  `bytes`: payload
// size, for the transfer counters.  Results parked in the pinned arena by a host-pointer caller are delivered as well.
int32_t mbox_seal_and_wait(size_t bytes, const double* a = nullptr, const double* b = nullptr, double* ddst = nullptr,
                           const int* isrc = nullptr, int icount = 0, int* idst = nullptr) {
    unsigned long long seq = 0;
    BH_TRY(mbox_seal(&seq, a, b, ddst, isrc, icount, idst));
    count_d2h(bytes);
    if (g_ctx.opt_final_sync) {
        const hipError_t e = hipStreamSynchronize(g_ctx.stream);
        if (e != hipSuccess) return fail(BH_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    } else {
        BH_TRY(mbox_poll(seq));
    }
    pin_arena_deliver();
    return check_peer_error();
}
// End of a device-pointer call whose results stay in HBM: nothing is owed to the host, later calls are ordered behind this
// one on the library stream (option final_sync = 1: drain as the host-pointer entry points do).
int32_t finish_device_call() {
    if (g_ctx.opt_final_sync || pin_arena_busy()) return sync_flush();
    BH_HIP(hipGetLastError());
    return check_peer_error();
}

// ---- projection -------------------------------------------------------------------------
int32_t ensure_reduced_buffers(bh_proj* P) {
    const int64_t mA = P->mA;
    if (!P->M) BH_TRY(dev_alloc(&P->M, mA * mA));
    if (!P->Lr) BH_TRY(dev_alloc(&P->Lr, mA * mA + mA));
    if (!P->info) P->info = P->counts + 4;      // (rides to the host with the AU_* counts: one copy by the mailbox's sealing thread)
    if (!P->tpart) BH_TRY(dev_alloc(&P->tpart, (P->ldA / 32 + 1) * std::max<int64_t>(mA, 1)));
    if (!P->W && mA <= 64) BH_TRY(dev_alloc(&P->W, 2 * 64 * 64));
    return BH_OK;
}

// Lr = chol(M) (lower, column-major mA x mA).  mA <= 64: one launch of the register-panel kernel (+ reciprocal diagonal
// after the matrix for trsv_small_kernel).  Larger: blocked right-looking — per 64-column panel potrf on the diagonal
// block, trsm for the rows below it, syrk for the trailing matrix (3 launches per panel; ~0.3 ms at mA = 256, against 1.6 ms for one right-looking workgroup).
int32_t launch_chol(bh_proj* P, const CgState* gate) {
    const int mA = (int)P->mA;
    hipStream_t s = g_ctx.stream;
    P->linv_valid = false;
    if (mA <= 64) {
        hipLaunchKernelGGL(chol_small_kernel, dim3(1), dim3(256), 0, s, (const double*)P->M, (int64_t)mA, P->Lr, (int64_t)mA, mA,
                           P->Lr + (int64_t)mA * mA, P->info, 0, gate == nullptr ? 1 : 0, gate);
        BH_HIP(hipGetLastError());
        return BH_OK;
    }
    double* dinv = P->Lr + (int64_t)mA * mA;      // scratch for the current panel's reciprocal diagonal (mA extra doubles)
    if (!g_ctx.trsm_lds_granted) {                 // 97 KiB of dynamic LDS: above what a kernel may use without asking
        BH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&chol_trsm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)kTrsmLdsBytes));
        g_ctx.trsm_lds_granted = true;
    }
    hipLaunchKernelGGL(copy_lower_kernel, dim3(std::min(1024, (mA * mA + 255) / 256)), dim3(256), 0, s, (const double*)P->M, P->Lr, mA,
                       P->info, gate);
    for (int k0 = 0; k0 < mA; k0 += 64) {
        const int nb = std::min(64, mA - k0);
        double* blk = P->Lr + k0 + (int64_t)k0 * mA;
        hipLaunchKernelGGL(chol_small_kernel, dim3(1), dim3(256), 0, s, (const double*)blk, (int64_t)mA, blk, (int64_t)mA, nb, dinv, P->info,
                           k0, 0, gate);
        const int rem = mA - k0 - nb;
        if (rem > 0) {
            hipLaunchKernelGGL(chol_trsm_kernel, dim3((rem + TRSM_T - 1) / TRSM_T), dim3(TRSM_T), kTrsmLdsBytes, s, P->Lr, mA, k0, nb,
                               (const double*)dinv, gate);
            const int nt = (rem + 15) / 16;
            hipLaunchKernelGGL(chol_syrk_kernel, dim3(nt, nt), dim3(256), 0, s, P->Lr, mA, k0, nb, gate);
        }
    }
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// M = A_free A_free' from the device-side mask, then Lr = chol(M).  `gate`: skip when gate->done (in-loop use).
int32_t launch_reduced_factor(bh_proj* P, bool use_mask, const CgState* gate) {
    const int mA = (int)P->mA;
    // Measured (n = 4096): VALU kernel 12 us at mA = 64, 107 us at mA = 256; MFMA kernel ~33 us flat up to mA ~ 350 (one
    // workgroup per tile leaves most CUs idle for few tiles) -> matrix cores from mA > 96; opt_gram_mfma = 2 forces them.
    if ((g_ctx.opt_gram_mfma == 1 && mA > 96) || g_ctx.opt_gram_mfma == 2) {
        const int nt = (mA + 15) / 16;            // 16 x 16 lower tiles on the matrix cores (v_mfma_f64_16x16x4_f64)
        hipLaunchKernelGGL(gram_free_mfma_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(GRAM_T), 0, g_ctx.stream, P->Ad, P->ldA, mA,
                           use_mask ? P->fixrank : (const int*)nullptr, P->M);
    } else {
        const int64_t pairs = (int64_t)mA * (mA + 1) / 2;
        hipLaunchKernelGGL(gram_free_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, g_ctx.stream, P->Ad, P->ldA, mA,
                           use_mask ? P->fixrank : (const int*)nullptr, P->M);
    }
    BH_TRY(launch_chol(P, gate));
    P->M_valid = true;
    return BH_OK;
}

ProjArgs proj_args(bh_proj* P, const CgState* st, bool reduced, bool force_mask = false) {
    ProjArgs a{};
    a.A = P->Ad; a.ldA = P->ldA; a.mA = (int)P->mA; a.n = (int)P->n; a.nfix = P->nfix;
    a.fixrank = (P->nfix > 0 || force_mask) ? P->fixrank : nullptr;
    a.fixidx = P->fixidx; a.tw = P->tw; a.state = st;
    a.reduced = reduced ? 1 : 0;
    a.L = reduced ? P->Lr : P->L;
    a.mpp = reduced ? (int)P->mA : (int)P->mA + P->nfix;
    return a;
}

// One pass of the CG loop body: register-resident kernel when the vectors fit (n <= 8192), generic otherwise.
template <int PHASE>
void launch_cg_step(const CgArgs& a, hipStream_t s) {
    const int nch = (a.n + 1) / 2;
    if (nch <= CG_T) hipLaunchKernelGGL((cg_step_reg_kernel<1, PHASE>), dim3(1), dim3(CG_T), 0, s, a);
    else if (nch <= 2 * CG_T) hipLaunchKernelGGL((cg_step_reg_kernel<2, PHASE>), dim3(1), dim3(CG_T), 0, s, a);
    else if (nch <= 4 * CG_T) hipLaunchKernelGGL((cg_step_reg_kernel<4, PHASE>), dim3(1), dim3(CG_T), 0, s, a);
    else hipLaunchKernelGGL((cg_step_kernel<PHASE>), dim3(1), dim3(CG_T), 0, s, a);
}

// First pass of a box-constrained CG with the initialisation folded in (n <= 8192).
void launch_cg_first_step(const CgArgs& a, hipStream_t s) {
    const int nch = (a.n + 1) / 2;
    if (nch <= CG_T) hipLaunchKernelGGL((cg_step_reg_kernel<1, 0, true>), dim3(1), dim3(CG_T), 0, s, a);
    else if (nch <= 2 * CG_T) hipLaunchKernelGGL((cg_step_reg_kernel<2, 0, true>), dim3(1), dim3(CG_T), 0, s, a);
    else hipLaunchKernelGGL((cg_step_reg_kernel<4, 0, true>), dim3(1), dim3(CG_T), 0, s, a);
}

// LDS of trsv_pair_kernel: x[m2] | tile[64*65] | part[4*m2] (only when the split trailing update fits the 160 KiB of a CU)
constexpr size_t kLdsPerCu = 160 * 1024;
int trsv_split_for(int m) {
    const size_t m2 = (size_t)((m + 1) & ~1);
    return (5 * m2 + 64 * 65) * sizeof(double) <= kLdsPerCu ? 4 : 1;
}
// The dynamic-LDS ceiling of the kernel is a property of the function, shared by every handle: only ever raise it.
int32_t ensure_trsv_lds(size_t lds) {
    if (lds <= g_ctx.trsv_lds_granted) return BH_OK;
    BH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&trsv_pair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    g_ctx.trsv_lds_granted = lds;
    return BH_OK;
}
size_t trsv_lds_bytes(int m) {
    const size_t m2 = (size_t)((m + 1) & ~1);
    return ((trsv_split_for(m) == 4 ? 5 : 1) * m2 + 64 * 65) * sizeof(double);
}

// v_out = P(r_pad): r_pad is a zero-padded ldA-length device vector, v_out has >= n entries.
int32_t launch_project(bh_proj* P, const double* r_pad, double* v_out, const CgState* st, bool device_mask = false) {
    // device_mask: the active set lives in P->fixrank on the device and may be ahead of the host's P->nfix (bh_cauchy_step)
    const int n = (int)P->n;
    if (P->mA == 0) {
        const int grid = std::max(1, std::min((n + 255) / 256, 1024));
        hipLaunchKernelGGL(proj_mask_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, r_pad, v_out,
                           (P->nfix > 0 || device_mask) ? P->fixrank : (const int*)nullptr, n, st);
        BH_HIP(hipGetLastError());
        return BH_OK;
    }
    ProjArgs a = proj_args(P, st, device_mask ? true : P->reduced, device_mask);
    const int grid1 = a.mA + (a.reduced ? 0 : (a.nfix + 255) / 256);
    hipLaunchKernelGGL(proj_left_mul_kernel, dim3(grid1), dim3(256), 0, g_ctx.stream, a, r_pad);
    if (a.reduced && a.mpp <= 64) hipLaunchKernelGGL(trsv_small_kernel, dim3(1), dim3(256), 0, g_ctx.stream, a);
    else hipLaunchKernelGGL(trsv_pair_kernel, dim3(1), dim3(CG_T), trsv_lds_bytes(a.mpp), g_ctx.stream, a, trsv_split_for(a.mpp));
    const int nch = (n + 1) / 2;
    if (a.mA <= 64) hipLaunchKernelGGL((proj_left_mul_tr_kernel<true, 4>), dim3((nch + 63) / 64), dim3(256), 0, g_ctx.stream, a, r_pad, v_out);
    else hipLaunchKernelGGL((proj_left_mul_tr_kernel<true, 16>), dim3((nch + 63) / 64), dim3(1024), 0, g_ctx.stream, a, r_pad, v_out);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

int32_t check_proj_ready(bh_proj* P) {
    if (!P) return fail(BH_ERR_INVALID_ARG, "NULL bh_proj");
    if (P->mA > 0 && !P->active_set) return fail(BH_ERR_PRECONDITION, "bh_proj_set_active has not been called (factor missing)");
    return BH_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// exports: library / device
// ------------------------------------------------------------------------------------------
extern "C" {

const char* bh_strerror(int32_t code) {
    switch (code) {
        case BH_OK: return "ok";
        case BH_ERR_INVALID_ARG: return "invalid argument";
        case BH_ERR_NOT_INIT: return "library not initialised (call bh_init)";
        case BH_ERR_HIP: return "HIP runtime error";
        case BH_ERR_RCCL: return "RCCL error";
        case BH_ERR_PRECONDITION: return "precondition of the reference violated";
        case BH_ERR_SHAPE: return "shape mismatch between handles";
        case BH_ERR_NO_DEVICE: return "no usable GPU device";
        case BH_ERR_UNSUPPORTED: return "unsupported configuration";
        default: return "unknown error code";
    }
}

const char* bh_last_error_detail(void) { return g_ctx.detail.c_str(); }

int32_t bh_init(int32_t device, int32_t flags) {
    if (g_ctx.init) {
        if (device != g_ctx.device)
            return fail(BH_ERR_INVALID_ARG, "bh_init: already initialised on another device (bh_shutdown first)");
        g_ctx.flags = flags;
        return BH_OK;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(BH_ERR_NO_DEVICE, "hipGetDeviceCount found no device");
    if (device < 0 || device >= count) return fail(BH_ERR_INVALID_ARG, "device ordinal out of range");
    BH_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    BH_HIP(hipGetDeviceProperties(&prop, device));
    g_ctx.n_cu = prop.multiProcessorCount;
    g_ctx.device = device;
    g_ctx.flags = flags;
    BH_HIP(hipStreamCreateWithFlags(&g_ctx.own_stream, hipStreamNonBlocking));
    g_ctx.stream = g_ctx.own_stream;
    BH_TRY(dev_alloc(&g_ctx.scratch_dev, 1024));
    BH_TRY(mbox_ensure());
    options_from_env(g_ctx, getenv, kMaxBlocksPerCu);
    g_ctx.init = true;
    return BH_OK;
}

static void peer_release(bool with_barrier);

int32_t bh_shutdown(void) {
    if (!g_ctx.init) return BH_OK;
    (void)hipStreamSynchronize(g_ctx.stream);
    if (g_ctx.comm && g_ctx.p_ncclCommDestroy) { g_ctx.p_ncclCommDestroy(g_ctx.comm); g_ctx.comm = nullptr; }
    if (g_ctx.peer.active) peer_release(true);
    g_ctx.comm_path = 0;
    CgWorkspace& c = g_ctx.cg;
    dev_free(c.slab); dev_free(c.d_state); dev_free(c.d_trace); dev_free(c.d_reroute);
    if (c.h_mirror) (void)hipHostFree(const_cast<unsigned long long*>(c.h_mirror));
    c = CgWorkspace();
    g_ctx.notes.workspace_gone();
    dev_free(g_ctx.scratch_dev); g_ctx.scratch_dev = nullptr;
    dev_free(g_ctx.rbuf); g_ctx.rbuf = nullptr; g_ctx.rbuf_cap = 0;
    if (g_ctx.mbox_h) { (void)hipHostFree(const_cast<unsigned long long*>(g_ctx.mbox_h)); g_ctx.mbox_h = nullptr; g_ctx.mbox_d = nullptr; }
    async_upload_destroy(g_ctx.upload_cache); g_ctx.upload_cache = nullptr;
    for (auto& im : g_ctx.image_pool) dev_free(im.ptr);
    g_ctx.image_pool.clear();
    if (g_ctx.own_stream) (void)hipStreamDestroy(g_ctx.own_stream);
    g_ctx.own_stream = nullptr; g_ctx.stream = nullptr;
    if (g_pin.base) { (void)hipHostFree(g_pin.base); g_pin = PinArena(); }
    g_ctx.vlds_attr_set = false; g_ctx.cgp_vlds_attr_set = false; g_ctx.gramsym_vlds_attr_set = false; g_ctx.reform_vlds_attr_set = false; g_ctx.trsm_lds_granted = false; g_ctx.trsv_lds_granted = 0;
    g_ctx.init = false; g_ctx.rank = 0; g_ctx.nranks = 1;
    return BH_OK;
}

int32_t bh_set_stream(void* hip_stream) {
    BH_REQUIRE_INIT();
    BH_TRY(sync_flush());
    g_ctx.stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : g_ctx.own_stream;
    return BH_OK;
}

int32_t bh_synchronize(void) {
    BH_REQUIRE_INIT();
    BH_TRY(sync_flush());
    return BH_OK;
}

int32_t bh_device_info(char* name_out, int64_t name_cap, int32_t* n_cu, char* arch_out, int64_t arch_cap) {
    BH_REQUIRE_INIT();
    hipDeviceProp_t prop;
    BH_HIP(hipGetDeviceProperties(&prop, g_ctx.device));
    if (name_out && name_cap > 0) { strncpy(name_out, prop.name, (size_t)name_cap - 1); name_out[name_cap - 1] = 0; }
    if (arch_out && arch_cap > 0) { strncpy(arch_out, prop.gcnArchName, (size_t)arch_cap - 1); arch_out[arch_cap - 1] = 0; }
    if (n_cu) *n_cu = prop.multiProcessorCount;
    return BH_OK;
}

int32_t bh_set_option(const char* key, int64_t value) {
    std::string why;
    const int32_t rc = option_set(g_ctx, key, value, g_ctx.init, &why, kMaxBlocksPerCu);   // the table of bh_options.h
    if (rc < BH_OK) return fail(rc, why);
    while ((int64_t)g_ctx.image_pool.size() > g_ctx.opt_image_pool) { dev_free(g_ctx.image_pool.back().ptr); g_ctx.image_pool.pop_back(); }   // image_pool
    if (rc != kOptionForCaller) return BH_OK;
    if (!strcmp(key, "comm_path")) {
        if (value == 1 && !g_ctx.peer.active) return fail(BH_ERR_PRECONDITION, "comm_path = 1 needs the peer-buffer communicator (BH_COMM=ipc or both)");
        if (value == 0 && comm_active() && g_ctx.comm == nullptr) return fail(BH_ERR_PRECONDITION, "comm_path = 0 needs an RCCL communicator (BH_COMM=rccl or both)");
        if (value != 0 && value != 1) return fail(BH_ERR_INVALID_ARG, "comm_path is 0 (RCCL) or 1 (peer buffers)");
        if (g_ctx.stream) (void)hipStreamSynchronize(g_ctx.stream);
        // leaving the peer-buffer path after a timed-out exchange: the error word is cleared so that the RCCL path can carry on
        // (re-selecting the peer path after a timeout is refused: the ranks' exchange counters no longer agree)
        if (value == 0 && g_ctx.peer.active && g_ctx.peer.h_err != nullptr && *g_ctx.peer.h_err != 0ull) {
            *g_ctx.peer.h_err = 0ull;
            g_ctx.peer.broken = true;
        }
        if (value == 1 && g_ctx.peer.broken) return fail(BH_ERR_RCCL, "the peer-buffer transport timed out earlier in this communicator's life");
        g_ctx.comm_path = (int)value;
        return BH_OK;
    }
    if (!strcmp(key, "profile")) { g_ctx.flags = value ? (g_ctx.flags | BH_FLAG_PROFILE) : (g_ctx.flags & ~BH_FLAG_PROFILE); return BH_OK; }
    return fail(BH_ERR_INVALID_ARG, std::string("unknown option ") + key);
}

// ---- multi-GPU -----------------------------------------------------------------------------
static int32_t load_rccl() {
    if (g_ctx.rccl_lib) return BH_OK;
    // BH_RCCL_LIB names a specific build.  Otherwise by SONAME: glibc hands back the copy the process has already mapped
    // (e.g. the one libtorch_hip.so brought in), so there is one RCCL per process.
    const char* names[] = {getenv("BH_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* nm : names) {
        if (!nm || !*nm) continue;
        g_ctx.rccl_lib = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
        if (g_ctx.rccl_lib) break;
        if (nm == names[0]) return fail(BH_ERR_RCCL, std::string("dlopen(BH_RCCL_LIB=") + nm + "): " + dlerror());
    }
    if (!g_ctx.rccl_lib) return fail(BH_ERR_RCCL, std::string("dlopen(librccl): ") + dlerror());
#define BH_SYM(field, name)                                                          \
    g_ctx.field = reinterpret_cast<decltype(g_ctx.field)>(dlsym(g_ctx.rccl_lib, name)); \
    if (!g_ctx.field) return fail(BH_ERR_RCCL, std::string("dlsym ") + name)
    BH_SYM(p_ncclGetUniqueId, "ncclGetUniqueId");
    BH_SYM(p_ncclCommInitRank, "ncclCommInitRank");
    BH_SYM(p_ncclCommDestroy, "ncclCommDestroy");
    BH_SYM(p_ncclAllReduce, "ncclAllReduce");
    BH_SYM(p_ncclGetErrorString, "ncclGetErrorString");
#undef BH_SYM
    return BH_OK;
}

// Which communicators bh_comm_init brings up: BH_COMM = "rccl" (default), "ipc" (peer-buffer exchange only: no librccl
// needed) or "both" (RCCL carries the all-reduces until bh_set_option("comm_path", 1) switches to the peer buffers).
enum { COMM_RCCL = 1, COMM_IPC = 2 };
static int comm_mode() {
    const char* m = getenv("BH_COMM");
    if (!m || !*m || !strcmp(m, "rccl")) return COMM_RCCL;
    if (!strcmp(m, "ipc") || !strcmp(m, "peer")) return COMM_IPC;
    if (!strcmp(m, "both")) return COMM_RCCL | COMM_IPC;
    return 0;
}

static bool peer_barrier(PeerShm* shm, int nranks, int timeout_s) {
    const int gen = shm->generation.load(std::memory_order_acquire);
    if (shm->arrive.fetch_add(1, std::memory_order_acq_rel) + 1 == nranks) {
        shm->arrive.store(0, std::memory_order_relaxed);
        shm->generation.store(gen + 1, std::memory_order_release);
        return true;
    }
    const auto t0 = std::chrono::steady_clock::now();
    while (shm->generation.load(std::memory_order_acquire) == gen) {
        sched_yield();
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(timeout_s)) return false;
    }
    return true;
}

static void peer_release(bool with_barrier) {
    PeerComm& pc = g_ctx.peer;
    if (pc.shm && with_barrier) (void)peer_barrier(pc.shm, g_ctx.nranks, 20);   // nobody unmaps while a peer may still push
    for (int p = 0; p < kMaxPeers; ++p)
        if (pc.peer_base[p] && pc.peer_base[p] != pc.inbox) (void)hipIpcCloseMemHandle(pc.peer_base[p]);
    if (pc.inbox) (void)hipFree(pc.inbox);
    if (pc.h_err) (void)hipHostFree(const_cast<unsigned long long*>(pc.h_err));
    if (pc.shm) munmap(pc.shm, sizeof(PeerShm));
    pc = PeerComm();
}

// Bring up the peer-buffer exchange among the `nranks` processes of ONE node: allocate this rank's inbox, publish its
// hipIpc handle on a shared-memory page named after the communicator id, map everybody else's.
static int32_t peer_init(int rank, int nranks, const unsigned char* id) {
    if (nranks > kMaxPeers) return fail(BH_ERR_UNSUPPORTED, "peer-buffer all-reduce supports at most 8 ranks (one node)");
    PeerComm& pc = g_ctx.peer;
    unsigned long long h = 1469598103934665603ull;            // FNV-1a of the id: the rendezvous name
    for (int i = 0; i < BH_UNIQUE_ID_BYTES; ++i) { h ^= id[i]; h *= 1099511628211ull; }
    char name[64];
    snprintf(name, sizeof(name), "/bh_ipc_%016llx", h);
    const int fd = shm_open(name, O_CREAT | O_RDWR, 0600);
    if (fd < 0) return fail(BH_ERR_RCCL, std::string("shm_open(") + name + ") failed");
    if (ftruncate(fd, sizeof(PeerShm)) != 0) { close(fd); return fail(BH_ERR_RCCL, "ftruncate on the rendezvous page failed"); }
    void* m = mmap(nullptr, sizeof(PeerShm), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return fail(BH_ERR_RCCL, "mmap of the rendezvous page failed");
    pc.shm = static_cast<PeerShm*>(m);

    // one allocation = one handle: [slots | flags | scal | seq, arrive, dead].  Fine-grained (uncached) so that a peer's stores and this
    // rank's polls meet in memory, not in somebody's L2.
    pc.inbox_bytes = kPeerSlotBytes + kPeerFlagBytes + kPeerScalBytes + 256;
    hipError_t e = hipExtMallocWithFlags(&pc.inbox, pc.inbox_bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) { (void)hipGetLastError(); e = hipExtMallocWithFlags(&pc.inbox, pc.inbox_bytes, hipDeviceMallocFinegrained); }
    // no coarse-grained fallback: the exchange kernels issue no cache-invalidating acquire and no L2 write-back (their
    // system-scope accesses rely on memory that is not cached in a local L2), so on a plain hipMalloc'ed inbox flag polls and
    // payload loads could be served from a stale line.  The rendezvous fails instead (collectively) and callers use RCCL.
    if (e != hipSuccess) { (void)hipGetLastError(); pc.inbox = nullptr; }
    bool ok = (e == hipSuccess);
    if (ok) ok = hipMemset(pc.inbox, 0, pc.inbox_bytes) == hipSuccess;
    char* base = static_cast<char*>(pc.inbox);
    const unsigned long long one = 1ull;
    if (ok) ok = hipMemcpy(base + kPeerSlotBytes + kPeerFlagBytes + kPeerScalBytes, &one, sizeof(one), hipMemcpyHostToDevice) == hipSuccess;   // seq = 1
    if (ok) ok = hipDeviceSynchronize() == hipSuccess;
    if (ok && nranks > 1) ok = hipIpcGetMemHandle(&pc.shm->handle[rank], pc.inbox) == hipSuccess;
    if (!ok) pc.shm->failed = 1;
    if (!peer_barrier(pc.shm, nranks, 120)) { shm_unlink(name); peer_release(false); return fail(BH_ERR_RCCL, "peer rendezvous: the other ranks did not arrive (same node? same id?)"); }
    for (int p = 0; p < nranks && !pc.shm->failed; ++p) {
        if (p == rank) { pc.peer_base[p] = pc.inbox; continue; }
        if (hipIpcOpenMemHandle(&pc.peer_base[p], pc.shm->handle[p], hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
            (void)hipGetLastError();
            pc.peer_base[p] = nullptr;
            pc.shm->failed = 1;
        }
    }
    const bool met = peer_barrier(pc.shm, nranks, 120);
    if (rank == 0 || !met) shm_unlink(name);   // everybody has mapped the page; nothing is left behind in /dev/shm (also on the failure exits)
    if (!met || pc.shm->failed) { peer_release(false); return fail(BH_ERR_RCCL, "peer rendezvous: hipIpc handle exchange failed on some rank"); }
    // from here on every failure is made COLLECTIVE (flag on the shared page + barrier) so that all ranks leave together
    void* hp = nullptr;
    void* dp = nullptr;
    bool local_ok = hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    if (local_ok) {
        memset(hp, 0, 64);
        pc.h_err = static_cast<volatile unsigned long long*>(hp);
        local_ok = hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess;
    }
    if (!local_ok) { (void)hipGetLastError(); pc.shm->failed = 1; }
    PeerArgs& a = pc.args;
    a = PeerArgs{};
    for (int p = 0; p < nranks; ++p) {
        char* b = static_cast<char*>(pc.peer_base[p]);
        a.slots[p] = reinterpret_cast<double*>(b);
        a.flags[p] = reinterpret_cast<unsigned long long*>(b + kPeerSlotBytes);
        a.scal[p] = reinterpret_cast<double*>(b + kPeerSlotBytes + kPeerFlagBytes);
    }
    a.seq = reinterpret_cast<unsigned long long*>(base + kPeerSlotBytes + kPeerFlagBytes + kPeerScalBytes);
    a.arrive = reinterpret_cast<unsigned*>(base + kPeerSlotBytes + kPeerFlagBytes + kPeerScalBytes + 64);
    a.dead = reinterpret_cast<unsigned*>(base + kPeerSlotBytes + kPeerFlagBytes + kPeerScalBytes + 128);
    a.err = static_cast<unsigned long long*>(dp);
    a.rank = rank; a.nranks = nranks; a.cap = kPeerCap; a.nblk_cap = kPeerBlkCap;
    const char* ts = getenv("BH_PEER_TIMEOUT_S");
    a.timeout_ticks = (unsigned long long)((ts && atof(ts) > 0 ? atof(ts) : 20.0) * 1e8);            // wall_clock64: 100 MHz
    // Reachability echo (a mapping that opens is not yet a mapping stores land in): one real exchange of a known vector
    // through every mapped inbox, with a short timeout, BEFORE anybody relies on the transport — a node where hipIpc maps
    // but peer stores do not arrive is found here, collectively, and callers fall back to RCCL instead of running into the
    // in-kernel timeout inside a timed region.  Rank r contributes (r + 1)(i + 1); the sum is exact in fp64.
    std::string echo_detail;
    const bool met1 = peer_barrier(pc.shm, nranks, 120);          // every rank's `failed` so far is visible behind it
    const char* skip = getenv("BH_PEER_ECHO_SKIP_RANK");          // test hook: this rank stays away from the echo
    if (met1 && !pc.shm->failed && skip && *skip && atoi(skip) == rank) {
        echo_detail = "this rank stayed away from the echo (BH_PEER_ECHO_SKIP_RANK)";
        pc.shm->failed = 1;
    } else if (met1 && !pc.shm->failed) {
        constexpr int kEcho = 2 * kPeerBlockChunks;               // one workgroup's worth
        double hv[kEcho], *dv = nullptr;
        for (int i = 0; i < kEcho; ++i) hv[i] = (double)(rank + 1) * (double)(i + 1);
        bool ok_e = hipMalloc(&dv, sizeof(hv)) == hipSuccess && hipMemcpy(dv, hv, sizeof(hv), hipMemcpyHostToDevice) == hipSuccess;
        if (ok_e) {
            PeerArgs ea = a;
            const char* es = getenv("BH_PEER_ECHO_TIMEOUT_S");
            ea.timeout_ticks = (unsigned long long)((es && atof(es) > 0 ? atof(es) : 5.0) * 1e8);
            hipLaunchKernelGGL(reduce_exchange_kernel, dim3(1), dim3(256), 0, g_ctx.stream, (const double*)nullptr, (int64_t)0, kPeerBlockChunks, 0, dv,
                               (const CgState*)nullptr, ea);
            ok_e = hipGetLastError() == hipSuccess && hipStreamSynchronize(g_ctx.stream) == hipSuccess &&
                   hipMemcpy(hv, dv, sizeof(hv), hipMemcpyDeviceToHost) == hipSuccess;
        }
        if (dv) (void)hipFree(dv);
        if (!ok_e) { (void)hipGetLastError(); echo_detail = "the echo exchange could not run"; }
        else if (*pc.h_err != 0ull) echo_detail = "the echo exchange timed out waiting for a peer's flag";
        else
            for (int i = 0; i < kEcho && echo_detail.empty(); ++i)
                if (hv[i] != 0.5 * nranks * (nranks + 1) * (i + 1)) echo_detail = "the echo exchange returned a wrong sum (a peer's stores did not land)";
        if (!echo_detail.empty()) pc.shm->failed = 1;
    } else {
        pc.shm->failed = 1;
    }
    const bool met2 = peer_barrier(pc.shm, nranks, 120);
    if (!met2 || pc.shm->failed) {
        peer_release(false);
        return fail(BH_ERR_RCCL, "peer rendezvous: reachability check failed" + (echo_detail.empty() ? std::string(" on another rank") : ": " + echo_detail));
    }
    pc.active = true;
    return BH_OK;
}

int32_t bh_comm_unique_id(void* id_out) {
    BH_REQUIRE_INIT();
    if (!id_out) return fail(BH_ERR_INVALID_ARG, "NULL id_out");
    static_assert(sizeof(ncclUniqueId) == BH_UNIQUE_ID_BYTES, "ncclUniqueId size");
    const int mode = comm_mode();
    if (mode == 0) return fail(BH_ERR_INVALID_ARG, "BH_COMM must be rccl, ipc or both");
    if (mode & COMM_RCCL) {
        BH_TRY(load_rccl());
        ncclUniqueId id;
        BH_NCCL(g_ctx.p_ncclGetUniqueId(&id));
        memcpy(id_out, &id, sizeof(id));
        return BH_OK;
    }
    // peer buffers only: the id merely names the rendezvous page
    unsigned char* o = static_cast<unsigned char*>(id_out);
    memset(o, 0, BH_UNIQUE_ID_BYTES);
    FILE* f = fopen("/dev/urandom", "rb");
    const size_t got = f ? fread(o, 1, 64, f) : 0;
    if (f) fclose(f);
    const unsigned long long salt = (unsigned long long)getpid() ^ (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count();
    memcpy(o + 64, &salt, sizeof(salt));
    memcpy(o + 72, &got, sizeof(got));
    return BH_OK;
}

int32_t bh_comm_init(int32_t rank, int32_t nranks, const void* id_in) {
    BH_REQUIRE_INIT();
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(BH_ERR_INVALID_ARG, "bad rank/nranks");
    if (comm_active()) return fail(BH_ERR_INVALID_ARG, "communicator already initialised");
    // nranks == 1 needs no communicator; BH_FORCE_COMM=1 creates a 1-rank communicator anyway so that the whole
    // exchange path (RCCL: dlopen, ncclCommInitRank, ncclAllReduce on the library stream; peer buffers: inbox, flags,
    // the fused reduce+exchange kernel) can be exercised and timed on a one-GPU box.
    const char* force = getenv("BH_FORCE_COMM");
    if (nranks == 1 && !(force && atoi(force) != 0)) { g_ctx.rank = 0; g_ctx.nranks = 1; return BH_OK; }
    // a bh_hess bakes in which rank applies the replicated C rows (rank 0): the rank must not change under a live handle
    if (g_ctx.live_hess > 0) return fail(BH_ERR_PRECONDITION, "bh_comm_init: destroy all bh_hess handles first (create them after the communicator)");
    if (!id_in) return fail(BH_ERR_INVALID_ARG, "NULL unique id");
    const int mode = comm_mode();
    if (mode == 0) return fail(BH_ERR_INVALID_ARG, "BH_COMM must be rccl, ipc or both");
    g_ctx.rank = rank;
    g_ctx.nranks = nranks;
    if (mode & COMM_RCCL) {
        int32_t rc = load_rccl();
        if (rc == BH_OK) {
            ncclUniqueId id;
            memcpy(&id, id_in, sizeof(id));
            ncclResult_t r = g_ctx.p_ncclCommInitRank(&g_ctx.comm, nranks, id, rank);
            if (r != ncclSuccess) { g_ctx.comm = nullptr; rc = fail(BH_ERR_RCCL, std::string("ncclCommInitRank: ") + g_ctx.p_ncclGetErrorString(r)); }
        }
        if (rc != BH_OK) { g_ctx.rank = 0; g_ctx.nranks = 1; return rc; }
    }
    if (mode & COMM_IPC) {
        const int32_t rc = peer_init(rank, nranks, static_cast<const unsigned char*>(id_in));
        if (rc != BH_OK) {
            if (g_ctx.comm && g_ctx.p_ncclCommDestroy) { g_ctx.p_ncclCommDestroy(g_ctx.comm); g_ctx.comm = nullptr; }
            g_ctx.rank = 0; g_ctx.nranks = 1;
            return rc;
        }
    }
    g_ctx.comm_path = (mode == COMM_IPC) ? 1 : 0;
    return BH_OK;
}

int32_t bh_comm_destroy(void) {
    if (comm_active() && g_ctx.live_hess > 0) return fail(BH_ERR_PRECONDITION, "bh_comm_destroy: destroy all bh_hess handles first");
    if (comm_active() && g_ctx.stream) (void)hipStreamSynchronize(g_ctx.stream);
    if (g_ctx.comm && g_ctx.p_ncclCommDestroy) g_ctx.p_ncclCommDestroy(g_ctx.comm);
    if (g_ctx.peer.active) peer_release(true);
    g_ctx.comm = nullptr; g_ctx.rank = 0; g_ctx.nranks = 1; g_ctx.comm_path = 0;
    return BH_OK;
}

int32_t bh_comm_info(int32_t* rank, int32_t* nranks) {
    if (rank) *rank = g_ctx.rank;
    if (nranks) *nranks = g_ctx.nranks;
    return BH_OK;
}

// ---- AlHessian ------------------------------------------------------------------------------
int32_t bh_hess_create(bh_hess** out, const double* J, int64_t d, int64_t n, int64_t ldJ, const double* C, int64_t q,
                       int64_t ldC, double mu) {
    BH_REQUIRE_INIT();
    if (!out) return fail(BH_ERR_INVALID_ARG, "NULL out");
    *out = nullptr;
    if (d < 0 || n < 1 || q < 0) return fail(BH_ERR_INVALID_ARG, "negative dimension");
    if (d > 0 && (!J || ldJ < d)) return fail(BH_ERR_INVALID_ARG, "J NULL or ldJ < d");
    if (q > 0 && (!C || ldC < q)) return fail(BH_ERR_INVALID_ARG, "C NULL or ldC < q");
    bh_hess* H = new bh_hess();
    H->d = d; H->n = n; H->q = q; H->mu = mu;
    int32_t rc = alloc_hess_common(H);
    if (rc == BH_OK) rc = upload_transposed(J, d, n, ldJ, H->Jd, 0, H->ld);
    if (rc == BH_OK) rc = upload_transposed(C, q, n, ldC, H->Jd, d, H->ld);
    if (rc == BH_OK) rc = finish_hess_create(H);
    if (rc == BH_OK) rc = sync_flush();
    if (rc != BH_OK) { bh_hess_destroy(H); return rc; }
    *out = H;
    H->counted = true;
    g_ctx.live_hess += 1;
    return BH_OK;
}

int32_t bh_hess_create_dev(bh_hess** out, const double* J_dev, int64_t d, int64_t n, int64_t ldJ, const double* C, int64_t q,
                           int64_t ldC, double mu) {
    BH_REQUIRE_INIT();
    if (!out) return fail(BH_ERR_INVALID_ARG, "NULL out");
    *out = nullptr;
    if (d < 0 || n < 1 || q < 0) return fail(BH_ERR_INVALID_ARG, "negative dimension");
    if (d > 0 && (!J_dev || ldJ < d)) return fail(BH_ERR_INVALID_ARG, "J NULL or ldJ < d");
    if (q > 0 && (!C || ldC < q)) return fail(BH_ERR_INVALID_ARG, "C NULL or ldC < q");
    bh_hess* H = new bh_hess();
    H->d = d; H->n = n; H->q = q; H->mu = mu;
    int32_t rc = alloc_hess_common(H);
    if (rc == BH_OK) rc = transpose_from_device(J_dev, d, n, ldJ, H->Jd, 0, H->ld);
    if (rc == BH_OK) rc = upload_transposed(C, q, n, ldC, H->Jd, d, H->ld);
    if (rc == BH_OK && hipStreamSynchronize(g_ctx.stream) != hipSuccess) rc = fail(BH_ERR_HIP, "bh_hess_create_dev: synchronize");
    if (rc == BH_OK) rc = finish_hess_create(H);
    if (rc != BH_OK) { bh_hess_destroy(H); return rc; }
    *out = H;
    H->counted = true;
    g_ctx.live_hess += 1;
    return BH_OK;
}

static int32_t gram_enter(bh_hess* H);

// f-4: the same upload without blocking the caller.  J must stay valid and unchanged until bh_hess_wait (or the first use
// of the handle, which waits implicitly) returns.
int32_t bh_hess_create_async(bh_hess** out, const double* J, int64_t d, int64_t n, int64_t ldJ, const double* C, int64_t q,
                             int64_t ldC, double mu) {
    BH_REQUIRE_INIT();
    if (!out) return fail(BH_ERR_INVALID_ARG, "NULL out");
    *out = nullptr;
    if (d < 0 || n < 1 || q < 0) return fail(BH_ERR_INVALID_ARG, "negative dimension");
    if (d > 0 && (!J || ldJ < d)) return fail(BH_ERR_INVALID_ARG, "J NULL or ldJ < d");
    if (q > 0 && (!C || ldC < q)) return fail(BH_ERR_INVALID_ARG, "C NULL or ldC < q");
    bh_hess* H = new bh_hess();
    H->d = d; H->n = n; H->q = q; H->mu = mu;
    int32_t rc = alloc_hess_common(H);
    // option gram_ingest (one rank, n <= 16384; elsewhere the call is what it is without the option): the handle is born in the Gram form
    const bool ingest = g_ctx.opt_gram_ingest != 0 && n <= 16384 && !(comm_active() && g_ctx.nranks > 1);
    if (rc == BH_OK && ingest) rc = gram_enter(H);
    if (rc == BH_OK) rc = upload_transposed(C, q, n, ldC, H->Jd, d, H->ld);      // the C block is small: synchronous
    if (rc == BH_OK && hipStreamSynchronize(g_ctx.stream) != hipSuccess) rc = fail(BH_ERR_HIP, "bh_hess_create_async: synchronize");
    if (rc == BH_OK && d > 0) {
        // column chunks of ~upload_chunk_mb MiB, a multiple of 32 columns (the transpose's tile width)
        int64_t cc = (g_ctx.opt_upload_chunk_mb << 20) / (8 * std::max<int64_t>(d, 1));
        cc = std::max<int64_t>(32, cc / 32 * 32);
        cc = std::min<int64_t>(cc, round_up(n, 32));
        const size_t need = (size_t)d * cc * sizeof(double);
        AsyncUpload* u = g_ctx.upload_cache;           // the previous upload's resources, if they are free and large enough
        g_ctx.upload_cache = nullptr;
        if (u && u->staging_bytes < need) { async_upload_destroy(u); u = nullptr; }
        bool ok = true;
        if (!u) {
            u = new AsyncUpload();
            ok = hipStreamCreateWithFlags(&u->s_copy, hipStreamNonBlocking) == hipSuccess &&
                 hipStreamCreateWithFlags(&u->s_xpose, hipStreamNonBlocking) == hipSuccess;
            for (int i = 0; i < 2 && ok; ++i) {
                ok = hipEventCreateWithFlags(&u->copied[i], hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&u->freed[i], hipEventDisableTiming) == hipSuccess &&
                     hipMalloc(reinterpret_cast<void**>(&u->staging[i]), need) == hipSuccess;
            }
            u->staging_bytes = need;
        }
        u->chunk_cols = cc;
        u->rc = BH_OK;
        u->gram = ingest;
        if (ok && ingest) {
            // one more stream (with the copy, the transpose and the library stream: four) and the partial blocks of the largest step
            u->gram_mu = mu;
            u->gram_plan = gram_ingest_plan(H->ld, cc, (n + cc - 1) / cc, d + H->q_eff, g_ctx.n_cu);
            if (!u->s_gram) ok = hipStreamCreateWithFlags(&u->s_gram, hipStreamNonBlocking) == hipSuccess;
            if (ok && u->gram_part_doubles < u->gram_plan.part_doubles) {
                dev_free(u->gram_part);
                u->gram_part = nullptr;
                u->gram_part_doubles = 0;
                ok = hipMalloc(reinterpret_cast<void**>(&u->gram_part), (size_t)u->gram_plan.part_doubles * sizeof(double)) == hipSuccess;
                if (ok) u->gram_part_doubles = u->gram_plan.part_doubles;
            }
        }
        if (!ok) {
            async_upload_destroy(u);
            rc = fail(BH_ERR_HIP, "bh_hess_create_async: streams / events / staging buffers");
        } else {
            H->up = u;
            u->worker = std::thread(async_upload_worker, H, J, d, n, ldJ, g_ctx.device);
        }
    } else if (rc == BH_OK) {
        // no rows on this rank (d_total < ranks): nothing to upload, but the d_total all-reduce of finish_hess_create must run where
        // the peers run theirs — at bh_hess_wait / first use — or any collective issued between create and wait (bh_resid_sqnorm,
        // another handle) would be matched against it
        if (comm_active()) H->pending_finish = true;
        else rc = finish_hess_create(H);
    }
    if (rc != BH_OK) { bh_hess_destroy(H); return rc; }
    *out = H;
    H->counted = true;
    g_ctx.live_hess += 1;
    return BH_OK;
}

int32_t bh_hess_wait(bh_hess* H) {
    BH_REQUIRE_INIT();
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    return hess_ready(H);
}

int32_t bh_hess_create_synthetic(bh_hess** out, int64_t d, int64_t n, int64_t row0, int64_t d_total, uint64_t seed,
                                 const double* colscale, double mu) {
    BH_REQUIRE_INIT();
    if (!out) return fail(BH_ERR_INVALID_ARG, "NULL out");
    *out = nullptr;
    if (d < 1 || n < 1 || row0 < 0 || d_total < row0 + d) return fail(BH_ERR_INVALID_ARG, "bad synthetic shape");
    bh_hess* H = new bh_hess();
    H->d = d; H->n = n; H->q = 0; H->mu = mu;
    int32_t rc = alloc_hess_common(H);
    if (rc != BH_OK) { bh_hess_destroy(H); return rc; }
    double* cs_dev = nullptr;
    if (colscale) {
        rc = dev_alloc(&cs_dev, n);
        if (rc == BH_OK && hipMemcpyAsync(cs_dev, colscale, (size_t)n * sizeof(double), hipMemcpyHostToDevice, g_ctx.stream) != hipSuccess)
            rc = fail(BH_ERR_HIP, "colscale upload");
        if (rc != BH_OK) { dev_free(cs_dev); bh_hess_destroy(H); return rc; }
    }
    hipLaunchKernelGGL(synth_fill_kernel, dim3(g_ctx.n_cu * 8), dim3(256), 0, g_ctx.stream, H->Jd, H->ld, d, n, row0, d_total,
                       seed, cs_dev, std::sqrt((double)d_total));
    hipError_t e = hipStreamSynchronize(g_ctx.stream);
    dev_free(cs_dev);
    if (e != hipSuccess) { bh_hess_destroy(H); return fail(BH_ERR_HIP, std::string("synth_fill: ") + hipGetErrorString(e)); }
    rc = finish_hess_create(H);
    if (rc != BH_OK) { bh_hess_destroy(H); return rc; }
    *out = H;
    H->counted = true;
    g_ctx.live_hess += 1;
    return BH_OK;
}

int32_t bh_hess_set_mu(bh_hess* H, double mu) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (mu == H->mu) return BH_OK;          // the Julia shim calls this on every handle(H): never a rebuild
    H->mu = mu;
    H->G_valid = false;                      // Gram form: rebuilt before the next product that reads G
    g_ctx.notes.handle_changed(H);
    return BH_OK;
}

static void gram_free(bh_hess* H) {
    if (H->G || H->gpart) {
        if (g_ctx.init) (void)hipStreamSynchronize(g_ctx.stream);   // launches still reading G may be queued
        dev_free(H->G); dev_free(H->gpart); dev_free(H->geq); dev_free(H->csort);
    }
    H->G = nullptr; H->gpart = nullptr; H->geq = nullptr; H->geq_doubles = 0; H->csort = nullptr;
    H->G_valid = false;
}

// Into the Gram form: G and the partial sums of the one-shot build; G stale.  A failed allocation leaves the implicit form.
static int32_t gram_enter(bh_hess* H) {
    int slabs = 1;
    int64_t slab_rows = 0;
    gram_geometry(H, &slabs, &slab_rows);
    int32_t rc = dev_alloc(&H->G, H->ld * H->ld);
    if (rc == BH_OK && slabs > 1) rc = dev_alloc(&H->gpart, (int64_t)slabs * H->ld * H->ld);
    if (rc != BH_OK) { gram_free(H); return rc; }        // the handle stays in the implicit form
    H->gram_slabs = slabs;
    H->gram_slab_rows = slab_rows;
    H->G_valid = false;                                  // built before the first product that reads it (after the ingest)
    H->form = BH_HESS_GRAM;
    H->stats.bytes_per_hmul = hmul_bytes(H);
    H->timed_bytes = 0.0; H->timed_n = 0;
    g_ctx.notes.handle_changed(H);
    return BH_OK;
}

int32_t bh_hess_set_form(bh_hess* H, int32_t form) {
    BH_REQUIRE_INIT();
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (form != BH_HESS_IMPLICIT && form != BH_HESS_GRAM) return fail(BH_ERR_INVALID_ARG, "form is BH_HESS_IMPLICIT (0) or BH_HESS_GRAM (1)");
    if (form == H->form) return BH_OK;
    if (form == BH_HESS_GRAM) {
        if (H->n > 16384) return fail(BH_ERR_UNSUPPORTED, "Gram form: n > 16384 (G would exceed 2 GiB)");
        if (comm_active() && g_ctx.nranks > 1) return fail(BH_ERR_UNSUPPORTED, "Gram form: one rank only (no all-reduce of G)");
        return gram_enter(H);
    }
    // an upload that is building G (option gram_ingest): join the worker, which drains its Gram launches, before G goes
    const int32_t rc = (H->up && H->up->gram) ? hess_ready(H) : BH_OK;
    gram_free(H);
    H->form = form;
    H->stats.bytes_per_hmul = hmul_bytes(H);
    H->timed_bytes = 0.0; H->timed_n = 0;
    g_ctx.notes.handle_changed(H);
    return rc;
}

int32_t bh_hess_get_form(const bh_hess* H, int32_t* form, int64_t* gram_builds) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (form) *form = H->form;
    if (gram_builds) *gram_builds = H->gram_builds;
    return BH_OK;
}

int32_t bh_hess_set_gram_read(bh_hess* H, int32_t mode) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (!gram_read_mode_ok(mode)) return fail(BH_ERR_INVALID_ARG, "mode is BH_GRAM_READ_FULL (0), BH_GRAM_READ_LOWER (1) or BH_GRAM_READ_LOWER_QUAD (2)");
    if (mode == H->gram_read) return BH_OK;
    const double before = hmul_bytes(H);
    H->gram_read = mode;
    if (hmul_bytes(H) != before) {              // the bytes a product streams changed: the mean over sampled launches starts again
        H->stats.bytes_per_hmul = hmul_bytes(H);
        H->timed_bytes = 0.0; H->timed_n = 0;
    }
    return BH_OK;
}

int32_t bh_hess_get_gram_read(const bh_hess* H, int32_t* mode, int32_t* served, int64_t* products_lower, int64_t* quads_from_g) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (mode) *mode = H->gram_read;
    if (served) *served = gram_served(H) ? 1 : 0;
    if (products_lower) *products_lower = H->products_lower;
    if (quads_from_g) *quads_from_g = H->quads_from_g;
    return BH_OK;
}

int32_t bh_hess_set_cauchy_search(bh_hess* H, int32_t mode) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (mode != BH_CAUCHY_STEPWISE && mode != BH_CAUCHY_SORTED) return fail(BH_ERR_INVALID_ARG, "mode is BH_CAUCHY_STEPWISE (0) or BH_CAUCHY_SORTED (1)");
    H->cauchy_search = mode;                    // (G, the step-chain ledger and the byte counters do not depend on it)
    return BH_OK;
}

int32_t bh_hess_get_cauchy_search(const bh_hess* H, int32_t* mode, int32_t* served, int64_t* searches_sorted) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (mode) *mode = H->cauchy_search;
    if (served) *served = H->n <= 16384 ? 1 : 0;
    if (searches_sorted) *searches_sorted = H->searches_sorted;
    return BH_OK;
}

int32_t bh_hess_set_cauchy_rows(bh_hess* H, int32_t mode) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (mode != BH_CAUCHY_ROWS_STEPWISE && mode != BH_CAUCHY_ROWS_SORTED)
        return fail(BH_ERR_INVALID_ARG, "mode is BH_CAUCHY_ROWS_STEPWISE (0) or BH_CAUCHY_ROWS_SORTED (1)");
    H->cauchy_rows = mode;                      // (J, G, the step-chain ledger and the byte counters do not depend on it)
    return BH_OK;
}

int32_t bh_hess_get_cauchy_rows(const bh_hess* H, int32_t* mode, int32_t* served, int64_t* searches_rows_sorted) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (mode) *mode = H->cauchy_rows;
    if (served) *served = cauchy_rows_served(H->n, H->ld) ? 1 : 0;
    if (searches_rows_sorted) *searches_rows_sorted = H->searches_rows_sorted;
    return BH_OK;
}

static bool cauchy_rows_workspace(bh_hess* H, hipStream_t s);

// With a communicator the workspace of the sorted rows form is allocated HERE, not at the first search: every rank learns at the same
// call whether it can take part, and no rank finds out alone, in the middle of a search, that it has to fall back.
int32_t bh_hess_set_cauchy_rows_ranks(bh_hess* H, int32_t on) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (on != 0 && on != 1) return fail(BH_ERR_INVALID_ARG, "on is 0 or 1");
    if (on == 1 && cauchy_rows_served(H->n, H->ld) && !cauchy_rows_workspace(H, g_ctx.stream))
        return fail(BH_ERR_HIP, "bh_hess_set_cauchy_rows_ranks: no room for the workspace of the sorted rows form");
    H->cauchy_rows_ranks = on;                  // (J, G, the step-chain ledger and the byte counters do not depend on it)
    return BH_OK;
}

int32_t bh_hess_get_cauchy_rows_ranks(const bh_hess* H, int32_t* on) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (on) *on = H->cauchy_rows_ranks;
    return BH_OK;
}

int32_t bh_hess_free_image_info(const bh_hess* H, const bh_proj* P, int32_t* state, int64_t* width, int64_t* builds, int64_t* moves,
                                int64_t* calls_served) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    const FreeImageBook& b = H->fi;
    int st = FI_STATE_NONE;
    if (b.present) {
        st = FI_STATE_VALID;
        if (P != nullptr && H->fi_epoch != P->mask_epoch) {
            const bool known = P->active_set && P->n == H->n && P->last_chunks.size() == (size_t)((H->n + 63) / 64);
            st = known ? free_image_state(b, P->last_chunks.data()) : FI_STATE_STALE;
        }
    }
    if (state) *state = st;
    if (width) *width = b.present ? b.nfree : 0;
    if (builds) *builds = b.builds;
    if (moves) *moves = b.moves;
    if (calls_served) *calls_served = b.served;
    return BH_OK;
}

int32_t bh_hess_free_image_read(bh_hess* H, double* image_out, int64_t image_cap, int32_t* map_out, int64_t map_cap, int64_t* rows,
                                int64_t* stride) {
    BH_REQUIRE_INIT();
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (!H->fi.present) return fail(BH_ERR_PRECONDITION, "bh_hess_free_image_read: the handle has no compact image");
    const int64_t nrows = H->d + H->q_eff, ldf = H->fi.ldf;
    if (rows) *rows = nrows;
    if (stride) *stride = ldf;
    if ((image_out && image_cap < nrows * ldf) || (map_out && map_cap < ldf)) return fail(BH_ERR_INVALID_ARG, "bh_hess_free_image_read: buffer too small");
    if (image_out) {
        count_d2h((size_t)(nrows * ldf) * sizeof(double));
        note_dma();
        BH_HIP(hipMemcpyAsync(image_out, H->Jf, (size_t)(nrows * ldf) * sizeof(double), hipMemcpyDeviceToHost, g_ctx.stream));
    }
    if (map_out) {
        count_d2h((size_t)ldf * sizeof(int));
        note_dma();
        BH_HIP(hipMemcpyAsync(map_out, H->fi_map, (size_t)ldf * sizeof(int), hipMemcpyDeviceToHost, g_ctx.stream));
    }
    BH_TRY(sync_flush());
    return BH_OK;
}

int32_t bh_hess_destroy(bh_hess* H) {
    g_ctx.notes.handle_changed(H);
    if (!H) return BH_OK;
    if (H->up) {                              // an upload still in flight: let it finish before its buffers go
        AsyncUpload* u = H->up;
        if (u->worker.joinable()) u->worker.join();
        async_upload_cleanup(u);
        H->up = nullptr;
    }
    if (H->counted) g_ctx.live_hess -= 1;
    if (g_ctx.init) (void)hipStreamSynchronize(g_ctx.stream);
    image_release(H->Jd, H->Jd_doubles);
    image_release(H->Jf, H->Jf_doubles);                          // (the stream is drained: no launch still reads the compact image)
    dev_free(H->Af);
    dev_free(H->fi_map); dev_free(H->fi_ops);
    dev_free(H->vpad); dev_free(H->zpad); dev_free(H->upad); dev_free(H->tbuf); dev_free(H->timg); dev_free(H->timg_gen); dev_free(H->cblk);
    dev_free(H->partials); dev_free(H->sq_partials); dev_free(H->scalar);
    dev_free(H->G); dev_free(H->gpart); dev_free(H->geq); dev_free(H->csort); dev_free(H->crows);
    for (auto e : H->ev) if (e) (void)hipEventDestroy(e);
    delete H;
    return BH_OK;
}

int32_t bh_hess_shape(const bh_hess* H, int64_t* d, int64_t* n, int64_t* q) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (d) *d = H->d;
    if (n) *n = H->n;
    if (q) *q = H->q;
    return BH_OK;
}

static int32_t hmul_impl(bh_hess* H, const double* v, double* out, bool dev) {
    BH_REQUIRE_INIT();
    if (!H || !v || !out) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    const double* vp = H->vpad;
    if (dev) BH_TRY(device_operand(&vp, H->vpad, v, H->n, H->ld));
    else BH_TRY(stage_vec(H->vpad, v, H->n, false));
    BH_TRY(launch_hmul(H, vp, H->zpad, nullptr, -1));
    BH_TRY(fetch_vec(out, H->zpad, H->n, dev));
    BH_TRY(dev ? finish_device_call() : sync_flush());
    H->stats.n_hmul += 1;
    return BH_OK;
}
int32_t bh_hmul(bh_hess* H, const double* v, double* out_n) { return hmul_impl(H, v, out_n, false); }
int32_t bh_hmul_dev(bh_hess* H, const double* v_dev, double* out_n_dev) { return hmul_impl(H, v_dev, out_n_dev, true); }

int32_t bh_vthv(bh_hess* H, const double* v, double* out_scalar) {
    BH_REQUIRE_INIT();
    if (!H || !v || !out_scalar) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    BH_TRY(stage_vec(H->vpad, v, H->n, false));
    BH_TRY(launch_quad(H, H->vpad));
    BH_TRY(fetch_vec(out_scalar, H->scalar, 1, false));
    BH_TRY(sync_flush());
    return BH_OK;
}

static int32_t jv_impl(bh_hess* H, const double* v, double* out, bool dev) {
    BH_REQUIRE_INIT();
    if (!H || !v || (!out && H->d > 0)) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    if (dev) {
        const double* vp = H->vpad;
        BH_TRY(device_operand(&vp, H->vpad, v, H->n, H->ld));
        BH_TRY(launch_jv(H, vp, out, false, nullptr));
        BH_TRY(finish_device_call());
    } else {
        BH_TRY(stage_vec(H->vpad, v, H->n, false));
        BH_TRY(launch_jv(H, H->vpad, H->upad, false, nullptr));
        BH_TRY(fetch_vec(out, H->upad, H->d, false));
        BH_TRY(sync_flush());
    }
    H->stats.n_jv += 1;
    return BH_OK;
}
int32_t bh_jv(bh_hess* H, const double* v, double* out_d) { return jv_impl(H, v, out_d, false); }
int32_t bh_jv_dev(bh_hess* H, const double* v_dev, double* out_d_dev) { return jv_impl(H, v_dev, out_d_dev, true); }

static int32_t jtv_impl(bh_hess* H, const double* u, double* out, bool dev) {
    BH_REQUIRE_INIT();
    if (!H || (!u && H->d > 0) || !out) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    const double* u_dev = u;
    if (!dev) { BH_TRY(stage_vec(H->upad, u, H->d, false)); u_dev = H->upad; }
    BH_TRY(launch_jtv(H, u_dev, H->zpad));
    BH_TRY(fetch_vec(out, H->zpad, H->n, dev));
    BH_TRY(dev ? finish_device_call() : sync_flush());
    H->stats.n_jtv += 1;
    return BH_OK;
}
int32_t bh_jtv(bh_hess* H, const double* u, double* out_n) { return jtv_impl(H, u, out_n, false); }
int32_t bh_jtv_dev(bh_hess* H, const double* u_dev, double* out_n_dev) { return jtv_impl(H, u_dev, out_n_dev, true); }

// ---- MixedConstraints -----------------------------------------------------------------------
int32_t bh_proj_create(bh_proj** out, const double* A, int64_t mA, int64_t n, int64_t ldA) {
    BH_REQUIRE_INIT();
    if (!out) return fail(BH_ERR_INVALID_ARG, "NULL out");
    *out = nullptr;
    if (mA < 0 || n < 1) return fail(BH_ERR_INVALID_ARG, "negative dimension");
    if (mA > 0 && (!A || ldA < mA)) return fail(BH_ERR_INVALID_ARG, "A NULL or ldA < mA");
    if (mA > n) return fail(BH_ERR_PRECONDITION, "mA > n");
    bh_proj* P = new bh_proj();
    P->mA = mA; P->n = n; P->ldA = round_up(n, 16);
    int32_t rc = dev_alloc(&P->Ad, std::max<int64_t>(mA, 1) * P->ldA);
    if (rc == BH_OK) rc = dev_alloc(&P->fixrank, P->ldA);
    if (rc == BH_OK) rc = dev_alloc(&P->fixidx, n);
    if (rc == BH_OK) rc = dev_alloc(&P->newidx, n);
    if (rc == BH_OK) rc = dev_alloc(&P->counts, 8);
    if (rc == BH_OK) rc = dev_alloc(&P->chunks_dev, (n + 63) / 64 + 1);
    if (rc == BH_OK) rc = dev_alloc(&P->tw, n + 16);
    if (rc == BH_OK) rc = dev_alloc(&P->rpad, P->ldA);
    if (rc == BH_OK) rc = dev_alloc(&P->vtmp, P->ldA);
    if (rc == BH_OK && hipMemsetAsync(P->rpad, 0, P->ldA * sizeof(double), g_ctx.stream) != hipSuccess) rc = fail(BH_ERR_HIP, "memset");
    if (rc == BH_OK && hipMemsetAsync(P->fixrank, 0xff, P->ldA * sizeof(int), g_ctx.stream) != hipSuccess) rc = fail(BH_ERR_HIP, "memset");
    if (rc == BH_OK) rc = upload_transposed(A, mA, n, ldA, P->Ad, 0, P->ldA);
    if (rc != BH_OK) { bh_proj_destroy(P); return rc; }
    P->mask_epoch = ++g_mask_epoch;
    P->nfix = 0; P->mpp = (int)mA;
    BH_TRY(sync_flush());
    *out = P;
    return BH_OK;
}

int32_t bh_proj_set_active(bh_proj* P, const uint64_t* fix_chunks, int64_t n, const double* L, int64_t mpp, int64_t ldL) {
    BH_REQUIRE_INIT();
    if (!P) return fail(BH_ERR_INVALID_ARG, "NULL bh_proj");
    if (n != P->n) return fail(BH_ERR_SHAPE, "fixvars length differs from n");
    int nfix = 0;
    if (fix_chunks) {
        for (int64_t wd = 0; wd < (n + 63) / 64; ++wd) {
            uint64_t bits = fix_chunks[wd];
            if (wd == (n + 63) / 64 - 1 && (n & 63)) bits &= (1ull << (n & 63)) - 1ull;      // stray bits beyond n do not count
            nfix += __builtin_popcountll(bits);
        }
    }
    const int64_t want = P->mA + nfix;
    const size_t nwords = (size_t)((n + 63) / 64);
    {   // The Julia shim re-pushes before every projection; with the reduced form (or no linear rows) the device state
        // depends on fixvars only, so an identical push is a no-op (no upload, no refactorisation).
        const bool form_reduced = (P->mA == 0) || (g_ctx.opt_proj_form != 0);
        if (form_reduced && P->active_set && P->reduced == (P->mA > 0) && fix_chunks && P->last_chunks.size() == nwords &&
            memcmp(P->last_chunks.data(), fix_chunks, nwords * sizeof(uint64_t)) == 0)
            return BH_OK;       // whole words compared: stray bits beyond n only ever cause a (harmless) rebuild
    }
    if (want > n) return fail(BH_ERR_PRECONDITION, "mpp = mA + count(fixvars) > n (src/polyhedral_constraints.jl:43,128)");
    const bool reduced = (P->mA > 0) && (g_ctx.opt_proj_form != 0);
    if (P->mA > 0) {
        if (!L && !reduced) return fail(BH_ERR_INVALID_ARG, "L is required when mA > 0 (augmented form)");
        P->have_L = false;
        if (L) {
            if (mpp != want) return fail(BH_ERR_SHAPE, "mpp != mA + count(fixvars)");
            if (ldL < mpp) return fail(BH_ERR_INVALID_ARG, "ldL < mpp");
            if (!reduced) {
                if (mpp * mpp > P->L_cap) {
                    dev_free(P->L); P->L = nullptr; P->L_cap = 0;
                    BH_TRY(dev_alloc(&P->L, mpp * mpp));
                    P->L_cap = mpp * mpp;
                }
                count_h2d((size_t)mpp * mpp * sizeof(double));
                note_dma();
                BH_HIP(hipMemcpy2DAsync(P->L, (size_t)mpp * sizeof(double), L, (size_t)ldL * sizeof(double), (size_t)mpp * sizeof(double),
                                        (size_t)mpp, hipMemcpyHostToDevice, g_ctx.stream));
                P->have_L = true;
            }
        }
        const size_t lds = trsv_lds_bytes(reduced ? (int)P->mA : (int)want);
        if (lds > kLdsPerCu) return fail(BH_ERR_UNSUPPORTED, "factor too large for the single-workgroup triangular solve");
        BH_TRY(ensure_trsv_lds(lds));
    } else if (mpp != want && L != nullptr) {
        return fail(BH_ERR_SHAPE, "mpp != count(fixvars) for mA == 0");
    }
    // The mask goes up as the BitVector image it arrived as (n/8 bytes, through the pinned arena and a copy-free kernel read);
    // two small kernels expand it into fixrank / fixidx on the device.  (Fallback without a mapped arena: expanded on the host.)
    double* pin = arena_kernels() ? pin_alloc((int64_t)nwords) : nullptr;
    if (pin != nullptr) {
        if (fix_chunks) memcpy(pin, fix_chunks, nwords * sizeof(uint64_t));
        else memset(pin, 0, nwords * sizeof(uint64_t));
        count_h2d(nwords * sizeof(uint64_t));
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((P->ldA + 255) / 256, 256));
        hipLaunchKernelGGL(flags_from_chunks_kernel, dim3(grid), dim3(256), 0, g_ctx.stream,
                           reinterpret_cast<const unsigned long long*>(pin_dev_view(pin)), P->fixrank, (int)n, (int)P->ldA);
        hipLaunchKernelGGL(canon_mask_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, P->fixrank, P->fixidx, (int)n, (int)P->ldA,
                           (unsigned long long*)nullptr, P->counts);
        BH_HIP(hipGetLastError());
    } else {
        std::vector<int> rank((size_t)P->ldA, -1), idx;
        if (fix_chunks) {
            for (int64_t i = 0; i < n; ++i)
                if ((fix_chunks[i >> 6] >> (i & 63)) & 1ull) { rank[(size_t)i] = (int)idx.size(); idx.push_back((int)i); }
        }
        count_h2d((size_t)(P->ldA + nfix) * sizeof(int));
        note_dma();
        BH_HIP(hipMemcpyAsync(P->fixrank, rank.data(), (size_t)P->ldA * sizeof(int), hipMemcpyHostToDevice, g_ctx.stream));
        if (nfix > 0) BH_HIP(hipMemcpyAsync(P->fixidx, idx.data(), (size_t)nfix * sizeof(int), hipMemcpyHostToDevice, g_ctx.stream));
        BH_HIP(hipStreamSynchronize(g_ctx.stream));          // rank / idx are locals of this block
    }
    P->mask_epoch = ++g_mask_epoch;
    P->nfix = nfix; P->mpp = (int)want; P->reduced = reduced;
    int info_host = 0;
    if (reduced) {
        // reduced form: factor A_free A_free' (mA x mA) on the device; bound changes need no host factor
        BH_TRY(ensure_reduced_buffers(P));
        BH_TRY(launch_reduced_factor(P, nfix > 0, nullptr));
    }
    if (reduced && !g_pin.dma && g_ctx.mbox_h != nullptr) {
        // the factorisation flag rides to the host with the seal that ends the call
        BH_TRY(mbox_seal_and_wait(sizeof(int), nullptr, nullptr, nullptr, P->info, 1, mbox_dev<int>(kMbInts)));
        info_host = mbox_host<int>(kMbInts)[0];
    } else {
        if (reduced) {
            count_d2h(sizeof(int));
            note_dma();
            BH_HIP(hipMemcpyAsync(&info_host, P->info, sizeof(int), hipMemcpyDeviceToHost, g_ctx.stream));
        }
        BH_TRY(sync_flush());   // host vectors go out of scope
    }
    if (info_host != 0) {
        P->active_set = false;
        return fail(BH_ERR_PRECONDITION, "A_free*A_free' is not positive definite (PosDefException in the reference's cholesky)");
    }
    P->active_set = true;
    if (fix_chunks) {
        // whole words are kept and compared (Julia keeps the bits beyond n zero; stray bits only ever cause a rebuild)
        P->last_chunks.assign(fix_chunks, fix_chunks + nwords);
    } else {
        P->last_chunks.assign(nwords, 0ull);
    }
    return BH_OK;
}

int32_t bh_proj_destroy(bh_proj* P) {
    if (!P) return BH_OK;
    if (g_ctx.init) (void)hipStreamSynchronize(g_ctx.stream);
    dev_free(P->Ad); dev_free(P->fixrank); dev_free(P->fixidx); dev_free(P->L); dev_free(P->tw); dev_free(P->rpad); dev_free(P->vtmp);
    dev_free(P->Lr); dev_free(P->M); dev_free(P->W);            // (P->info points into P->counts)
    dev_free(P->newidx); dev_free(P->counts); dev_free(P->chunks_dev); dev_free(P->tpart);
    delete P;
    return BH_OK;
}

int32_t bh_proj_shape(const bh_proj* P, int64_t* mA, int64_t* n, int64_t* n_fixed) {
    if (!P) return fail(BH_ERR_INVALID_ARG, "NULL bh_proj");
    if (mA) *mA = P->mA;
    if (n) *n = P->n;
    if (n_fixed) *n_fixed = P->nfix;
    return BH_OK;
}

static int32_t project_impl(bh_proj* P, const double* r, double* v_out, bool dev) {
    BH_REQUIRE_INIT();
    BH_TRY(check_proj_ready(P));
    if (!r || !v_out) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    BH_TRY(stage_vec(P->rpad, r, P->n, dev));
    BH_TRY(launch_project(P, P->rpad, P->vtmp, nullptr));
    BH_TRY(fetch_vec(v_out, P->vtmp, P->n, dev));
    BH_TRY(dev ? finish_device_call() : sync_flush());
    return BH_OK;
}
int32_t bh_project(bh_proj* P, const double* r, double* v_out) { return project_impl(P, r, v_out, false); }
int32_t bh_project_dev(bh_proj* P, const double* r_dev, double* v_out_dev) { return project_impl(P, r_dev, v_out_dev, true); }

int32_t bh_left_mul(bh_proj* P, const double* x, double* out_mpp) {
    BH_REQUIRE_INIT();
    if (!P || !x || !out_mpp) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    BH_TRY(stage_vec(P->rpad, x, P->n, false));
    ProjArgs a = proj_args(P, nullptr, false);
    const int grid1 = a.mA + (a.nfix + 255) / 256;
    if (grid1 > 0) hipLaunchKernelGGL(proj_left_mul_kernel, dim3(grid1), dim3(256), 0, g_ctx.stream, a, P->rpad);
    BH_HIP(hipGetLastError());
    BH_TRY(fetch_vec(out_mpp, P->tw, P->mA + P->nfix, false));
    BH_TRY(sync_flush());
    return BH_OK;
}

int32_t bh_left_mul_tr(bh_proj* P, const double* y, double* out_n) {
    BH_REQUIRE_INIT();
    if (!P || !y || !out_n) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    BH_TRY(stage_vec(P->tw, y, P->mA + P->nfix, false));
    ProjArgs a = proj_args(P, nullptr, false);
    const int nch = ((int)P->n + 1) / 2;
    hipLaunchKernelGGL((proj_left_mul_tr_kernel<false, 4>), dim3((nch + 63) / 64), dim3(256), 0, g_ctx.stream, a,
                       (const double*)nullptr, P->vtmp);
    BH_HIP(hipGetLastError());
    BH_TRY(fetch_vec(out_n, P->vtmp, P->n, false));
    BH_TRY(sync_flush());
    return BH_OK;
}

// ---- projected_cg ---------------------------------------------------------------------------
// results_final: every kernel that writes w (or H*w) had COMPLETED before the launch that published `done` started (two-kernel
// iteration, loop stopped by the exit test in an H*p launch's prologue: solved / iterations exhausted).  The device-pointer entry
// point then returns without draining the stream: what is still in flight are prologue-only launches that write nothing.
// compact: the loop ran on the compact image of the free columns and left compact operands (a call handed back reports false).
struct PcgFin { int done, status, iter, n_hmul; bool results_final = false; unsigned tag = 0; bool compact = false; };

static void pcg_fin_fill(PcgFin* fin, const MirrorWord& mw, unsigned tag, bool results_final) {
    fin->done = mw.done; fin->status = mw.status; fin->iter = mw.iter; fin->n_hmul = mw.n_hmul;
    fin->results_final = results_final; fin->tag = tag;
}

// The tag of the next loop on the progress word (16 bits, never 0).
static unsigned next_mirror_tag(CgWorkspace& c) {
    c.tag = (c.tag + 1) & 0xffffu;
    if (c.tag == 0) c.tag = 1;
    return c.tag;
}

// g doubles as an H*p input: stale padding of its staged copy would be multiplied into the dot products.
static int32_t zero_staged_g_padding(CgWorkspace& c, const double* gp, int64_t n, int64_t n_pad, bool g_pad_zeroed) {
    if (gp == c.g && n < n_pad && !g_pad_zeroed) BH_HIP(hipMemsetAsync(c.g + n, 0, (size_t)(n_pad - n) * sizeof(double), g_ctx.stream));
    return BH_OK;
}

// How many iterations the host enqueues per launch-ahead batch.  One batch is always in flight while the host waits for
// the one before it, so the GPU never idles as long as the host can enqueue a batch faster than the GPU runs one; every
// iteration enqueued past the exit is a gated no-op that still costs ~1.5 us per kernel (measured, tools/dispatch_floor.py)
// and, with several ranks, a full all-reduce.  Long iterations (large J) therefore want batch 1, short ones a deeper queue.
// Measured at config 3 "ic" (23 iterations of 315 us): 7.247 ms per subproblem at batch 1, 7.281 at 4, 7.775 at 64.
static int launch_batch_size(const bh_hess* H) {
    if (g_ctx.opt_batch > 0) return (int)g_ctx.opt_batch;
    // rank-independent on purpose (see finish_hess_create): the even share of the rows over all ranks plus the full C
    // block, not this rank's own d + q_eff
    const double rows = H->form == BH_HESS_GRAM ? (double)H->ld : (double)((H->d_total + g_ctx.nranks - 1) / g_ctx.nranks + H->q);
    const double est_us = (multi_panel(H) ? 16.0 : 8.0) * rows * (double)H->n / 7.0e6;      // ~7 TB/s streaming rate
    return est_us >= 100.0 ? 1 : est_us >= 40.0 ? 2 : 4;
}

// ---- compact image of the free columns (option free_image) ----------------------------------
// Jf goes back to the image pool.  (Launches that read it may be queued: the stream is drained first.)
static void free_image_release(bh_hess* H) {
    g_ctx.notes.compact_slots_changed(H);                    // the map goes with the image
    if (H->Jf) {
        if (g_ctx.init) (void)hipStreamSynchronize(g_ctx.stream);
        image_release(H->Jf, H->Jf_doubles);
    }
    else if (H->Af && g_ctx.init) (void)hipStreamSynchronize(g_ctx.stream);
    dev_free(H->Af);                                         // Af goes wherever Jf goes: its slot order is Jf's
    H->Af = nullptr; H->Af_doubles = 0; H->af_epoch = 0;
    H->Jf = nullptr; H->Jf_doubles = 0; H->fi_epoch = 0;
    H->fi.present = false;
}

// Bytes one H*p of the CG loop streams from the compact image at its current width (hmul_bytes with n -> nfree).
static double free_image_bytes(const bh_hess* H) {
    return 8.0 * (double)(H->d + H->q_eff) * (double)H->fi.nfree + 16.0 * (double)H->fi.nfree;
}

// Decides, for one eligible call, whether its CG loop runs on the compact image (*use), building it or moving columns first
// when the policy says so (bh_free_image_plan.h).  *earns: the call runs on the full image and earns credit towards a build.
// An allocation that fails leaves the handle on the full image without an error.
static int32_t free_image_prepare(bh_hess* H, bh_proj* P, bool* use, bool* earns) {
    *use = false; *earns = false;
    const int opt = (int)g_ctx.opt_free_image;
    if (opt == 0 || P->nfix <= 0) return BH_OK;
    FreeImageBook& b = H->fi;
    if (b.present && H->fi_epoch == P->mask_epoch) { b.served += 1; *use = true; return BH_OK; }      // the same active set as last time
    // the host's copy of the mask decides, and only when it is current (bh_cauchy_step leaves the device mask ahead of the host
    // until its renumbering has come back)
    const int64_t n = H->n;
    const size_t nwords = (size_t)((n + 63) / 64);
    if (!P->active_set || P->last_chunks.size() != nwords) return BH_OK;
    const uint64_t* want = P->last_chunks.data();
    if (free_image_count(want, n) != P->nfix) return BH_OK;
    int64_t k_new = 0, k_freed = 0;
    if (b.present) free_image_diff(b, want, &k_new, &k_freed);
    const int64_t nrows = H->d + H->q_eff;
    const FreeImageAction act = free_image_decide(opt, b.present, nrows, n, P->nfix, k_new, k_freed, b.credit, H->last_n_hmul);
    hipStream_t s = g_ctx.stream;
    if (act == FI_FULL) {
        *earns = opt == 1 && !(b.present && k_freed == 0) && free_image_worthwhile(nrows, P->nfix, H->last_n_hmul);
        return BH_OK;
    }
    if (act == FI_USE) { H->fi_epoch = P->mask_epoch; b.served += 1; *use = true; return BH_OK; }        // an identical mask pushed again
    if (act == FI_MOVE) {
        g_ctx.notes.compact_slots_changed(H);
        free_image_book_move(b, want, H->fi_ops_h);
        const int k = (int)H->fi_ops_h.size();
        count_h2d((size_t)k * sizeof(int));
        note_dma();
        BH_HIP(hipMemcpyAsync(H->fi_ops, H->fi_ops_h.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice, s));
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((nrows * k + 255) / 256, (int64_t)g_ctx.n_cu * 8));
        hipLaunchKernelGGL(free_image_move_kernel, dim3(grid), dim3(256), 0, s, H->Jf, b.ldf, nrows, (int)b.nfree, k, (const int*)H->fi_ops, H->fi_map);
        BH_HIP(hipGetLastError());
        H->fi_epoch = P->mask_epoch; b.served += 1; *use = true;
        return BH_OK;
    }
    // FI_BUILD (also: again, after a variable was freed — the image never grows)
    free_image_release(H);
    if (!H->fi_map) {
        if (hipMalloc(reinterpret_cast<void**>(&H->fi_map), (size_t)H->ld * sizeof(int)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&H->fi_ops), (size_t)H->ld * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError();
            dev_free(H->fi_map); dev_free(H->fi_ops);
            H->fi_map = nullptr; H->fi_ops = nullptr;
            return BH_OK;
        }
    }
    g_ctx.notes.compact_slots_changed(H);
    free_image_book_build(b, want, n);
    b.present = false;                                       // until the image exists
    const int64_t need = std::max<int64_t>(nrows, 1) * b.ldf;
    if (!image_from_pool(need, &H->Jf, &H->Jf_doubles)) {
        if (hipMalloc(reinterpret_cast<void**>(&H->Jf), (size_t)need * sizeof(double)) != hipSuccess) {   // out of memory: the handle stays on the full image
            (void)hipGetLastError();
            H->Jf = nullptr; H->Jf_doubles = 0; b.builds -= 1;
            return BH_OK;
        }
        H->Jf_doubles = need;
    }
    b.present = true;
    count_h2d((size_t)b.ldf * sizeof(int));
    note_dma();
    BH_HIP(hipMemcpyAsync(H->fi_map, b.map.data(), (size_t)b.ldf * sizeof(int), hipMemcpyHostToDevice, s));
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nrows, (int64_t)g_ctx.n_cu * 8));
    hipLaunchKernelGGL(free_image_build_kernel, dim3(grid), dim3(256), 0, s, (const double*)H->Jd, H->ld, nrows, (const int*)H->fi_map, H->Jf, b.ldf);
    BH_HIP(hipGetLastError());
    H->fi_epoch = P->mask_epoch; b.served += 1; *use = true;
    return BH_OK;
}

// Option free_image_eq, behind a free_image_prepare that said "use": Af[r * ldf + c'] = A[r * ldA + map[c']], zero where the map
// is -1, valid for this call (bh_free_image_plan.h: free_image_af_valid) or formed again by ONE launch enqueued behind the build
// or the move of Jf, which leaves fi_map current.  It is never moved (at most 64 rows: 2 MiB at n = 4096) and its launch is
// not priced into the policy.  free_image_build_kernel serves as it stands: it takes source, stride, row count, map,
// destination and ldf; its grid is min(mA, ...) >= 1 workgroups striding over the rows (row < mA); the 16-byte loads at an even
// map entry need an even source stride, and the three-kernel shape only exists with ldA == ld, a multiple of 16; the map has ldf
// entries, every one below n <= ldA or -1; the stores cover [0, ldf) of each of the mA rows of the mA * ldf allocation.
// *ok = false: the allocation failed — the call stays on the full image without an error.
static int32_t free_image_prepare_lineq(bh_hess* H, const bh_proj* P, bool* ok) {
    *ok = false;
    const FreeImageBook& b = H->fi;
    if (H->Af != nullptr && free_image_af_valid(H->af_epoch, H->fi_epoch, P->mask_epoch)) { *ok = true; return BH_OK; }
    const int64_t need = std::max<int64_t>(P->mA, 1) * b.ldf;
    if (H->Af_doubles < need) {
        if (H->Af) { (void)hipStreamSynchronize(g_ctx.stream); dev_free(H->Af); }
        H->Af = nullptr; H->Af_doubles = 0; H->af_epoch = 0;
        if (hipMalloc(reinterpret_cast<void**>(&H->Af), (size_t)need * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            H->Af = nullptr;
            return BH_OK;
        }
        H->Af_doubles = need;
    }
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(P->mA, (int64_t)g_ctx.n_cu * 8));
    hipLaunchKernelGGL(free_image_build_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const double*)P->Ad, P->ldA, P->mA, (const int*)H->fi_map,
                       H->Af, b.ldf);
    BH_HIP(hipGetLastError());
    H->af_epoch = H->fi_epoch;
    *ok = true;
    return BH_OK;
}

// ------------------------------------------------------------------------------------------
// projected_cg: the plan of one call (decided once), its run context, one launcher pair per shape
// ------------------------------------------------------------------------------------------
struct PcgPlan {
    PcgSelection sel{};             // the shape and its flags (bh_pcg_plan.h)
    bool gram = false;              // the loop streams G instead of J
    int max_iter = 0;
    int64_t nrows = 0;              // rows of the image the H*p launch streams
    int cfg = -1, grid = 1;         // row-stream geometry and its grid (fused shape on the compact image: of the compact width)
    int nblk = 1;                   // workgroups of the update / slab-reduction kernel
    int nch_v = 0;                  // chunks of v the projection kernel forms
    int nrv = 1;                    // who writes the r.v partials: the projection kernel (64 chunks per workgroup) or the update kernel
    int vv_off = 0;                 // v.v partials of the init launch, behind the r.v partials (nrv <= n_pad / 128)
    double* pbuf[2] = {nullptr, nullptr};    // ping-pong: p ...
    double* rvbuf[2] = {nullptr, nullptr};   // ... the r.v partials (fused shape)
    double* rbuf[2] = {nullptr, nullptr};    // ... r and the gamma partials, one per workgroup (box shape over RCCL)
    double* gbuf[2] = {nullptr, nullptr};
    LaunchAhead sched{};            // the launch-ahead schedule (bh_launch_ahead.h)
};

// What the launches of one call share.
struct PcgRun {
    bh_hess* H;
    bh_proj* P;
    CgWorkspace& c;
    hipStream_t s;
    CgArgs a{};
    PcgPlan plan;
    double* wp = nullptr;           // the caller's w
    double* hw = nullptr;
    // the loop's operands: the caller's, or their compact twins (free_image)
    const double *og = nullptr, *owl = nullptr, *owu = nullptr;
    double* ow = nullptr;
    const int* ofix = nullptr;
    int on = 0, onch = 0;
    int64_t old = 0;                // row stride of the image and of the slabs
    bool fi_use = false;            // the loop runs on the compact image of the free columns
    int expect_stop_at = 0;         // the launch expected to find the loop finished
};

// Geometry of the fused shape for a loop over `nch` chunks of `n_loop` variables.
static void pcg_fused_geometry(PcgPlan& p, int nch, int n_loop) {
    p.cfg = pick_config(nch);
    p.grid = grid_for(p.cfg, p.nrows);
    p.nblk = (nch + 15) / 16;
    p.nch_v = p.sel.gen_linv ? nch : (n_loop + 1) / 2;              // proj_apply_linv_kernel also keeps the padding of v at zero
    p.nrv = p.sel.fuse_gen ? (p.nch_v + 63) / 64 : p.nblk;
}

// Decides everything about the call from the handles and the options.  Launches and allocates nothing.
static PcgPlan pcg_make_plan(const bh_hess* H, const bh_proj* P, int max_iter, bool g_padded, bool hw_wanted, bool hw_free_part_ok,
                             double atol_f2b, bool allow_free_image) {
    const CgWorkspace& c = g_ctx.cg;
    const int64_t n = H->n, n_pad = H->ld;
    PcgPlan p;
    p.gram = H->form == BH_HESS_GRAM;
    p.max_iter = max_iter;
    const int rs_cfg = multi_panel(H) ? -1 : pick_config(H->nchunks);
    PcgSelectIn in{};
    in.mA = P->mA; in.gram_handle = p.gram;
    in.cg_fused = g_ctx.opt_cg_fused; in.gram_cg_fused = g_ctx.opt_gram_cg_fused; in.linv_refine = g_ctx.opt_linv_refine; in.fold_init = g_ctx.opt_fold_init;
    in.comm = comm_active(); in.peer_path = use_peer_path();
    in.reduced = P->reduced; in.tpart = P->tpart != nullptr; in.W = P->W != nullptr; in.M_valid = P->M_valid; in.lda_is_ld = P->ldA == H->ld;
    in.rs_cfg_ok = rs_cfg >= 0; in.cgp3_ok = rs_cfg >= 0 && cgp3_supported(rs_cfg); in.peer_blocks_fit = (H->nchunks + 15) / 16 <= kPeerBlkCap;
    in.iterates = max_iter >= 1; in.g_padded = g_padded; in.vectors_in_regs = (n + 1) / 2 <= 4 * CG_T;
    in.hw_wanted = hw_wanted; in.hw_free_part_ok = hw_wanted && hw_free_part_ok; in.atol_f2b_positive = atol_f2b > 0; in.allow_free_image = allow_free_image;
    in.free_image_eq = g_ctx.opt_free_image_eq;
    p.sel = pcg_select(in);
    const int batch = launch_batch_size(H);
    const bool rccl_path = comm_active() && !use_peer_path();
    // (an RCCL all-reduce cannot be gated from the device: every over-launched iteration pays for one.  With history on the handle
    // the first batch is the previous call's count exactly, so a repeated subproblem enqueues as many collectives as it has H*p
    // products; without history it stays small.)
    int cold = std::min(batch, rccl_path ? 1 : 2);
    p.sched.max_units = max_iter; p.sched.batch = batch; p.sched.off = 0; p.sched.look_first = true;
    p.sched.await_iter = false; p.sched.lock_step = true;           // (bh_launch_ahead.h: the lock-step rule)
    p.pbuf[0] = c.p; p.pbuf[1] = c.p2;
    if (p.sel.shape == PCG_FUSED) {
        p.nrows = p.gram ? H->ld : H->d + H->q_eff;                 // Gram form: the rows of the ld x ld image of G
        pcg_fused_geometry(p, H->nchunks, (int)n);
        p.vv_off = (int)(n_pad / 4);
        p.rvbuf[0] = c.rvpart; p.rvbuf[1] = c.rvpart + n_pad / 2;
        // S(j + 1) speaks for iteration j: either "stopped" (done) or "iter = j + 1, streaming".  Every iteration of the RCCL form
        // holds a collective; the peer-buffer exchange sits inside a kernel that a gated launch skips.
        p.sched.await_iter = true; p.sched.lock_step = p.sel.rccl_gen;
        cold = p.sel.rccl_gen ? 1 : std::min(batch, 2);
    } else if (p.sel.shape == PCG_RCCL_BOX) {
        p.nrows = H->d + H->q_eff;
        p.cfg = rs_cfg; p.grid = grid_for(rs_cfg, p.nrows); p.nblk = (H->nchunks + 15) / 16;
        p.rbuf[0] = c.r; p.rbuf[1] = c.r2;
        p.gbuf[0] = H->sq_partials + H->g_cap; p.gbuf[1] = H->sq_partials + 2 * (int64_t)H->g_cap;
        cold = 1;
    }
    p.sched.first = launch_ahead_first(H->last_n_hmul, cold);
    return p;
}

// The loop moves to the compact image of the free columns: compact operands (staging vectors of bh_minor_iterate: free during a
// bh_pcg, and read for the last time by step_bounds_kernel in front of a bh_minor_iterate's loop), no mask, the geometry of the
// compact width.  A wanted H*w is accumulated in slot order, its free part only (bh_pcg_plan.h: hw_free_part_ok).
static void pcg_use_free_image(PcgRun& r) {
    bh_hess* H = r.H; CgWorkspace& c = r.c;
    const FreeImageBook& b = H->fi;
    r.fi_use = true;
    r.og = c.x; r.owl = c.xlow; r.owu = c.xupp; r.ow = c.s;
    r.ofix = nullptr;
    if (r.hw != nullptr) r.hw = c.hwc;
    r.on = (int)b.nfree; r.onch = (int)(round_up(b.nfree, 16) / 2);
    r.old = b.ldf;                                            // (after a move the live width is smaller than the stride)
    pcg_fused_geometry(r.plan, r.onch, r.on);
    H->call_bytes = free_image_bytes(H);
    c.reroute_seq += 1;
}

// The projection kernels of the three-kernel equality iteration on the compact image (option free_image_eq): A is its compact
// image Af, mA x ldf; every live slot is free, so there is no mask; W, M, tw and tpart stay the constraint handle's own — they
// depend on the free set only.  In bounds: proj_left_mul_kernel reads ldf / 2 chunks of a row of Af and of the gathered g
// (ldf <= ld, the length of every workspace vector; both are zero from nfree on); proj_apply_linv_kernel touches the chunks below
// nch_pad = round_up(nfree, 16) / 2 <= ldf / 2 of Af and of the vectors, and the (nch_pad + 15) / 16 <= ld / 32 partial blocks
// of tpart the update kernel wrote.
// Hand-back (a non-finite g on a fixed variable: the gather raises `reroute`, bh_freeimg.hip.h): the stream and the update
// kernels of the call return at once, the projection kernels have no such gate and CgState may be a previous call's.  Every
// launch of a rerouted compact call writes workspace only — the gather: the compact g, w_l, w_u, w (and +0 into the caller's w on
// the fixed variables, an output the full loop writes in every entry); proj_left_mul_kernel: P->tw; proj_apply_linv_kernel: cg.v,
// cg.p and the r.v, v.v partials — and the loop on the full image that follows forms all of these again before it reads them
// (its own init launches; U(1) takes r from g and w = 0).
static void pcg_compact_proj_args(ProjArgs& pa, const PcgRun& r) {
    pa.A = r.H->Af; pa.ldA = r.old; pa.n = r.on; pa.nfix = 0; pa.fixrank = nullptr; pa.nch_pad = r.onch;
}

// ---- fused shape: S(1) | U(1) S(2) | U(2) S(3) | ...  The stream kernel of iteration j+1 is what detects "solved" after
// iteration j, so it is always enqueued together with U(j) (as a gated no-op if the loop ended in U(j)).
static int32_t pcg_fused_stream(PcgRun& r, int j) {             // H*p of iteration j (1-based), p_j formed on the fly
    bh_hess* H = r.H; CgWorkspace& c = r.c; const PcgPlan& p = r.plan;
    RowStreamArgs ra = rs_args(H, p.nrows, nullptr);
    ra.partials = H->partials;
    if (p.gram) { ra.J = H->G; ra.d_rows = p.nrows; ra.mu = 1.0; ra.partials = nullptr; ra.t_out = c.Hp; }     // H*p leaves as one vector
    if (r.fi_use) { ra.J = H->Jf; ra.ld = r.old; ra.nchunks = r.onch; }
    if (p.sel.fuse_gen) { ra.v = c.p; ra.negate = 0; }                            // used by j == 1 only: p_1 = -P(g), formed by the init kernels
    else { ra.v = r.og; ra.negate = 1; ra.negmask = r.ofix; }                    //                      p_1 = -mask(g), formed on the fly
    CgFuse& f = ra.cf;
    f.st = c.d_state; f.j = j; f.n = r.on; f.max_iter = p.max_iter; f.init_done = p.sel.gen_linv ? 2 : p.sel.fuse_gen ? 1 : 0; f.vv_off = p.vv_off;
    f.vvec = c.v; f.p_old = p.pbuf[(j - 1) & 1]; f.p_new = p.pbuf[j & 1];
    f.rvpart = p.rvbuf[(j - 1) & 1]; f.nrv = p.nrv;
    f.w = r.ow; f.wl = r.owl; f.wu = r.owu;
    if (r.fi_use) { f.reroute = c.d_reroute; f.reroute_seq = c.reroute_seq; }
    f.sqpart = H->sq_partials; f.gpart = H->sq_partials + H->g_cap;      // one entry per WORKGROUP (up to g_cap of them), not per chunk
    f.kappa2 = r.a.kappa2; f.atol_f2b = r.a.atol_f2b;
    f.trace = r.a.trace; f.trace_cap = r.a.trace_cap; f.mirror = r.a.mirror; f.tag = r.a.tag;
    int slot = -1;
    const bool expect_stop = j == r.expect_stop_at || j > p.max_iter || (r.expect_stop_at == 0 && j > 1);
    BH_TRY(profile_begin(H, j - 1, &slot));
    // a handle without history cannot predict its exit: its look-ahead launches (j > 1) take the no-prefetch symbol too, so
    // that launches which stop in their prologue never show up under the streaming kernel's name in a profile
    if (p.gram) launch_gram_cg(p.cfg, ra, p.grid, r.s, expect_stop);
    else launch_row_stream_cgp(p.cfg, ra, p.grid, r.s, expect_stop);
    if (slot >= 0) BH_HIP(hipEventRecord(H->ev[2 * slot + 1], r.s));
    return BH_OK;
}

static int32_t pcg_fused_update(PcgRun& r, int j) {
    bh_hess* H = r.H; bh_proj* P = r.P; CgWorkspace& c = r.c; const PcgPlan& p = r.plan; hipStream_t s = r.s;
    const int nblk = p.nblk, grid = p.grid;
    CgUpdArgs u{};
    u.st = c.d_state; u.j = j; u.partials = H->partials; u.ld = r.old; u.nchunks = r.onch; u.G = grid; u.Gs = grid; u.Gq = grid;
    u.sqpart = H->sq_partials; u.gpart = H->sq_partials + H->g_cap; u.rvpart_in = p.rvbuf[(j - 1) & 1]; u.rvpart_out = p.rvbuf[j & 1]; u.nrv = p.nrv;
    u.p = p.pbuf[j & 1]; u.w = r.ow; u.hw = r.hw; u.r = c.r; u.g = r.og; u.v = c.v; u.fixrank = r.ofix;
    if (r.fi_use) { u.map = H->fi_map; u.w_full = r.wp; u.reroute = c.d_reroute; u.reroute_seq = c.reroute_seq; }
    u.n = r.on; u.atol_neg = r.a.atol_neg; u.trace = r.a.trace; u.trace_cap = r.a.trace_cap; u.mirror = r.a.mirror; u.tag = r.a.tag;
    // Gram form: ONE "slab", the finished G p; the partials of dot(p, H*p) and of gamma stay one per workgroup of the G·v grid
    // (up to n_cu * kMaxBlocksPerCu of them: LaneBatch holds the first 512 in registers and folds the rest in index order)
    if (p.gram) { u.partials = c.Hp; u.Gs = 1; }
    if (!p.sel.fuse_gen) {
        if (p.sel.peer_fused) hipLaunchKernelGGL((cg_reduce_update_kernel<false, true>), dim3(nblk), dim3(256), 0, s, u, g_ctx.peer.args);
        else hipLaunchKernelGGL((cg_reduce_update_kernel<false, false>), dim3(nblk), dim3(256), 0, s, u, PeerArgs{});
        return BH_OK;
    }
    if (p.sel.rccl_gen) {
        // the collective is enqueued by the host between the slab reduction (which packs this rank's share of p'Hp behind the
        // vector) and the update kernel, which then sums ONE slab — the all-reduced H*p
        const int n_pad = r.a.n_pad;
        hipLaunchKernelGGL(reduce_partials_sq_kernel, dim3(nblk), dim3(256), 0, s, (const double*)H->partials, H->ld, H->nchunks, grid,
                           c.hpx, (const double*)H->sq_partials, n_pad, (const CgState*)c.d_state, j);
        BH_HIP(hipGetLastError());
        BH_TRY(allreduce_inplace(c.hpx, (int64_t)n_pad + 2, H));
        u.partials = c.hpx; u.Gs = 1; u.sqpart = c.hpx + n_pad; u.Gq = 1;
    }
    // (A, L and the vectors are replicated: past the exchange every rank forms the same partials of A_free r, the same v)
    u.A = P->Ad; u.ldA = P->ldA; u.mA = (int)P->mA; u.tpart = P->tpart; u.init_in_memory = p.sel.gen_linv ? 0 : 1;
    if (r.fi_use) { u.A = H->Af; u.ldA = r.old; }                 // (u.fixrank is NULL already: every live slot is free)
    if (r.fi_use) hipLaunchKernelGGL(cg_reduce_update_compact_kernel, dim3(nblk), dim3(256), 0, s, u);
    else if (p.sel.peer_fused) hipLaunchKernelGGL((cg_reduce_update_kernel<true, true>), dim3(nblk), dim3(256), 0, s, u, g_ctx.peer.args);
    else hipLaunchKernelGGL((cg_reduce_update_kernel<true, false>), dim3(nblk), dim3(256), 0, s, u, PeerArgs{});
    // y = (A_free A_free')^{-1} (A_free r): partial sums + the two triangular solves; then v = r_free - A_free'y and r.v
    ProjArgs pa = proj_args(P, c.d_state, true);
    pa.tpart = P->tpart; pa.tpart_nblk = nblk; pa.rvpart = p.rvbuf[j & 1]; pa.fused_j = j;
    if (p.sel.gen_linv) {
        pa.W = P->W; pa.nch_pad = r.onch; pa.Mgram = p.sel.linv_refine ? P->M : nullptr;
        if (r.fi_use) pcg_compact_proj_args(pa, r);
        hipLaunchKernelGGL((proj_apply_linv_kernel<false>), dim3((unsigned)p.nrv), dim3(256), 0, s, pa, (const double*)c.r, c.v);
        return BH_OK;
    }
    hipLaunchKernelGGL(trsv_small_kernel, dim3(1), dim3(256), 0, s, pa);
    hipLaunchKernelGGL((proj_left_mul_tr_kernel<true, 4>), dim3((p.nch_v + 63) / 64), dim3(256), 0, s, pa, (const double*)c.r, c.v);
    return BH_OK;
}

static int32_t pcg_fused_first(PcgRun& r) {
    bh_hess* H = r.H; bh_proj* P = r.P; CgWorkspace& c = r.c; const PcgPlan& p = r.plan; hipStream_t s = r.s;
    if (r.fi_use) {
        // g, w_l, w_u gathered through the slot -> column map by one launch in front of S(1); w is scattered into the caller's
        // buffer by the update kernel itself
        FreeGatherArgs ga{};
        ga.g = r.a.g; ga.wl = r.a.wl; ga.wu = r.a.wu; ga.fixrank = P->fixrank; ga.map = H->fi_map;
        ga.gc = c.x; ga.wlc = c.xlow; ga.wuc = c.xupp; ga.wc = c.s; ga.w = r.wp;
        ga.n = r.a.n; ga.n_pad = r.a.n_pad; ga.nfree = r.on;
        ga.reroute = c.d_reroute; ga.seq = c.reroute_seq; ga.mirror = r.a.mirror; ga.tag = r.a.tag;
        hipLaunchKernelGGL(free_image_gather_kernel, dim3((unsigned)((r.a.n_pad + 255) / 256)), dim3(256), 0, s, ga);
    }
    if (p.sel.gen_linv) {
        if (!P->linv_valid) {
            hipLaunchKernelGGL(tri_inv_small_kernel, dim3(1), dim3(256), 0, s, (const double*)P->Lr, (int)P->mA, P->W);
            P->linv_valid = true;
        }
        // :705-710 in two launches: tw = A_free mask(g); v = P(g), p_1 = -v and the partials of r.v, v.v.  r = g and w = 0 are
        // formed by the first update kernel, CgState is set by workgroup 0 of the first H*p launch (init_done = 2).
        // (on the compact image: of the gathered g, through Af — r.og is r.a.g otherwise)
        ProjArgs pa = proj_args(P, nullptr, true);
        if (r.fi_use) pcg_compact_proj_args(pa, r);
        hipLaunchKernelGGL(proj_left_mul_kernel, dim3((unsigned)P->mA), dim3(256), 0, s, pa, r.og);
        pa.tpart = P->tw; pa.tpart_nblk = 1; pa.rvpart = p.rvbuf[0]; pa.vvpart = p.rvbuf[0] + p.vv_off; pa.p_out = c.p;
        pa.W = P->W; pa.nch_pad = r.onch; pa.Mgram = p.sel.linv_refine ? P->M : nullptr; pa.fused_j = 0;
        hipLaunchKernelGGL((proj_apply_linv_kernel<true>), dim3((unsigned)p.nrv), dim3(256), 0, s, pa, r.og, c.v);
    } else if (p.sel.fuse_gen) {
        // :702-718 by the init kernels: r = g, w = 0, v = P(r), rtv, p_1 = -v (in c.p), tol_cg, CgState (stop_at = 0)
        hipLaunchKernelGGL((cg_init_kernel<false>), dim3(1), dim3(CG_T), 0, s, r.a);
        BH_TRY(launch_project(P, c.r, c.v, c.d_state));
        hipLaunchKernelGGL(cg_init_finish_kernel, dim3(1), dim3(CG_T), 0, s, r.a);
    }
    return pcg_fused_stream(r, 1);
}

static int32_t pcg_fused_unit(PcgRun& r, int index) {              // index = j - 1: U(j), S(j + 1)
    BH_TRY(pcg_fused_update(r, index + 1));
    BH_TRY(pcg_fused_stream(r, index + 2));                         // (iteration max_iter + 1 only ever runs its prologue: iter > max_iter)
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// ---- box constraints over RCCL: TWO kernels and the collective per iteration.  An ncclAllReduce is enqueued by
// the host, so it cannot sit inside the update kernel as the peer-buffer exchange does; instead the update of iteration j-1 moves
// into the prologue of the H*p launch of iteration j (row_stream_kernel<..., CGP = 3>: every workgroup redoes it for the whole
// 32 KiB vector, the owners of a chunk store it), and the slab reduction packs this rank's share of p'Hp behind the vector that
// goes through the all-reduce:  S(1) | R(1) AR(1) S(2) | R(2) AR(2) S(3) | ...
static int32_t pcg_rccl_box_stream(PcgRun& r, int j) {
    bh_hess* H = r.H; CgWorkspace& c = r.c; const PcgPlan& p = r.plan; const CgArgs& a = r.a;
    RowStreamArgs ra = rs_args(H, p.nrows, nullptr);
    ra.partials = H->partials;
    ra.v = a.g; ra.negate = 1; ra.negmask = a.fixrank;                // j == 1: p_1 = -mask(g), formed on the fly
    CgFuse& f = ra.cf;
    f.st = c.d_state; f.j = j; f.n = a.n; f.max_iter = p.max_iter; f.init_done = 0;
    f.p_old = p.pbuf[(j - 1) & 1]; f.p_new = p.pbuf[j & 1];
    f.r_old = p.rbuf[(j - 1) & 1]; f.r_new = p.rbuf[j & 1];
    f.gpart_in = p.gbuf[(j - 1) & 1]; f.gpart = p.gbuf[j & 1];
    f.w_rw = r.wp; f.w = r.wp; f.hw = r.hw; f.g = a.g; f.fixrank = a.fixrank;
    f.wl = a.wl; f.wu = a.wu;
    f.sqpart = H->sq_partials;
    f.Hp = c.hpx; f.sq_index = a.n_pad;
    f.kappa2 = a.kappa2; f.atol_f2b = a.atol_f2b; f.atol_neg = a.atol_neg;
    f.trace = a.trace; f.trace_cap = a.trace_cap; f.mirror = a.mirror; f.tag = a.tag;
    int slot = -1;
    BH_TRY(profile_begin(H, j - 1, &slot));
    launch_row_stream_cgp3(p.cfg, ra, p.grid, r.s);
    if (slot >= 0) BH_HIP(hipEventRecord(H->ev[2 * slot + 1], r.s));
    return BH_OK;
}

static int32_t pcg_rccl_box_unit(PcgRun& r, int index) {           // index = j - 1: R(j), AR(j), S(j + 1)
    bh_hess* H = r.H; CgWorkspace& c = r.c; const PcgPlan& p = r.plan;
    const int j = index + 1;
    hipLaunchKernelGGL(reduce_partials_sq_kernel, dim3(p.nblk), dim3(256), 0, r.s, (const double*)H->partials, H->ld, H->nchunks, p.grid,
                       c.hpx, (const double*)H->sq_partials, r.a.n_pad, (const CgState*)c.d_state, j);
    BH_HIP(hipGetLastError());
    BH_TRY(allreduce_inplace(c.hpx, (int64_t)r.a.n_pad + 2, H));
    return pcg_rccl_box_stream(r, j + 1);
}

// ---- separate-kernel shape.  Kernels of iterations past the exit see state->done and return at once.
static int32_t pcg_separate_first(PcgRun& r) {
    const bool box = r.P->mA == 0;
    // fold_init: no init kernel — the first H*p forms p0 = -mask(g) on the fly and the first step kernel does the initialisation
    // of :702-718 itself
    if (!r.plan.sel.fold_init && box) {
        hipLaunchKernelGGL((cg_init_kernel<true>), dim3(1), dim3(CG_T), 0, r.s, r.a);
    } else if (!r.plan.sel.fold_init) {
        hipLaunchKernelGGL((cg_init_kernel<false>), dim3(1), dim3(CG_T), 0, r.s, r.a);
        BH_TRY(launch_project(r.P, r.c.r, r.c.v, r.c.d_state));
        hipLaunchKernelGGL(cg_init_finish_kernel, dim3(1), dim3(CG_T), 0, r.s, r.a);
    }
    BH_HIP(hipGetLastError());
    return BH_OK;
}

static int32_t pcg_separate_unit(PcgRun& r, int index) {
    bh_hess* H = r.H; CgWorkspace& c = r.c;
    if (r.plan.sel.fold_init && index == 0) {
        // the state still holds the previous call's `done`: this launch is never a no-op, so it is not gated
        BH_TRY(launch_hmul(H, r.a.g, c.Hp, nullptr, index, true, r.a.fixrank));                    // :722 with p = -P(g)
        launch_cg_first_step(r.a, r.s);
        return BH_OK;
    }
    BH_TRY(launch_hmul(H, c.p, c.Hp, c.d_state, index));   // :722
    if (r.P->mA == 0) {
        launch_cg_step<0>(r.a, r.s);
    } else {
        launch_cg_step<1>(r.a, r.s);
        BH_TRY(launch_project(r.P, c.r, c.v, c.d_state));            // :741
        launch_cg_step<2>(r.a, r.s);
    }
    return BH_OK;
}

// What goes out in front of the loop (the init launches, S(1) of the shapes that have one) ...
static int32_t pcg_launch_first(PcgRun& r) {
    switch (r.plan.sel.shape) {
        case PCG_FUSED: return pcg_fused_first(r);
        case PCG_RCCL_BOX: return pcg_rccl_box_stream(r, 1);
        default: return pcg_separate_first(r);
    }
}
// ... and launch unit `index` of the schedule: iteration index + 1.
static int32_t pcg_launch_unit(PcgRun& r, int index) {
    switch (r.plan.sel.shape) {
        case PCG_FUSED: return pcg_fused_unit(r, index);
        case PCG_RCCL_BOX: return pcg_rccl_box_unit(r, index);
        default: return pcg_separate_unit(r, index);
    }
}

// Launches the whole projected_cg on device vectors and returns once the host has seen the loop finish (the stream may
// still hold over-launched no-op kernels).  gp/wlp/wup: n doubles readable in 16-byte chunks; wp: output.
// Which shape runs: pcg_make_plan (the rule: bh_pcg_plan.h); the launch schedule and its lock-step rule: bh_launch_ahead.h.
static int32_t pcg_run(bh_hess* H, bh_proj* P, const double* gp, const double* wlp, const double* wup, double* wp, bool w_in_ws,
                       double kappa2, double atol_negcurv, double atol_f2b, int64_t trace_cap, PcgFin* fin_out, double* hw = nullptr,
                       bool g_pad_zeroed = false /* the staged copy of g arrived with its padding already zero */,
                       bool allow_free_image = true /* false: the compact loop handed this call back (bh_freeimg.hip.h) */,
                       bool hw_free_part_ok = false /* nothing reads hw on the fixed variables (options free_image_minor, free_image_chain) */) {
    const int64_t n = H->n, n_pad = H->ld;
    const int64_t max_iter64 = 2 * (n - P->mA - P->nfix);   // src/basic_tralcnlss.jl:714
    if (max_iter64 < 0) return fail(BH_ERR_PRECONDITION, "n - mA - count(fixvars) < 0");
    if (max_iter64 >= 0xfffff) return fail(BH_ERR_UNSUPPORTED, "2*(n - mA - count(fixvars)) exceeds the 20-bit iteration counters of the progress word");
    CgWorkspace& c = g_ctx.cg;
    H->ev_pending.clear();
    g_ctx.notes.cg_loop_begins(hw != nullptr);
    H->call_bytes = hmul_bytes(H);

    PcgRun run{H, P, c, g_ctx.stream};
    CgArgs& a = run.a;
    a.st = c.d_state; a.w = wp; a.r = c.r; a.v = c.v; a.p = c.p; a.Hp = c.Hp; a.g = gp; a.wl = wlp; a.wu = wup;
    a.fixrank = P->nfix > 0 ? P->fixrank : nullptr;
    a.n = (int)n; a.n_pad = (int)n_pad; a.w_in_ws = w_in_ws ? 1 : 0; a.max_iter = (int)max_iter64; a.kappa2 = kappa2; a.atol_neg = atol_negcurv; a.atol_f2b = atol_f2b;
    a.trace = trace_cap > 0 ? c.d_trace : nullptr; a.trace_cap = (int)std::min<int64_t>(trace_cap, 0x7fffffff);
    a.mirror = c.d_mirror; a.tag = next_mirror_tag(c);
    a.hw = hw;
    run.wp = wp; run.hw = hw;
    run.og = gp; run.owl = wlp; run.owu = wup; run.ow = wp; run.ofix = a.fixrank;
    run.on = (int)n; run.onch = H->nchunks; run.old = H->ld;
    run.expect_stop_at = H->last_n_hmul > 0 ? H->last_n_hmul + 1 : 0;

    run.plan = pcg_make_plan(H, P, a.max_iter, gp == c.g || n == n_pad, hw != nullptr, hw_free_part_ok, atol_f2b, allow_free_image);
    const PcgSelection& sel = run.plan.sel;
    if (sel.shape != PCG_SEPARATE) BH_TRY(hess_ready(H));
    if (sel.shape == PCG_FUSED && run.plan.gram) BH_TRY(ensure_gram(H));      // G rebuilt first when stale, on the same stream
    H->stats.cg_kernels = sel.cg_kernels;
    if (sel.shape != PCG_SEPARATE || sel.fold_init) BH_TRY(zero_staged_g_padding(c, gp, n, n_pad, g_pad_zeroed));
    bool fi_use = false, fi_earns = false;
    if (sel.free_image_eligible) BH_TRY(free_image_prepare(H, P, &fi_use, &fi_earns));      // (option free_image)
    if (fi_use && P->mA > 0) {                                                              // (option free_image_eq)
        BH_TRY(free_image_prepare_lineq(H, P, &fi_use));
        if (!fi_use) H->fi.served -= 1;
    }
    if (fi_use) pcg_use_free_image(run);

    BH_TRY(pcg_launch_first(run));
    // Progress comes back through one host-mapped 8-byte word the kernels store to (no copy kernels, no events).
    MirrorWord mw{};
    BH_TRY(launch_ahead(run.plan.sched, [&](int index) { return pcg_launch_unit(run, index); },
                        [&](int n_hmul_target, int iter_target, MirrorWord* m) { return wait_mirror(c, a.tag, n_hmul_target, m, iter_target); }, &mw));
    if (!mw.done) return fail(BH_ERR_HIP, "internal: CG loop did not terminate");
    if (fi_use && mw.status == kCgReroute) {
        // a non-finite g on a fixed variable: the full image decides (every compact launch still queued returns at once)
        H->fi.served -= 1;
        return pcg_run(H, P, gp, wlp, wup, wp, w_in_ws, kappa2, atol_negcurv, atol_f2b, trace_cap, fin_out, hw, g_pad_zeroed, false);
    }
    if (fi_earns) H->fi.credit += free_image_saving(mw.n_hmul, P->nfix, n);
    // (the fused shape with its exchange, if any, inside a kernel; over RCCL over-launched collectives are still in flight)
    const bool results_final = sel.shape == PCG_FUSED && !sel.rccl_gen &&
                               (mw.status == BH_CG_SOLVED || mw.status == BH_CG_MAX_ITER_REACHED || mw.status == BH_CG_NONE);
    pcg_fin_fill(fin_out, mw, a.tag, results_final);
    fin_out->compact = fi_use;
    // exchanges that really ran (one per executed H*p): how many update kernels were ENQUEUED past the exit depends on when
    // this rank polled its progress word, and those exchange nothing
    if (sel.peer_fused) H->stats.n_allreduce += mw.n_hmul;
    return BH_OK;
}

// The tie log the final publish_state left next to the progress word.  The words are stored before the progress word by the
// same thread, but only a drained stream makes that an ordering guarantee.
static void read_tie_words(bh_hess* H) {
    const unsigned long long tw = g_ctx.cg.h_mirror[1], mb = g_ctx.cg.h_mirror[2];
    H->margin_kind = (int)((tw >> 48) & 0xf); H->tie_flags = (int)((tw >> 40) & 0xff);
    H->tie_first = (int)((tw >> 20) & 0xfffff); H->margin_at = (int)(tw & 0xfffff);
    memcpy(&H->min_margin, &mb, sizeof(double));
    H->tie_read = true;
}

// Bookkeeping of one finished projected_cg (normally after the caller's hipStreamSynchronize; `drained` = false when the
// device-pointer entry point returned on results_final without draining).
static int32_t pcg_finish(bh_hess* H, const PcgFin& fin, bool drained = true) {
    if (!fin.done) return fail(BH_ERR_HIP, "internal: CG loop did not terminate");
    H->stats.n_pcg += 1;
    H->last_n_hmul = fin.n_hmul;
    H->tie_tag = fin.tag;
    H->tie_read = false;
    if (drained) read_tie_words(H);     // else: read on demand (bh_pcg_tie_info drains first)
    H->stats.n_hmul += fin.n_hmul;
    H->stats.n_cg_iter += fin.iter - 1;
    H->stats.n_proj += fin.iter;
    if (!H->ev_pending.empty()) {
        for (size_t i = 0; i < H->ev_pending.size(); ++i) {
            if (H->ev_pending[i] >= fin.n_hmul) continue;         // an over-launched no-op: not an H*p
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, H->ev[2 * i], H->ev[2 * i + 1]) == hipSuccess) {
                H->stats.hmul_ms += ms;
                H->stats.hmul_timed += 1;
                H->timed_bytes += H->call_bytes;
                H->timed_n += 1;
            }
        }
        if (H->timed_n > 0) H->stats.bytes_per_hmul = H->timed_bytes / (double)H->timed_n;
        H->ev_pending.clear();
    }
    return BH_OK;
}

static int32_t pcg_impl(bh_hess* H, bh_proj* P, const double* g_minor, const double* w_l, const double* w_u, double kappa2,
                        double atol_negcurv, double atol_f2b, double* w_out, int32_t* status, int32_t* iters, double* trace,
                        int64_t trace_cap, int32_t* n_hmul_out, bool dev) {
    BH_REQUIRE_INIT();
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    BH_TRY(check_proj_ready(P));
    if (!g_minor || !w_l || !w_u || !w_out) return fail(BH_ERR_INVALID_ARG, "NULL vector argument");
    if (H->n != P->n) return fail(BH_ERR_SHAPE, "H.n != lincons.n");
    if (trace == nullptr) trace_cap = 0;
    if (trace_cap < 0) return fail(BH_ERR_INVALID_ARG, "negative trace_cap");
    const int64_t n = H->n;
    BH_TRY(ensure_cg_workspace(H->ld, trace_cap));
    CgWorkspace& c = g_ctx.cg;
    // Device callers with even n and 16-byte aligned buffers hand over memory the kernels can use in place (16-byte chunk
    // loads stay in bounds); host callers, odd n and unaligned pointers go through the zero-padded workspace.
    auto aligned16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; };
    // With a communicator the choice must not depend on this rank's pointers: in place only when n == ld, where the CG iteration
    // shape chosen in pcg_run (two-kernel / three-kernel, which exchange different payloads and round pHp differently) is the
    // same whether a rank works in place or through the workspace; below ld every rank stages.
    const bool in_place = dev && (n % 2 == 0) && aligned16(g_minor) && aligned16(w_l) && aligned16(w_u) && aligned16(w_out) &&
                          (!comm_active() || n == H->ld);
    const double *gp = g_minor, *wlp = w_l, *wup = w_u;
    double* wp = w_out;
    if (!in_place) {
        if (!dev) {
            BH_TRY(stage_vecs(c.g, {g_minor, w_l, w_u}, n, c.n_pad));      // c.g, c.wl, c.wu are consecutive
        } else {
            BH_TRY(stage_vec(c.g, g_minor, n, true));
            BH_TRY(stage_vec(c.wl, w_l, n, true));
            BH_TRY(stage_vec(c.wu, w_u, n, true));
        }
        gp = c.g; wlp = c.wl; wup = c.wu; wp = c.w;
    }
    PcgFin fin{};
    BH_TRY(pcg_run(H, P, gp, wlp, wup, wp, !in_place, kappa2, atol_negcurv, atol_f2b, trace_cap, &fin, nullptr, !dev));
    if (!in_place) BH_TRY(fetch_vec(w_out, c.w, n, dev));
    if (trace_cap > 0) count_d2h((size_t)4 * trace_cap * sizeof(double));
    if (trace_cap > 0) note_dma();
    if (trace_cap > 0) BH_HIP(hipMemcpyAsync(trace, c.d_trace, (size_t)4 * trace_cap * sizeof(double), hipMemcpyDeviceToHost, g_ctx.stream));
    // The final hipStreamSynchronize costs ~10 us (measured: 650 -> 640 us per config-3 subproblem).  It is skipped when nothing
    // can still be written: device vectors used in place (no staged result to fetch), no trace, and the loop stopped in the
    // prologue of an H*p launch (PcgFin::results_final) — w was complete before that launch began.  Otherwise the stream is
    // drained as before (option "final_sync" = 1 forces it).
    const bool drain = g_ctx.opt_final_sync || !(in_place && trace_cap == 0 && fin.results_final);
    if (drain) BH_TRY(sync_flush());      // drains the over-launched no-op kernels; orders w for any consumer
    BH_TRY(pcg_finish(H, fin, drain));
    if (status) *status = fin.status;
    if (iters) *iters = fin.iter;
    if (n_hmul_out) *n_hmul_out = fin.n_hmul;
    return BH_OK;
}

int32_t bh_pcg(bh_hess* H, bh_proj* P, const double* g_minor, const double* w_l, const double* w_u, double kappa2,
               double atol_negcurv, double atol_f2b, double* w_out, int32_t* status, int32_t* iters, double* trace,
               int64_t trace_cap, int32_t* n_hmul) {
    return pcg_impl(H, P, g_minor, w_l, w_u, kappa2, atol_negcurv, atol_f2b, w_out, status, iters, trace, trace_cap, n_hmul, false);
}

int32_t bh_pcg_tie_info(const bh_hess* H, int32_t* tie_flags, int32_t* first_tie_hmul, double* min_margin, int32_t* min_margin_kind,
                        int32_t* min_margin_hmul) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    if (!H->tie_read) {
        // the call returned without draining the stream: do it now, and make sure no later call has overwritten the words
        bh_hess* Hm = const_cast<bh_hess*>(H);
        if (g_ctx.init && g_ctx.stream) BH_HIP(hipStreamSynchronize(g_ctx.stream));
        if ((unsigned)((g_ctx.cg.h_mirror[0] >> 48) & 0xffffu) != (H->tie_tag & 0xffffu))
            return fail(BH_ERR_PRECONDITION, "bh_pcg_tie_info: another projected_cg has run since this handle's last one (ask right after the call)");
        read_tie_words(Hm);
    }
    if (tie_flags) *tie_flags = H->tie_flags;
    if (first_tie_hmul) *first_tie_hmul = H->tie_first;
    if (min_margin) *min_margin = H->min_margin;
    if (min_margin_kind) *min_margin_kind = H->margin_kind;
    if (min_margin_hmul) *min_margin_hmul = H->margin_at;
    return BH_OK;
}

int32_t bh_pcg_dev(bh_hess* H, bh_proj* P, const double* g_minor_dev, const double* w_l_dev, const double* w_u_dev, double kappa2,
                   double atol_negcurv, double atol_f2b, double* w_out_dev, int32_t* status, int32_t* iters, double* trace,
                   int64_t trace_cap, int32_t* n_hmul) {
    return pcg_impl(H, P, g_minor_dev, w_l_dev, w_u_dev, kappa2, atol_negcurv, atol_f2b, w_out_dev, status, iters, trace, trace_cap,
                    n_hmul, true);
}


// linesearch(g_model, H, w, w_l, w_u, fix_bounds) — src/basic_tralcnlss.jl:766-791 (device part shared with bh_minor_iterate):
// wHw = vthv(H, w_pad) -> H->scalar (all-reduced), then alpha -> c.scalars[0]; optionally w_pad *= alpha.
// hw: H*w accumulated by the CG loop (then w'Hw = w.hw, no sweep over J), or NULL (then wHw = vthv(H, w): one J*v pass).
static int32_t launch_linesearch(bh_hess* H, bh_proj* P, const double* g_dev, double* w_pad, const double* wl_dev, const double* wu_dev,
                                 bool scale_w, double* hw = nullptr, double* alpha_dst = nullptr /* default: c.scalars[0] */) {
    CgWorkspace& c = g_ctx.cg;
    if (hw == nullptr) {
        BH_TRY(launch_quad(H, w_pad));
    }
    hipLaunchKernelGGL(linesearch_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, g_dev, w_pad, wl_dev, wu_dev,
                       P->nfix > 0 ? P->fixrank : (const int*)nullptr, (const double*)H->scalar, hw, (int)H->n, scale_w ? 1 : 0,
                       alpha_dst ? alpha_dst : c.scalars);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

static int32_t linesearch_impl(bh_hess* H, bh_proj* P, const double* g_model, const double* w, const double* w_l, const double* w_u,
                               double* alpha_out, bool dev) {
    BH_REQUIRE_INIT();
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    BH_TRY(check_proj_ready(P));
    if (!g_model || !w || !w_l || !w_u || !alpha_out) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    if (H->n != P->n) return fail(BH_ERR_SHAPE, "H.n != lincons.n");
    const int64_t n = H->n;
    BH_TRY(ensure_cg_workspace(H->ld, 0));
    CgWorkspace& c = g_ctx.cg;
    if (dev) {
        // the line-search kernel reads its vectors element by element (used where they lie); only vthv(H, w) needs w in whole
        // 16-byte chunks up to the padded length
        const double* wp = c.w;
        if (n == H->ld && (reinterpret_cast<uintptr_t>(w) & 15u) == 0) wp = w;
        else {
            BH_HIP(hipMemsetAsync(c.w, 0, (size_t)H->ld * sizeof(double), g_ctx.stream));
            BH_TRY(stage_vec(c.w, w, n, true));
        }
        BH_TRY(mbox_ensure());
        BH_TRY(launch_linesearch(H, P, g_model, const_cast<double*>(wp), w_l, w_u, false, nullptr, mbox_dev<double>(kMbScal)));
        BH_TRY(mbox_seal_and_wait(sizeof(double)));
        *alpha_out = *mbox_host<double>(kMbScal);
        return BH_OK;
    }
    BH_HIP(hipMemsetAsync(c.w, 0, (size_t)H->ld * sizeof(double), g_ctx.stream));
    BH_TRY(stage_vec(c.w, w, n, false));
    BH_TRY(stage_vec(c.g, g_model, n, false));
    BH_TRY(stage_vec(c.wl, w_l, n, false));
    BH_TRY(stage_vec(c.wu, w_u, n, false));
    BH_TRY(launch_linesearch(H, P, c.g, c.w, c.wl, c.wu, false));
    BH_TRY(fetch_vec(alpha_out, c.scalars, 1, false));
    BH_TRY(sync_flush());
    return BH_OK;
}
int32_t bh_linesearch(bh_hess* H, bh_proj* P, const double* g_model, const double* w, const double* w_l, const double* w_u,
                      double* alpha_out) {
    return linesearch_impl(H, P, g_model, w, w_l, w_u, alpha_out, false);
}
int32_t bh_linesearch_dev(bh_hess* H, bh_proj* P, const double* g_model_dev, const double* w_dev, const double* w_l_dev,
                          const double* w_u_dev, double* alpha_out) {
    return linesearch_impl(H, P, g_model_dev, w_dev, w_l_dev, w_u_dev, alpha_out, true);
}

// minor_iterate(x, s, g_model, H, lincons, delta, kappa2) — src/basic_tralcnlss.jl:649-675, entirely on the device:
// step bounds (:660-665), projected_cg (:667), linesearch + scaling (:669-672).
static int32_t minor_iterate_impl(bh_hess* H, bh_proj* P, const double* x, const double* s_vec, const double* g_model, const double* xlow,
                                  const double* xupp, double delta, double kappa2, double atol_negcurv, double atol_f2b, double* w_out,
                                  int32_t* status, int32_t* iters, int32_t* n_hmul_out, double* alpha_out, bool dev) {
    BH_REQUIRE_INIT();
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL bh_hess");
    BH_TRY(check_proj_ready(P));
    if (!x || !s_vec || !g_model || !xlow || !xupp || !w_out) return fail(BH_ERR_INVALID_ARG, "NULL vector argument");
    if (H->n != P->n) return fail(BH_ERR_SHAPE, "H.n != lincons.n");
    const int64_t n = H->n;
    BH_TRY(ensure_cg_workspace(H->ld, 0));
    CgWorkspace& c = g_ctx.cg;
    // device callers: x, s and the bounds are only read element-wise (no staging); g_minor is copied device-to-device into
    // the zero-padded workspace vector the CG kernels read in 16-byte chunks
    const double *xp = x, *sp = s_vec, *lop = xlow, *upp = xupp;
    const double* gp = c.g;
    double* wp = c.w;
    // ls_from_cg: the CG loop accumulates H*w next to w, so linesearch's w'Hw (vthv(H,w), :775) costs a dot product
    // instead of another sweep over J (-0.3 ms per minor iterate at config 3); mathematically identical, rounding ~1e-15.
    double* hw = g_ctx.opt_ls_from_cg ? c.hw : nullptr;
    if (!dev) {
        g_ctx.notes.compact_operands_overwritten();
        BH_TRY(stage_vecs(c.s, {s_vec, x, xlow, xupp, g_model}, n, c.n_pad));      // c.s, c.x, c.xlow, c.xupp, c.g are consecutive
        xp = c.x; sp = c.s; lop = c.xlow; upp = c.xupp;
        BH_TRY(mbox_ensure());
    } else {
        // device callers: x, s and the bounds are only read element-wise; g_minor and w are used where they lie when the
        // kernels' 16-byte chunk accesses stay inside them (else through the zero-padded workspace)
        BH_TRY(device_operand(&gp, c.g, g_model, n, H->ld));
        // (w: the two-kernel iteration reads and writes whole 16-byte chunks up to the padded length)
        const bool w_ok = (n == H->ld) && (reinterpret_cast<uintptr_t>(w_out) & 15u) == 0;
        if (w_ok) wp = w_out;
        BH_TRY(mbox_ensure());
    }
    const int grid = std::max(1, std::min((int)((n + 255) / 256), 1024));
    hipLaunchKernelGGL(step_bounds_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, xp, sp, lop, upp,
                       P->nfix > 0 ? P->fixrank : (const int*)nullptr, delta, (int)n, c.wl, c.wu);
    PcgFin fin{};
    // free_image_minor: with step_from_cg off the line search's w'Hw is the only consumer of hw, and w is zero on the fixed
    // variables — the free part of H*w is enough, so the loop may run on the compact image
    // free_image_chain: with step_from_cg on, bh_step_accumulate_dev takes the free part too (the fixed part of g_minor is read by
    // nothing inside an inner step, and the model value is carried: bh_step_chain_plan.h)
    const bool chain = g_ctx.opt_free_image_chain == 1 && g_ctx.opt_step_from_cg == 1;
    const bool hw_free_part_ok = hw != nullptr && ((g_ctx.opt_free_image_minor == 1 && g_ctx.opt_step_from_cg == 0) || chain);
    BH_TRY(pcg_run(H, P, gp, c.wl, c.wu, wp, wp == c.w, kappa2, atol_negcurv, atol_f2b, 0, &fin, hw, !dev, true, hw_free_part_ok));
    double alpha = std::nan("");
    const bool do_ls = fin.status != BH_CG_NEGATIVE_CURVATURE;       // :669
    // alpha is written by the line search straight into the host-mapped mailbox (no DMA of its own)
    if (do_ls && fin.compact && hw_free_part_ok && chain) {
        // ... and hwc scaled with w, for the accumulate that follows
        hipLaunchKernelGGL(free_image_linesearch_scale_hw_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, (const double*)c.x, c.s, (const double*)c.xlow,
                           (const double*)c.xupp, c.hwc, (const int*)H->fi_map, wp, (int)H->fi.nfree, mbox_dev<double>(kMbScal));
        BH_HIP(hipGetLastError());
    } else if (do_ls && fin.compact && hw_free_part_ok) {
        // the compact operands the loop left (pcg_use_free_image): g, w, w_l, w_u in slot order and the free part of H*w
        hipLaunchKernelGGL(free_image_linesearch_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, (const double*)c.x, c.s, (const double*)c.xlow,
                           (const double*)c.xupp, (const double*)c.hwc, (const int*)H->fi_map, wp, (int)H->fi.nfree, mbox_dev<double>(kMbScal));
        BH_HIP(hipGetLastError());
    } else if (do_ls) {
        BH_TRY(launch_linesearch(H, P, gp, wp, c.wl, c.wu, true, hw, mbox_dev<double>(kMbScal)));
    }
    if (wp == c.w) BH_TRY(fetch_vec(w_out, c.w, n, dev));
    if (!dev) {
        BH_TRY(sync_flush());                               // w comes back through the pinned arena: the stream is drained
        if (do_ls) { count_d2h(sizeof(double)); alpha = *mbox_host<double>(kMbScal); }
    } else if (do_ls) {
        BH_TRY(mbox_seal_and_wait(sizeof(double)));        // alpha: written by the line search straight into the mailbox
        alpha = *mbox_host<double>(kMbScal);
    } else {
        BH_TRY(finish_device_call());
    }
    BH_TRY(pcg_finish(H, fin, !dev));
    // cg.hw (or, after a loop on the compact image in the chain, cg.hwc) now holds H*w for the w just delivered, scaled with it by
    // the line search: bh_step_accumulate_dev may use it
    g_ctx.notes.minor_iterate_done(H, w_out, g_model, dev, hw != nullptr, fin.compact, chain, H->fi.nfree);
    if (status) *status = fin.status;
    if (iters) *iters = fin.iter;
    if (n_hmul_out) *n_hmul_out = fin.n_hmul;
    if (alpha_out) *alpha_out = alpha;
    return BH_OK;
}

int32_t bh_minor_iterate(bh_hess* H, bh_proj* P, const double* x, const double* s_vec, const double* g_model, const double* xlow,
                         const double* xupp, double delta, double kappa2, double atol_negcurv, double atol_f2b, double* w_out,
                         int32_t* status, int32_t* iters, int32_t* n_hmul_out, double* alpha_out) {
    return minor_iterate_impl(H, P, x, s_vec, g_model, xlow, xupp, delta, kappa2, atol_negcurv, atol_f2b, w_out, status, iters, n_hmul_out,
                              alpha_out, false);
}
int32_t bh_minor_iterate_dev(bh_hess* H, bh_proj* P, const double* x_dev, const double* s_dev, const double* g_model_dev,
                             const double* xlow_dev, const double* xupp_dev, double delta, double kappa2, double atol_negcurv,
                             double atol_f2b, double* w_out_dev, int32_t* status, int32_t* iters, int32_t* n_hmul_out, double* alpha_out) {
    return minor_iterate_impl(H, P, x_dev, s_dev, g_model_dev, xlow_dev, xupp_dev, delta, kappa2, atol_negcurv, atol_f2b, w_out_dev, status,
                              iters, n_hmul_out, alpha_out, true);
}

// g = Jx'*rx + Cx'*y_bar — src/basic_tralcnlss.jl:45,:74 (r = this rank's d rows; C'y_bar added by rank 0; all-reduced).
static int32_t adopt_device_mask(bh_proj* P, uint64_t* fix_chunks_out, int* info_out, int* counts_out = nullptr);

static int32_t grad_impl(bh_hess* H, const double* r, const double* ybar, double* g_out, bool dev) {
    BH_REQUIRE_INIT();
    if (!H || (!r && H->d > 0) || (!ybar && H->q > 0) || !g_out) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    BH_TRY(stage_vec(H->upad, r, H->d, dev));
    BH_TRY(stage_vec(H->upad + H->d, ybar, H->q, false));         // q multipliers: always a (tiny) host vector
    BH_TRY(launch_jtv(H, H->upad, H->zpad, true));
    BH_TRY(fetch_vec(g_out, H->zpad, H->n, dev));
    BH_TRY(sync_flush());          // (ybar is a host vector in both forms: the pinned arena has traffic in flight)
    H->stats.n_jtv += 1;
    return BH_OK;
}
int32_t bh_grad(bh_hess* H, const double* r, const double* ybar, double* g_out) { return grad_impl(H, r, ybar, g_out, false); }
int32_t bh_grad_dev(bh_hess* H, const double* r_dev, const double* ybar, double* g_out_dev) { return grad_impl(H, r_dev, ybar, g_out_dev, true); }

// dot(rx, rx) of mx = 0.5*dot(rx,rx) + ... — src/basic_tralcnlss.jl:44 (new_point), :58 (evaluate_al): r = this rank's rows of
// the residual; the partial sums of squares are all-reduced (rank order), so every rank gets the same bits.
int32_t bh_resid_sqnorm(const double* r, int64_t d, double* out) {
    BH_REQUIRE_INIT();
    if (d < 0 || (!r && d > 0) || !out) return fail(BH_ERR_INVALID_ARG, "bad argument");
    if (d + 4 > g_ctx.rbuf_cap) {
        dev_free(g_ctx.rbuf);
        g_ctx.rbuf = nullptr; g_ctx.rbuf_cap = 0;
        BH_TRY(dev_alloc(&g_ctx.rbuf, d + 4));
        g_ctx.rbuf_cap = d + 4;
    }
    double* acc = g_ctx.rbuf + round_up(d, 2);   // 2 doubles, 16-byte aligned: the exchange works on whole chunks
    BH_TRY(stage_vec(g_ctx.rbuf, r, d, false));
    hipLaunchKernelGGL(weighted_sqsum_kernel, dim3(1), dim3(1024), 0, g_ctx.stream, (const double*)g_ctx.rbuf, d, d, 1.0, acc);
    BH_HIP(hipGetLastError());
    BH_TRY(allreduce_inplace(acc, 1, nullptr));
    BH_TRY(fetch_vec(out, acc, 1, false));
    BH_TRY(sync_flush());
    return BH_OK;
}

// g_minor = H*s + g — src/basic_tralcnlss.jl:412,:437.
static int32_t hmul_add_impl(bh_hess* H, const double* s_vec, const double* g, double* out_n, bool dev, const double* w_add = nullptr,
                             double* s_inout = nullptr) {
    BH_REQUIRE_INIT();
    if (!H || !s_vec || !g || !out_n) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    const int64_t n = H->n;
    BH_TRY(ensure_cg_workspace(H->ld, 0));
    const int grid = std::max(1, std::min((int)((n + 255) / 256), 1024));
    if (w_add != nullptr)      // s .+= w (:436) on the caller's device vector, then H*s + g
        hipLaunchKernelGGL(vec_add_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const double*)s_inout, w_add, s_inout, (int)n);
    const double* sp = H->vpad;
    if (dev) BH_TRY(device_operand(&sp, H->vpad, s_vec, n, H->ld));
    else BH_TRY(stage_vec(H->vpad, s_vec, n, false));
    BH_TRY(launch_hmul(H, sp, H->zpad, nullptr, -1));
    if (dev) {
        hipLaunchKernelGGL(vec_add_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const double*)H->zpad, g, out_n, (int)n);
        BH_HIP(hipGetLastError());
    } else {
        CgWorkspace& c = g_ctx.cg;
        BH_TRY(stage_vec(c.g, g, n, false));
        hipLaunchKernelGGL(vec_add_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const double*)H->zpad, (const double*)c.g, H->zpad, (int)n);
        BH_TRY(fetch_vec(out_n, H->zpad, n, false));
    }
    BH_TRY(dev ? finish_device_call() : sync_flush());
    H->stats.n_hmul += 1;
    g_ctx.notes.gminor_written(H, s_vec, g, out_n, dev);
    return BH_OK;
}
int32_t bh_hmul_add(bh_hess* H, const double* s_vec, const double* g, double* out_n) { return hmul_add_impl(H, s_vec, g, out_n, false); }
int32_t bh_hmul_add_dev(bh_hess* H, const double* s_dev, const double* g_dev, double* out_n_dev) {
    return hmul_add_impl(H, s_dev, g_dev, out_n_dev, true);
}
// s .+= w ; g_minor = H*s + g — src/basic_tralcnlss.jl:436-437, on device vectors (s is updated in place).
int32_t bh_step_accumulate_dev(bh_hess* H, double* s_dev, const double* w_dev, const double* g_dev, double* g_minor_out_dev) {
    if (!w_dev || !s_dev) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    // The inner step's pattern (src/basic_tralcnlss.jl:434-437): g_minor_out holds H*s + g, it was the g_model of the
    // bh_minor_iterate_dev that has just produced w, and that call's CG loop accumulated H*w.  Then H*(s + w) + g = g_minor + H*w:
    // two n-vector kernels instead of a sweep over J.  Recognised by the three pointers; anything else recomputes H*s + g.
    //
    // Option free_image_chain: behind a minor iterate whose loop ran on the compact image the H*w at hand is its free part, in slot
    // order (cg.hwc).  Then only the free entries of g_minor are brought up to date — AFTER SUCH A CALL g_minor_out HOLDS H*s + g ON
    // THE FREE VARIABLES ONLY, its entries on the fixed variables keep the value they had (nothing inside an inner step reads them:
    // the next CG loop and the reduced-gradient norm mask them, and the active set only grows while one J lives) — and the model
    // value q(s) = g.s + s'Hs / 2, which bh_model_reduction_dev could no longer take from such a g_minor, is carried along by
    // q(s + w) = q(s) + w.g_minor + w'Hw / 2 over the free slots.  Which path runs: step_acc_select (bh_step_chain_plan.h).
    const bool ok = g_ctx.init && H && g_dev && g_minor_out_dev;
    CgWorkspace& c = g_ctx.cg;
    const bool compact_live = ok && c.hwc != nullptr && H->fi.present && H->fi_map != nullptr;
    StepAccIn in = g_ctx.notes.accumulate_begins(H, w_dev, g_minor_out_dev, s_dev, g_dev, ok, c.hw != nullptr, compact_live, ok ? H->fi.nfree : 0);
    in.step_from_cg = g_ctx.opt_step_from_cg; in.free_image_chain = g_ctx.opt_free_image_chain;
    const StepAccPlan plan = step_acc_select(in);
    if (plan.path == STEP_ACC_SWEEP) return hmul_add_impl(H, s_dev, g_dev, g_minor_out_dev, true, w_dev, s_dev);
    const int64_t n = H->n;
    const int grid = std::max(1, std::min((int)((n + 255) / 256), 1024));
    if (plan.path == STEP_ACC_FULL || plan.path == STEP_ACC_FULL_CARRY) {
        if (plan.path == STEP_ACC_FULL_CARRY)        // (reads g_minor before it is updated)
            hipLaunchKernelGGL(step_carry_q_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, w_dev, (const double*)c.hw, (const double*)g_minor_out_dev,
                               (int)n, c.scalars);
        hipLaunchKernelGGL(vec_add_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const double*)s_dev, w_dev, s_dev, (int)n);
        hipLaunchKernelGGL(vec_add_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const double*)g_minor_out_dev, (const double*)c.hw,
                           g_minor_out_dev, (int)n);
    } else {
        // q0 = g.s + s.(g_minor - g) / 2 from the vectors while all of g_minor is still valid (s is read before it moves)
        if (plan.q_init)
            hipLaunchKernelGGL(model_from_gminor_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, g_dev, (const double*)s_dev, (const double*)g_minor_out_dev,
                               (int)n, c.scalars + 2);
        hipLaunchKernelGGL(vec_add_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const double*)s_dev, w_dev, s_dev, (int)n);
        const int q_mode = plan.path != STEP_ACC_COMPACT_CARRY ? kStepQNone : plan.q_init ? kStepQInit : kStepQCarry;
        hipLaunchKernelGGL(free_image_step_accumulate_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, (const double*)c.s, (const double*)c.hwc,
                           (const int*)H->fi_map, g_minor_out_dev, (int)H->fi.nfree, c.scalars, q_mode);
    }
    BH_HIP(hipGetLastError());
    g_ctx.notes.accumulate_done(H, s_dev, g_dev, g_minor_out_dev, plan);
    return finish_device_call();
}

// active_indx = active_bounds(lincons, x, s, delta); add_active!(lincons, chol_aat, active_indx) — or, when mA + |active_indx| > n,
// active_bounds!(lincons, x+s, chol_aat) — src/basic_tralcnlss.jl:439-453, src/polyhedral_constraints.jl:203-261, on the device:
// the active set lives in HBM, newly fixed variables are taken out of A_free A_free' by a Gram DOWNDATE over just their
// columns (then the mA x mA refactorisation) instead of the reference's from-scratch O(p^3) cholesky_aug_aat rebuild; only
// three counts come back.
int32_t bh_proj_update_active_dev(bh_proj* P, const double* x_dev, const double* s_dev, const double* xlow_dev, const double* xupp_dev,
                                  double delta, double atol, int32_t* n_at_bound, int32_t* n_fixed, int32_t* branch, uint64_t* fix_chunks_out) {
    BH_REQUIRE_INIT();
    if (!P || !x_dev || !s_dev || !xlow_dev || !xupp_dev) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    if (P->mA > 0 && g_ctx.opt_proj_form == 0)
        return fail(BH_ERR_UNSUPPORTED, "bh_proj_update_active_dev needs the reduced projection form (proj_form = 1)");
    const int mA = (int)P->mA;
    hipStream_t s = g_ctx.stream;
    if (mA > 0) {
        BH_TRY(ensure_reduced_buffers(P));
        const size_t lds = trsv_lds_bytes(mA);
        if (lds > kLdsPerCu) return fail(BH_ERR_UNSUPPORTED, "factor too large for the single-workgroup triangular solve");
        BH_TRY(ensure_trsv_lds(lds));
    }
    const bool had_factor = P->active_set && P->reduced && P->M_valid;   // M and Lr describe the CURRENT active set: a downdate is enough
    hipLaunchKernelGGL(active_update_kernel, dim3(1), dim3(CG_T), 0, s, x_dev, s_dev, xlow_dev, xupp_dev, delta, atol, (int)P->n, (int)P->ldA,
                       mA, P->fixrank, P->newidx, P->counts);
    P->mask_epoch = ++g_mask_epoch;
    BH_HIP(hipGetLastError());
    int counts[4] = {0, 0, 0, 0};
    if (mA > 0) {
        // with linear equalities the host chooses between a Gram downdate and a rebuild: it needs the counts now (mailbox round
        // trip); box constraints need nothing between the two kernels, their counts come back with the mask below
        BH_TRY(mbox_ensure());
        BH_TRY(mbox_seal_and_wait(sizeof(counts), nullptr, nullptr, nullptr, P->counts, 4, mbox_dev<int>(kMbInts)));
        for (int i = 0; i < 4; ++i) counts[i] = mbox_host<int>(kMbInts)[i];
        if (counts[AU_BRANCH] == 0 && had_factor) {
            if (counts[AU_NEW] > 0) {
                hipLaunchKernelGGL(gram_downdate_list_kernel, dim3(std::max(1, std::min(1024, (mA * mA + 255) / 256))), dim3(256), 0, s, P->M,
                                   (const double*)P->Ad, P->ldA, mA, (const int*)P->newidx, (const int*)P->counts);
                BH_TRY(launch_chol(P, nullptr));
            }
        } else {
            BH_TRY(launch_reduced_factor(P, true, nullptr));      // active set replaced (or no factor yet): from the mask
        }
    }
    P->active_set = false;
    int info_host = 0;
    int counts_now[4] = {0, 0, 0, 0};
    BH_TRY(adopt_device_mask(P, fix_chunks_out, &info_host, counts_now));   // (canon_mask_kernel leaves AU_AT_BOUND / AU_BRANCH untouched)
    if (info_host != 0) {
        P->active_set = false;
        return fail(BH_ERR_PRECONDITION, "A_free*A_free' is not positive definite (PosDefException in the reference's cholesky)");
    }
    if (mA == 0) for (int i = 0; i < 4; ++i) counts[i] = counts_now[i];                  // arrived with the mask
    if (n_at_bound) *n_at_bound = counts[AU_AT_BOUND];
    if (n_fixed) *n_fixed = P->nfix;
    if (branch) *branch = counts[AU_BRANCH];
    return BH_OK;
}

// norm_reduced_gradient(g, lincons) = norm(projection(lincons, -g)) — src/basic_tralcnlss.jl:869-875 (criticality_measure :839).
// The projector is linear and every operation in it is sign-symmetric in IEEE arithmetic, so ||P(-g)|| and ||P(g)|| are the
// same bits: g is projected as it is.
int32_t bh_reduced_gradient_norm_dev(bh_proj* P, const double* g_dev, double* out) {
    BH_REQUIRE_INIT();
    BH_TRY(check_proj_ready(P));
    if (!g_dev || !out) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    BH_TRY(mbox_ensure());
    double* res = mbox_dev<double>(kMbScal);
    if (P->mA == 0) {
        // box constraints: projection = mask, fused with the norm (one launch, the caller's vector read in place)
        hipLaunchKernelGGL(vec_norm_masked_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, g_dev, P->nfix > 0 ? (const int*)P->fixrank : (const int*)nullptr,
                           (int)P->n, res);
    } else {
        // a vector that needs no padding (n a multiple of 16, 16-byte aligned) is projected where it lies
        const double* rp = g_dev;
        if (P->n != P->ldA || (reinterpret_cast<uintptr_t>(g_dev) & 15u) != 0) {
            BH_TRY(stage_vec(P->rpad, g_dev, P->n, true));
            rp = P->rpad;
        }
        BH_TRY(launch_project(P, rp, P->vtmp, nullptr));
        hipLaunchKernelGGL(vec_norm_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, (const double*)P->vtmp, (int)P->n, res);
    }
    BH_HIP(hipGetLastError());
    BH_TRY(mbox_seal_and_wait(sizeof(double)));
    *out = *mbox_host<double>(kMbScal);
    return BH_OK;
}

// model_reduction = dot(g,s) + 0.5*vthv(H,s) — src/basic_tralcnlss.jl:458.
int32_t bh_model_reduction_dev(bh_hess* H, const double* g_dev, const double* s_dev, double* out) {
    BH_REQUIRE_INIT();
    if (!H || !g_dev || !s_dev || !out) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    BH_TRY(ensure_cg_workspace(H->ld, 0));
    CgWorkspace& c = g_ctx.cg;
    const ModelQuery note = g_ctx.notes.model_query(H, s_dev, g_dev);
    const ModelPath path = model_select(g_ctx.opt_step_from_cg, note.match, note.fixed_part_stale, note.q_valid);
    if (path == MODEL_CARRIED) {
        // a chain of steps under option free_image_chain: g_minor is stale on the fixed variables, q(s) was carried instead
        // (bh_step_accumulate_dev) — it rides to the host with the seal, no launch of its own
        BH_TRY(mbox_ensure());
        BH_TRY(mbox_seal_and_wait(sizeof(double), c.scalars + kStepQSlot, nullptr, mbox_dev<double>(kMbScal)));
        *out = mbox_host<double>(kMbScal)[0];
        return BH_OK;
    }
    if (path == MODEL_FROM_GMINOR) {
        // the library wrote g_minor = H*s + g for exactly these vectors (and, by the caller's opt-in, nobody has touched them since):
        // s'Hs = s.(g_minor - g), g.s — no sweep over J (the rounding of the difference is that of g.s itself: eps |g||s|)
        hipLaunchKernelGGL(model_from_gminor_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, g_dev, s_dev, static_cast<const double*>(note.gm), (int)H->n, c.scalars + 2);
        BH_HIP(hipGetLastError());
        BH_TRY(mbox_ensure());
        BH_TRY(mbox_seal_and_wait(2 * sizeof(double), c.scalars + 2, c.scalars + 3, mbox_dev<double>(kMbScal)));
        *out = mbox_host<double>(kMbScal)[1] + 0.5 * mbox_host<double>(kMbScal)[0];
        return BH_OK;
    }
    const double* sp = H->vpad;
    BH_TRY(device_operand(&sp, H->vpad, s_dev, H->n, H->ld));
    BH_TRY(launch_quad(H, sp));
    hipLaunchKernelGGL(vec_dot_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, g_dev, s_dev, (int)H->n, c.scalars + 1);
    BH_HIP(hipGetLastError());
    BH_TRY(mbox_ensure());
    // s'Hs (all-reduced, so it lives in device memory) and g's ride to the host with the seal
    BH_TRY(mbox_seal_and_wait(2 * sizeof(double), H->scalar, c.scalars + 1, mbox_dev<double>(kMbScal)));
    const double vthv = mbox_host<double>(kMbScal)[0], gs = mbox_host<double>(kMbScal)[1];
    *out = gs + 0.5 * vthv;
    return BH_OK;
}

// After the device-side active set (P->fixrank >= 0 <=> fixed) has changed — bh_cauchy_step, bh_proj_update_active_dev —
// bring the canonical device arrays (fixrank = rank among the fixed, fixidx) and the host bookkeeping in line with it
// WITHOUT moving the mask through the host: a scan kernel renumbers in place, and only the count, the BitVector image
// (n/8 bytes: what the caller's lincons.fixvars needs) and the factorisation flag come back.
static int32_t adopt_device_mask(bh_proj* P, uint64_t* fix_chunks_out, int* info_out, int* counts_out) {
    const int64_t n = P->n;
    const size_t nwords = (size_t)((n + 63) / 64);
    BH_TRY(mbox_ensure());
    const bool via_mbox = kMbChunks + nwords * sizeof(uint64_t) <= kMboxBytes - kMboxPayloadOff;
    std::vector<uint64_t> chunks(nwords, 0ull);
    int counts[5] = {0, 0, 0, 0, 0};          // AU_* and, for mA > 0, the factorisation flag (P->info = P->counts + 4)
    const bool with_info = P->mA > 0 && P->info != nullptr;
    if (via_mbox) {
        // the scan kernel writes the BitVector image straight into the mailbox; counts + flag ride with the seal
        hipLaunchKernelGGL(canon_mask_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, P->fixrank, P->fixidx, (int)n, (int)P->ldA,
                           mbox_dev<unsigned long long>(kMbChunks), P->counts);
        BH_HIP(hipGetLastError());
        BH_TRY(mbox_seal_and_wait(nwords * sizeof(uint64_t) + sizeof(counts), nullptr, nullptr, nullptr, P->counts, with_info ? 5 : 4,
                                  mbox_dev<int>(kMbInts)));
        for (size_t i = 0; i < nwords; ++i) chunks[i] = mbox_host<unsigned long long>(kMbChunks)[i];
        for (int i = 0; i < (with_info ? 5 : 4); ++i) counts[i] = mbox_host<int>(kMbInts)[i];
    } else {
        hipLaunchKernelGGL(canon_mask_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, P->fixrank, P->fixidx, (int)n, (int)P->ldA, P->chunks_dev, P->counts);
        BH_HIP(hipGetLastError());
        count_d2h(nwords * sizeof(uint64_t) + sizeof(counts));
        note_dma();
        BH_HIP(hipMemcpyAsync(chunks.data(), P->chunks_dev, nwords * sizeof(uint64_t), hipMemcpyDeviceToHost, g_ctx.stream));
        BH_HIP(hipMemcpyAsync(counts, P->counts, (with_info ? 5 : 4) * sizeof(int), hipMemcpyDeviceToHost, g_ctx.stream));
        BH_TRY(sync_flush());
    }
    P->nfix = counts[AU_FIXED]; P->mpp = (int)P->mA + P->nfix; P->reduced = P->mA > 0; P->have_L = false;
    P->mask_epoch = ++g_mask_epoch;
    P->last_chunks = chunks;
    P->active_set = true;
    if (fix_chunks_out) memcpy(fix_chunks_out, chunks.data(), nwords * sizeof(uint64_t));
    if (info_out) *info_out = with_info ? counts[4] : 0;
    if (counts_out) for (int i = 0; i < 4; ++i) counts_out[i] = counts[i];
    return BH_OK;
}

// ------------------------------------------------------------------------------------------
// cauchy_step: the plan of one search (decided once), its run context, one launcher per form
// ------------------------------------------------------------------------------------------
// option cauchy_gram_eq: passes between two formations of a = G D g, B = G D A' from the device-side mask
// (the smallest power of two at which a formation costs at most 5 % of the passes in between: DESIGN.md §8 f-5)
constexpr int kCauchyGramEqRefresh = 128;
constexpr int kDowndateRefresh = 8;     // chol_downdate = 1: breakpoints between two from-scratch factorisations

struct CauchyPlan {
    CauchyForm form = CAUCHY_SWEEP; bool fused = false; int refresh = 0;   // the selection (bh_cauchy_plan.h)
    int block = 0;                  // ... and the effective cauchy_block: K >= 2 breakpoints per launch of the one-kernel form, else 0
    bool gemm = false;              // row space with equalities: B = J~ D A' by image_b_mfma_kernel (else mA J v sweeps)
    bool gen_tiled = false;         // ... and its row body in tiles of 64 rows (few equalities: one row per thread, see bh_cauchy.hip.h)
    bool factor_downdate = false;   // sweeping form: rank-one downdates of the factor itself
    int img_grid = 1, fused_grid = 1, gen_grid = 1, reform_cfg = 0, reform_grid = 1;
    int part_G = 1;                 // how many partial sums a row kernel leaves
    int max_pass = 1;
    LaunchAhead sched{};            // the launch-ahead schedule (bh_launch_ahead.h)
    bool image() const { return form == CAUCHY_ROWSPACE_BOX || form == CAUCHY_ROWSPACE_EQ; }
    bool reforms_at(int index) const { return refresh > 0 && index > 0 && (index % refresh) == 0; }
};

// What the passes of one search share.
struct CauchyRun {
    bh_hess* H;
    bh_proj* P;
    CgWorkspace& c;
    hipStream_t s;
    CauchyArgs a{};
    CauchyPlan plan;
    int64_t img_rows = 0;           // rows of J~ = [J; C] on this rank
    int64_t img_cap = 0;            // ... as the images are laid out: rounded up to even (16-byte aligned tails)
    double* img_scal = nullptr;
    CauchyPass* pp = nullptr;
    double* part_pp[2] = {nullptr, nullptr};
    double* sbuf[2] = {nullptr, nullptr};   // s_c ping-pong of the fused form (H*d is never formed there)
    double* sbuf3 = nullptr;                // option cauchy_block: the third s_c buffer, the records and the K-deep partial sums
    CauchyBlockRec* brec = nullptr;
    double* bpart[2] = {nullptr, nullptr};
    int reform_sweeps = 0;          // sweeps over J of one re-formation, for stats.n_jv
};

// Decides everything about the search from the handles and the options.  Launches and allocates nothing.
static CauchyPlan cauchy_make_plan(const bh_hess* H, const bh_proj* P, bool allow_sorted) {
    const int mA = (int)P->mA;
    CauchySelectIn in{};
    in.gram_handle = H->form == BH_HESS_GRAM; in.mA = mA; in.comm = comm_active(); in.lda_is_ld = P->ldA == H->ld;
    in.multi_panel = multi_panel(H); in.last_cauchy_passes = P->last_cauchy_passes;
    in.cauchy_image = g_ctx.opt_cauchy_image; in.cauchy_image_max_ma = g_ctx.opt_cauchy_image_max_ma; in.cauchy_fused = g_ctx.opt_cauchy_fused;
    in.cauchy_gram = g_ctx.opt_cauchy_gram; in.cauchy_gram_eq = g_ctx.opt_cauchy_gram_eq; in.cauchy_image_refresh = g_ctx.opt_cauchy_image_refresh;
    in.n = H->n; in.cauchy_block = g_ctx.opt_cauchy_block;
    in.gram_sorted = allow_sorted && H->cauchy_search == BH_CAUCHY_SORTED;      // (allow_sorted = false: the re-run of a handed-back call)
    CauchyRowsIn rin{};
    rin.rows_sorted = allow_sorted && H->cauchy_rows == BH_CAUCHY_ROWS_SORTED;
    rin.gram_handle = in.gram_handle; rin.mA = mA; rin.comm = in.comm; rin.n = H->n; rin.ld = H->ld;
    rin.ranks = H->cauchy_rows_ranks != 0;                                      // (bh_hess_set_cauchy_rows_ranks: form 6 also with a communicator)
    const CauchySelection sel = cauchy_rows_apply(rin, cauchy_select(in));      // (bh_cauchy_rows_plan.h: form 6 or the selection as it is)
    CauchyPlan p;
    p.form = sel.form; p.fused = sel.fused; p.refresh = sel.refresh; p.block = sel.block;
    // B = J~ D A' (rows x mA): ONE sweep on the matrix cores (image_b_mfma_kernel) when the images share their leading dimension,
    // else mA J v sweeps over masked rows of A
    p.gemm = g_ctx.opt_cauchy_gemm != 0 && P->ldA == H->ld;
    p.gen_tiled = mA > 16;
    // chol_downdate = 1 only has a case where refactoring is expensive (mA > 64: blocked factorisation, 0.21 ms at mA = 256);
    // up to 64 rows the register-panel Cholesky (18.5 us) costs what the rank-one downdate costs (20 us), so the factor is
    // always rebuilt from the downdated Gram matrix there — as accurate as the reference's from-scratch rebuild.
    p.factor_downdate = g_ctx.opt_chol_downdate && mA > 64;
    const int64_t img_rows = H->d + H->q_eff;
    p.reform_cfg = pick_config(std::min<int>(H->nchunks, (int)kMaxChunks));
    p.reform_grid = std::min(kCauchyFusedGrid, grid_for(p.reform_cfg, img_rows));
    p.img_grid = (int)std::max<int64_t>(1, std::min<int64_t>(p.fused ? kCauchyFusedGrid : kCauchyImgGrid, (img_rows + 255) / 256));
    // (fewer, fatter workgroups measured slower: docs/design_history_r3.md)
    p.fused_grid = (int)std::max<int64_t>(1, std::min<int64_t>(kCauchyFusedGrid, (img_rows + CA_T - 1) / CA_T));
    // with equalities a workgroup takes tiles of 64 rows; the partial sums still have to fit the [2][kCauchyImgGrid] slot
    p.gen_grid = (int)std::max<int64_t>(1, std::min<int64_t>(kCauchyImgGrid, (img_rows + 63) / 64));
    p.part_G = (p.form == CAUCHY_ROWSPACE_EQ && p.gen_tiled) ? p.gen_grid : p.img_grid;
    p.max_pass = (int)(H->n + 1);
    // image-space passes take ~17 us: keep a deeper queue ahead of the GPU (over RCCL every over-launched pass costs a collective)
    p.sched.batch = (!p.image() && p.form != CAUCHY_GRAM_EQ) ? launch_batch_size(H) : (comm_active() && !use_peer_path()) ? 4 : 8;
    // (fused form: launch k carries decision k-1, so u launches stand for u - 1 passes)
    p.sched.off = p.fused ? 1 : 0;
    p.sched.max_units = p.max_pass + p.sched.off; p.sched.first = 2 + p.sched.off;
    p.sched.await_iter = false; p.sched.lock_step = true; p.sched.look_first = false;
    // K breakpoints per launch: unit 0 is launch 0, block launch 1 takes decision 0, every later one K decisions (the wait callable
    // translates unit targets into passes: cauchy_block_pass_target); one rank only, so decisions follow `done` as seen
    // (a unit of K passes: four of them queued keep the GPU as busy as eight single passes; batch <= first keeps the units
    // enqueued behind the end of a search below first + batch, whenever the host happens to look: tests/test_cauchy_block_cpu.py)
    if (p.block > 0) {
        p.sched.max_units = 2 + (p.max_pass + p.block - 1) / p.block; p.sched.lock_step = false;
        p.sched.first = 3 + p.sched.off; p.sched.batch = 4;
    }
    return p;
}

// Workspaces of the sorted forms (H->csort: form 5, H->crows: form 6): every offset is bh_cauchy_sort_layout.h's.  The hand-back
// flag is cleared once behind the allocation; the scan kernel leaves it cleared.
static hipError_t cauchy_sort_clear_flag(double* base, int64_t ld, CauchyForm form, hipStream_t s) {
    return hipMemsetAsync(base + cauchy_sort_layout(ld, form, 0).flag, 0, sizeof(int), s);
}
static int cauchy_rows_grid(const bh_hess* H, int64_t img_rows) {
    const int64_t groups = (img_rows + RS_R - 1) / RS_R;
    return (int)std::max<int64_t>(1, std::min<int64_t>(groups, (int64_t)RS_GRID_PER_CU * g_ctx.n_cu));
}
// Allocated at the first search that wants it; false (and no error left behind) when the device has no room: that call and every
// later one stay on the stepwise path until an allocation succeeds.
static bool cauchy_rows_workspace(bh_hess* H, hipStream_t s) {
    if (H->crows) return true;
    const int grid = cauchy_rows_grid(H, H->d + H->q);
    void* p = nullptr;
    if (hipMalloc(&p, (size_t)cauchy_sort_layout(H->ld, CAUCHY_ROWS_SORTED, grid).total * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    H->crows = static_cast<double*>(p); H->crows_grid = grid;
    if (cauchy_sort_clear_flag(H->crows, H->ld, CAUCHY_ROWS_SORTED, s) != hipSuccess) {
        (void)hipGetLastError();
        dev_free(H->crows);
        H->crows = nullptr; H->crows_grid = 0;
        return false;
    }
    return true;
}

// The buffers of the chosen form, grown before the first launch: the images t_d, t_s (+ partial sums and a 16-double tail), a and B
// of the row-space form with equalities, a and B of the Gram form with equalities.
static int32_t cauchy_ensure_buffers(CauchyRun& r) {
    bh_hess* H = r.H;
    const int mA = (int)r.P->mA;
    const int64_t img_cap = r.img_cap;
    if (r.plan.image()) {
        BH_TRY(hess_ready(H));
        if (!H->timg) BH_TRY(dev_alloc(&H->timg, 2 * img_cap + 2 * kCauchyImgGrid + 16));
        r.img_scal = H->timg + 2 * img_cap + 2 * kCauchyImgGrid;
        r.a.img_part = comm_active() ? r.img_scal : H->timg + 2 * img_cap;
        r.a.img_G = comm_active() ? 1 : r.plan.part_G;
        if (r.plan.form == CAUCHY_ROWSPACE_EQ && H->timg_gen_doubles < (int64_t)(1 + mA) * img_cap) {
            dev_free(H->timg_gen);
            H->timg_gen = nullptr; H->timg_gen_doubles = 0;
            BH_TRY(dev_alloc(&H->timg_gen, (int64_t)(1 + mA) * img_cap));
            H->timg_gen_doubles = (int64_t)(1 + mA) * img_cap;
        }
    }
    if (r.plan.form == CAUCHY_GRAM_EQ && H->geq_doubles < (int64_t)(1 + mA) * H->ld) {
        if (H->geq) BH_HIP(hipStreamSynchronize(r.s));            // (launches of an earlier search may still be queued)
        dev_free(H->geq);
        H->geq = nullptr; H->geq_doubles = 0;
        BH_TRY(dev_alloc(&H->geq, (int64_t)(1 + mA) * H->ld));
        H->geq_doubles = (int64_t)(1 + mA) * H->ld;
    }
    r.sbuf[0] = r.c.w; r.sbuf[1] = r.c.Hp;
    if (r.plan.form == CAUCHY_GRAM_SORTED && !H->csort) {
        BH_TRY(dev_alloc(&H->csort, cauchy_sort_layout(H->ld, CAUCHY_GRAM_SORTED, 0).total));
        BH_HIP(cauchy_sort_clear_flag(H->csort, H->ld, CAUCHY_GRAM_SORTED, r.s));
    }
    if (r.plan.fused) {
        r.pp = reinterpret_cast<CauchyPass*>(r.img_scal + 8);     // 2 x 32 bytes in the 16-double tail of timg
        r.part_pp[0] = H->timg + 2 * img_cap; r.part_pp[1] = r.part_pp[0] + 2 * kCauchyFusedGrid;
        r.a.fixpass = reinterpret_cast<int*>(r.c.v); r.a.pp0 = r.pp;
    }
    if (r.plan.block > 0) {
        // (sized for any K and any width the rule admits: allocated once per handle)
        constexpr int64_t rec_doubles = (2 * (int64_t)sizeof(CauchyBlockRec) + 7) / 8;
        const int64_t part_doubles = (int64_t)kCauchyBlockMaxK * 2 * kCauchyFusedGrid;
        if (!H->cblk) BH_TRY(dev_alloc(&H->cblk, kCauchyBlockMaxN + rec_doubles + 2 * part_doubles));
        r.sbuf3 = H->cblk;
        r.brec = reinterpret_cast<CauchyBlockRec*>(H->cblk + kCauchyBlockMaxN);
        r.bpart[0] = H->cblk + kCauchyBlockMaxN + rec_doubles; r.bpart[1] = r.bpart[0] + part_doubles;
        r.a.pp0 = reinterpret_cast<CauchyPass*>(r.brec);          // cauchy_init_kernel writes the first five words of record 0
    }
    return BH_OK;
}

// What every launch of cauchy_image_kernel / the row body with equalities is told about the images (first, fresh: the caller's).
static CauchyImgArgs cauchy_img_args(const CauchyRun& r) {
    const bh_hess* H = r.H;
    CauchyImgArgs ia{};
    ia.st = r.c.d_state; ia.J = H->Jd; ia.ld = H->ld; ia.nrows = r.img_rows; ia.d_rows = H->d; ia.mu = H->mu;
    ia.td = H->timg; ia.ts = H->timg + r.img_cap; ia.part = H->timg + 2 * r.img_cap;
    return ia;
}

static int cauchy_mask_grid(int64_t n) { return std::max(1, std::min((int)((n + 255) / 256), 1024)); }

// Factor of the current active set and y = (A_free A_free')^{-1} A_free(-g) (left in P->tw), as in the sweeping form:
// [downdate + refactorisation + right-hand side + the two solves: y] in one launch behind a decision, two launches at pass 0.
static int32_t cauchy_factor_solve(CauchyRun& r, const ProjArgs& pa, int index) {
    bh_proj* P = r.P;
    const int mA = (int)P->mA;
    if (index > 0) {
        P->linv_valid = false;
        hipLaunchKernelGGL(cauchy_factor_solve_kernel, dim3(1), dim3(256), 0, r.s, P->M, P->Lr, mA, P->info, pa, (const double*)r.c.r,
                           (const double*)P->tpart, (const CgState*)r.c.d_state);
    } else {
        hipLaunchKernelGGL(proj_left_mul_kernel, dim3(mA), dim3(256), 0, r.s, pa, (const double*)r.c.r);     // t (:86-98), then y
        hipLaunchKernelGGL(trsv_small_kernel, dim3(1), dim3(256), 0, r.s, pa);
    }
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// Behind the row kernel of a two-kernel pass: the two sums over all ranks, then the single-workgroup decision.
static int32_t cauchy_sum_and_advance(CauchyRun& r, const double* part) {
    if (comm_active()) {
        hipLaunchKernelGGL(cauchy_image_sum_kernel, dim3(1), dim3(64), 0, r.s, part, r.plan.part_G, r.img_scal, (const CgState*)r.c.d_state);
        BH_TRY(allreduce_inplace(r.img_scal, 2, r.H, r.c.d_state));
    }
    hipLaunchKernelGGL(cauchy_advance_kernel, dim3(1), dim3(CA_T), 0, r.s, r.a);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// Form 0: per breakpoint the factor of the new active set, d = P(-g), one H*d sweep, the decision.
static int32_t cauchy_pass_sweep(CauchyRun& r, int index) {
    bh_hess* H = r.H; bh_proj* P = r.P; CgWorkspace& c = r.c; hipStream_t s = r.s;
    const int mA = (int)P->mA;
    if (index > 0 && mA > 0) {
        if (r.plan.factor_downdate && (index % kDowndateRefresh) == 0) {
            // every kDowndateRefresh-th breakpoint the factor is rebuilt from the device-side mask: hyperbolic downdates lose
            // accuracy cumulatively, and without bound once A_free A_free' approaches singularity (c = sqrt(1 - s^2) -> 0)
            BH_TRY(launch_reduced_factor(P, true, (const CgState*)c.d_state));
        } else if (r.plan.factor_downdate) {
            P->M_valid = false;     // only the factor follows the active set on this path
            // add_active!: one more fixed variable = rank-one downdate of chol(A_free A_free'), O(mA^2)
            P->linv_valid = false;
            hipLaunchKernelGGL(chol_downdate_kernel, dim3(1), dim3(CG_T), (size_t)mA * sizeof(double), s, P->Lr, (const double*)P->Ad,
                               P->ldA, mA, P->info, (const CgState*)c.d_state);
        } else {
            // refactor from the downdated Gram matrix, O(mA^3)
            hipLaunchKernelGGL(gram_downdate_kernel, dim3(std::max(1, (mA * mA + 255) / 256)), dim3(256), 0, s, P->M, P->Ad, P->ldA, mA,
                               (const CgState*)c.d_state);
            BH_TRY(launch_chol(P, (const CgState*)c.d_state));
        }
    }
    if (mA > 0) BH_TRY(launch_project(P, c.r, c.p, c.d_state, true));       // d = P(-g)   :592 / :632  (box: kept in place)
    BH_TRY(launch_hmul(H, c.p, c.Hp, c.d_state, -1));           // Hd = H*d    :609 / :633
    hipLaunchKernelGGL(cauchy_advance_kernel, dim3(1), dim3(CA_T), 0, s, r.a);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// Form 1, two kernels per breakpoint: cauchy_image_kernel over the rows, then the decision.
static int32_t cauchy_pass_rowspace_box(CauchyRun& r, int index) {
    bh_hess* H = r.H; CgWorkspace& c = r.c;
    CauchyImgArgs ia = cauchy_img_args(r);
    ia.first = index == 0 ? 1 : 0;
    ia.fresh = r.plan.reforms_at(index) ? 1 : 0;
    if (index == 0) {
        BH_TRY(launch_jv(H, c.p, H->timg, true, nullptr));              // t_d = J~ d_0 (:609 in the row space)
        H->stats.n_jv += 1;
    }
    if (ia.fresh) {
        // t_d = J~ d from the d the advance kernel keeps (d[ind] is zero already), t_s = J~ s_c: gated by `done`
        BH_TRY(launch_jv(H, c.p, H->timg, true, nullptr, (const CgState*)c.d_state));
        BH_TRY(launch_jv(H, c.w, H->timg + r.img_cap, true, nullptr, (const CgState*)c.d_state));
        r.reform_sweeps = 2;
    }
    hipLaunchKernelGGL(cauchy_image_kernel, dim3(r.plan.img_grid), dim3(256), 0, r.s, ia);
    return cauchy_sum_and_advance(r, ia.part);
}

// Form 1, one kernel per breakpoint: launch 0 forms the images; launch k > 0 takes decision k-1 in the prologue of the row kernel of
// pass k (cauchy_fused_kernel); a launch with a re-formation takes the decision alone and forms both images from J.
static int32_t cauchy_pass_rowspace_fused(CauchyRun& r, int index) {
    bh_hess* H = r.H; CgWorkspace& c = r.c; hipStream_t s = r.s;
    const CauchyPlan& p = r.plan;
    const CauchyArgs& a = r.a;
    if (index == 0) {                                              // launch 0: t_d = J~ d_0 (:609 in the row space), t_s = 0, their sums
        CauchyImgArgs ia = cauchy_img_args(r);
        ia.first = 1;
        BH_TRY(launch_jv(H, c.p, H->timg, true, nullptr));
        H->stats.n_jv += 1;
        hipLaunchKernelGGL(cauchy_image_kernel, dim3(p.img_grid), dim3(256), 0, s, ia);
        BH_HIP(hipGetLastError());
        return BH_OK;
    }
    CauchyFusedArgs fa{};
    fa.pp = r.pp; fa.k = index; fa.g = a.g; fa.dl = a.dl; fa.du = a.du; fa.sbuf[0] = r.sbuf[0]; fa.sbuf[1] = r.sbuf[1];
    fa.fixpass = a.fixpass; fa.fixrank = r.P->fixrank; fa.n = a.n; fa.nmm = a.nmm;
    fa.J = H->Jd; fa.ld = H->ld; fa.nrows = r.img_rows; fa.d_rows = H->d; fa.mu = H->mu;
    fa.td = H->timg; fa.ts = H->timg + r.img_cap;
    fa.part_in = r.part_pp[(index - 1) & 1]; fa.Gin = index == 1 ? p.img_grid : p.reforms_at(index - 1) ? p.reform_grid : p.fused_grid;
    fa.part_out = r.part_pp[index & 1];
    fa.mirror = a.mirror; fa.tag = a.tag;
    if (p.reforms_at(index)) {
        // decision index-1 alone (every group of 64 elements of s_c has its owner at any grid), then both images from J
        fa.decide_only = 1;
        const int dec_grid = (int)std::max<int64_t>(1, std::min<int64_t>(p.fused_grid, ((int64_t)a.n + 63) / 64));
        hipLaunchKernelGGL(cauchy_fused_kernel, dim3(dec_grid), dim3(CA_T), 0, s, fa);
        CauchyReformArgs ra{};
        ra.gate = r.pp + (index & 1); ra.k = index; ra.g = a.g; ra.fixpass = a.fixpass; ra.n = a.n; ra.s = r.sbuf[index & 1];
        ra.J = H->Jd; ra.ld = H->ld; ra.nrows = r.img_rows; ra.d_rows = H->d; ra.mu = H->mu; ra.nchunks = H->nchunks;
        ra.td = fa.td; ra.ts = fa.ts; ra.part = r.part_pp[index & 1];
        launch_cauchy_reform(p.reform_cfg, ra, p.reform_grid, s);
        r.reform_sweeps = 1;
    } else {
        hipLaunchKernelGGL(cauchy_fused_kernel, dim3(p.fused_grid), dim3(CA_T), 0, s, fa);
    }
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// Form 1, K breakpoints per launch (option cauchy_block): launch 0 as above; block launch b >= 1 verifies the decisions block b-1 ran
// ahead of, then runs K passes ahead itself (cauchy_block_kernel<K>, bh_cauchyblock.hip.h).
static int32_t cauchy_pass_rowspace_block(CauchyRun& r, int index) {
    bh_hess* H = r.H; hipStream_t s = r.s;
    const CauchyPlan& p = r.plan;
    const CauchyArgs& a = r.a;
    if (index == 0) return cauchy_pass_rowspace_fused(r, 0);
    CauchyBlockArgs ba{};
    ba.rec = r.brec; ba.b = index; ba.g = a.g; ba.dl = a.dl; ba.du = a.du;
    ba.sbuf[0] = r.sbuf[0]; ba.sbuf[1] = r.sbuf[1]; ba.sbuf[2] = r.sbuf3;
    ba.fixpass = a.fixpass; ba.fixrank = r.P->fixrank; ba.n = a.n; ba.nmm = a.nmm;
    ba.J = H->Jd; ba.ld = H->ld; ba.nrows = r.img_rows; ba.d_rows = H->d; ba.mu = H->mu;
    ba.td = H->timg; ba.ts = H->timg + r.img_cap;
    ba.part_in = index == 1 ? r.part_pp[0] : r.bpart[(index - 1) & 1]; ba.Gin = index == 1 ? p.img_grid : p.fused_grid;
    ba.part_out = r.bpart[index & 1];
    ba.mirror = a.mirror; ba.tag = a.tag;
    switch (p.block) {
        case 2: hipLaunchKernelGGL(cauchy_block_kernel<2>, dim3(p.fused_grid), dim3(CA_T), 0, s, ba); break;
        case 4: hipLaunchKernelGGL(cauchy_block_kernel<4>, dim3(p.fused_grid), dim3(CA_T), 0, s, ba); break;
        case 8: hipLaunchKernelGGL(cauchy_block_kernel<8>, dim3(p.fused_grid), dim3(CA_T), 0, s, ba); break;
        default: hipLaunchKernelGGL(cauchy_block_kernel<16>, dim3(p.fused_grid), dim3(CA_T), 0, s, ba); break;
    }
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// Form 2.  Three launches per pass (mA <= 64): [downdate + refactorisation + right-hand side + the two solves: y]
// -> [rows | d = P(-g) | t_fresh = A_free(-g) for the next pass] -> [decision]
static int32_t cauchy_pass_rowspace_eq(CauchyRun& r, int index) {
    bh_hess* H = r.H; bh_proj* P = r.P; CgWorkspace& c = r.c; hipStream_t s = r.s;
    const CauchyPlan& p = r.plan;
    const int mA = (int)P->mA;
    const int64_t n = H->n, rows_cap = r.img_cap;
    CauchyImgArgs ia = cauchy_img_args(r);
    ia.first = index == 0 ? 1 : 0;
    ia.fresh = p.reforms_at(index) ? 1 : 0;
    ProjArgs pa = proj_args(P, c.d_state, true, true);
    BH_TRY(cauchy_factor_solve(r, pa, index));
    if (index == 0 || ia.fresh) {
        // (index > 0: the re-formation of option cauchy_image_refresh, from the device-side mask — which holds the variable
        // the decision of pass index-1 fixed — and gated by `done`; t_s = J~ s_c from the s_c that decision left)
        const CgState* gate = index == 0 ? nullptr : (const CgState*)c.d_state;
        // a = J~ D g: one J v sweep over the masked g.  B = J~ D A' (rows x mA): the GEMM, or mA J v sweeps (CauchyPlan::gemm)
        const int mgrid = cauchy_mask_grid(n);
        for (int j = -1; j < (p.gemm ? 0 : mA); ++j) {
            const double* src = (j < 0) ? r.a.g : (const double*)(P->Ad + (int64_t)j * P->ldA);
            hipLaunchKernelGGL(proj_mask_kernel, dim3(mgrid), dim3(256), 0, s, src, H->vpad, (const int*)P->fixrank, (int)n, gate);
            BH_TRY(launch_jv(H, H->vpad, H->timg_gen + (int64_t)(j + 1) * rows_cap, true, nullptr, gate));
            if (index == 0) H->stats.n_jv += 1;
        }
        if (p.gemm && r.img_rows > 0) {                 // (a rank without rows has no rows of B)
            hipLaunchKernelGGL(image_b_mfma_kernel, dim3((unsigned)((r.img_rows + 127) / 128)), dim3(256), 0, s, (const double*)H->Jd, H->ld,
                               r.img_rows, (const double*)P->Ad, P->ldA, mA, (const int*)P->fixrank, H->timg_gen + rows_cap, rows_cap, gate);
            BH_HIP(hipGetLastError());
        }
        if (index > 0) {
            BH_TRY(launch_jv(H, c.w, H->timg + rows_cap, true, nullptr, gate));
            r.reform_sweeps = (p.gemm ? 1 : 1 + mA) + 1;
        }
    }
    CauchyImgGenArgs ga{};
    ga.b = ia; ga.a = H->timg_gen; ga.B = H->timg_gen + rows_cap; ga.rows_cap = rows_cap; ga.mA = mA;
    ga.A = P->Ad; ga.ldA = P->ldA; ga.tw = P->tw; ga.g = r.a.g;
    const int dblocks = ((int)(n + 1) / 2 + 63) / 64;
    hipLaunchKernelGGL(cauchy_gen_rows_and_d_kernel, dim3(p.part_G + dblocks + mA), dim3(256), 0, s, ga, p.gen_tiled ? 1 : 0, p.part_G, dblocks, pa,
                       (const double*)c.r, c.p, P->tpart);
    return cauchy_sum_and_advance(r, ia.part);
}

// Form 4: per pass [factor + solves: y] -> [Hd = -a - B y | d = P(-g) | t_fresh] -> [decision from Hd].
static int32_t cauchy_pass_gram_eq(CauchyRun& r, int index) {
    bh_hess* H = r.H; bh_proj* P = r.P; CgWorkspace& c = r.c; hipStream_t s = r.s;
    const int mA = (int)P->mA;
    const int64_t n = H->n;
    ProjArgs pa = proj_args(P, c.d_state, true, true);
    BH_TRY(cauchy_factor_solve(r, pa, index));
    // a = G D g: one G v launch over the masked g (G rebuilt first when it is stale).  B = G D A' (n x mA): the GEMM of the
    // row-space form over the n rows of G.  Pass 0, and again every kCauchyGramEqRefresh-th pass from the device-side mask,
    // which by then holds the variable fixed by the decision in between: the row kernel behind a formation applies no update.
    const bool form_ab = (index % kCauchyGramEqRefresh) == 0;
    if (form_ab) {
        hipLaunchKernelGGL(proj_mask_kernel, dim3(cauchy_mask_grid(n)), dim3(256), 0, s, r.a.g, H->vpad, (const int*)P->fixrank, (int)n,
                           (const CgState*)c.d_state);
        BH_TRY(launch_hmul(H, H->vpad, H->geq, c.d_state, -1));
        hipLaunchKernelGGL(image_b_mfma_kernel, dim3((unsigned)((n + 127) / 128)), dim3(256), 0, s, (const double*)H->G, H->ld, n,
                           (const double*)P->Ad, P->ldA, mA, (const int*)P->fixrank, H->geq + H->ld, H->ld, (const CgState*)c.d_state);
        BH_HIP(hipGetLastError());
    }
    CauchyGramEqArgs ga{};
    ga.st = c.d_state; ga.G = H->G; ga.ld = H->ld; ga.n = (int)n; ga.mA = mA; ga.a = H->geq; ga.B = H->geq + H->ld;
    ga.A = P->Ad; ga.ldA = P->ldA; ga.tw = P->tw; ga.g = r.a.g; ga.Hd = c.Hp; ga.fresh = form_ab ? 1 : 0;
    const int rblocks = (int)(H->ld / 16), dblocks = ((int)(n + 1) / 2 + 63) / 64;
    hipLaunchKernelGGL(cauchy_gram_eq_kernel, dim3(rblocks + dblocks + mA), dim3(256), 0, s, ga, rblocks, dblocks, pa, (const double*)c.r,
                       c.p, P->tpart);
    hipLaunchKernelGGL(cauchy_advance_kernel, dim3(1), dim3(CA_T), 0, s, r.a);
    BH_HIP(hipGetLastError());
    return BH_OK;
}

static int32_t cauchy_launch_pass(CauchyRun& r, int index) {
    switch (r.plan.form) {
        case CAUCHY_ROWSPACE_BOX:
            return r.plan.block > 0 ? cauchy_pass_rowspace_block(r, index) : r.plan.fused ? cauchy_pass_rowspace_fused(r, index) : cauchy_pass_rowspace_box(r, index);
        case CAUCHY_ROWSPACE_EQ: return cauchy_pass_rowspace_eq(r, index);
        case CAUCHY_GRAM_EQ: return cauchy_pass_gram_eq(r, index);
        default: return cauchy_pass_sweep(r, index);               // (CAUCHY_GRAM has no passes: one launch, see cauchy_impl)
    }
}

// The sorted forms — 5 (bh_cauchysort.hip.h, from G) and 6 (bh_cauchyrowsort.hip.h, from J): keys and ranks, the one read of the
// matrix, the scan — the same launches for every search length.  No host round trip before the final progress word.
// Form 5: G is made current by the route launch_hmul takes, without a product.
// Form 6 with a communicator (bh_hess_set_cauchy_rows_ranks): every rank scans its own img_rows = d + q_eff rows (the rows of C on
// rank 0 only), and phi'', X — plain sums over the rows — are summed over the ranks by ONE all-reduce of 2 ld doubles between the slab
// sums and the scan: rank 0's value first, then += rank r, the same bits everywhere.  Everything else the scan reads (T, rank, g, the
// bounds, the flag of cauchy_init_kernel) is replicated, so the replicas decide alike and a hand-back is collective; a NaN in one
// rank's rows reaches every rank through the sum.  A rank without rows launches the row scan with a grid of 1 and no row group: one
// slab of +0.  The exchange is not gated by the loop state: every rank always takes part.
static int32_t cauchy_launch_sorted(CauchyRun& r) {
    bh_hess* H = r.H;
    BH_TRY(hess_ready(H));
    const bool gram = r.plan.form == CAUCHY_GRAM_SORTED;
    if (gram) BH_TRY(ensure_gram(H));   // G rebuilt when stale; before the rank kernel, whose hand-back flag only the scan kernel clears
    const int64_t ld = H->ld;
    double* w = gram ? H->csort : H->crows;
    const CauchySortLayout L = cauchy_sort_layout(ld, r.plan.form, 0);
    CauchySortCore core{};
    core.c = r.a; core.ld = ld; core.T = w + L.T; core.b = w + L.b;
    core.rank = reinterpret_cast<int*>(w + L.rank); core.inv = reinterpret_cast<int*>(w + L.inv); core.flag = reinterpret_cast<int*>(w + L.flag);
    const int key_tiles = (int)((H->n + CS_RANK_TILE - 1) / CS_RANK_TILE);
    BH_HIP(hipMemsetAsync(core.rank, 0, (size_t)ld * sizeof(int), r.s));  // the tiles add their counts into it
    hipLaunchKernelGGL(cauchy_sort_rank_kernel, dim3((unsigned)((ld + CS_RANK_T - 1) / CS_RANK_T), (unsigned)key_tiles), dim3(CS_RANK_T), 0, r.s, core);
    if (gram) {
        CauchySortArgs sa{core};
        sa.G = H->G; sa.UL = w + L.UL; sa.scan = w + L.scan;
        sa.npanels = (int)((ld / 2 + CS_ROW_T * CS_ROW_CPT - 1) / (CS_ROW_T * CS_ROW_CPT));
        const int row_groups = (int)((H->n + CS_ROW_R - 1) / CS_ROW_R);
        const int row_grid = std::max(1, std::min(row_groups, 4 * g_ctx.n_cu / sa.npanels));
        hipLaunchKernelGGL(cauchy_sort_rows_kernel, dim3((unsigned)row_grid, (unsigned)sa.npanels), dim3(CS_ROW_T), 0, r.s, sa);
        hipLaunchKernelGGL(cauchy_sort_scan_kernel, dim3(1), dim3(CS_SCAN_T), 0, r.s, sa);
    } else {
        CauchyRowSortArgs ra{core};
        ra.scan = w + L.scan; ra.red = w + L.red; ra.slab = w + L.slab;
        ra.J = H->Jd; ra.nrows = r.img_rows; ra.d_rows = H->d; ra.mu = H->mu;
        ra.grid = std::min(cauchy_rows_grid(H, r.img_rows), H->crows_grid);
        hipLaunchKernelGGL(cauchy_rowsort_rows_kernel, dim3((unsigned)ra.grid), dim3(RS_T), 0, r.s, ra);
        hipLaunchKernelGGL(cauchy_rowsort_reduce_kernel, dim3((unsigned)((ld + RS_RED_T - 1) / RS_RED_T), 2u), dim3(RS_RED_T), 0, r.s, ra);
        if (comm_active()) {
            BH_HIP(hipGetLastError());
            BH_TRY(allreduce_inplace(ra.red, 2 * ld, H));                   // phi'', then X, by segment: the one collective of the search
        }
        hipLaunchKernelGGL(cauchy_rowsort_scan_kernel, dim3(1), dim3(CS_SCAN_T), 0, r.s, ra);
    }
    BH_HIP(hipGetLastError());
    return BH_OK;
}

// Counters of the handle and the record bh_cauchy_info reads, from the plan and the final progress word.
static void cauchy_account(CauchyRun& r, const MirrorWord& mw, uint64_t launches_in) {
    bh_hess* H = r.H; bh_proj* P = r.P;
    const CauchyPlan& p = r.plan;
    if (p.form == CAUCHY_SWEEP) H->stats.n_hmul += mw.n_hmul;  // (image-space search: passes, not sweeps over J)
    // from G with equalities: the G v launches that ran — pass 0 and every kCauchyGramEqRefresh-th pass (those enqueued behind the end are gated off)
    if (p.form == CAUCHY_GRAM_EQ) H->stats.n_hmul += 1 + std::max(mw.n_hmul - 1, 0) / kCauchyGramEqRefresh;
    // option cauchy_image_refresh: the sweeps over J of the re-formations that ran — pass indices R, 2R, ... below the number of passes
    // (those enqueued behind the end are gated off)
    if (p.refresh > 0) H->stats.n_jv += (int64_t)r.reform_sweeps * (std::max(mw.n_hmul - 1, 0) / p.refresh);
    P->last_cauchy_passes = mw.n_hmul;
    P->last_cauchy_form = (int)p.form;
    P->last_cauchy_launches = (int)(g_kernel_launches - launches_in);
}

// cauchy_step(x, g, H, chol_aat, lincons, delta) — src/basic_tralcnlss.jl:574-639, device-resident: initial
// active_bounds! (poly:203-215), projection of -g, then per breakpoint one H*d, one projection and — instead of the
// reference's O(p^3) host refactorisation (add_active! -> cholesky_aug_aat) — a rank-one downdate of A_free A_free' and an
// mA x mA Cholesky on the device.  On return lincons' active set is the one the reference would hold (fix_chunks_out).
// Which form runs: cauchy_make_plan (the rule: bh_cauchy_plan.h); its passes: cauchy_launch_pass.
static int32_t cauchy_impl(bh_hess* H, bh_proj* P, const double* x, const double* g, const double* xlow, const double* xupp, double delta,
                           double* s_out, uint64_t* fix_chunks_out, int32_t* n_breakpoints, int32_t* n_hmul_out, bool dev,
                           bool allow_sorted = true) {
    BH_REQUIRE_INIT();
    if (!H || !P) return fail(BH_ERR_INVALID_ARG, "NULL handle");
    if (!x || !g || !xlow || !xupp || !s_out) return fail(BH_ERR_INVALID_ARG, "NULL vector argument");
    if (H->n != P->n) return fail(BH_ERR_SHAPE, "H.n != lincons.n");
    if (P->mA > 0 && g_ctx.opt_proj_form == 0)
        return fail(BH_ERR_UNSUPPORTED, "bh_cauchy_step needs the reduced projection form (proj_form = 1)");
    const int64_t n = H->n;
    if (n + 1 >= 0xfffff) return fail(BH_ERR_UNSUPPORTED, "n exceeds the 20-bit pass counter of the progress word");
    const int mA = (int)P->mA;
    const uint64_t launches_in = g_kernel_launches;
    BH_TRY(ensure_cg_workspace(H->ld, 0));
    CgWorkspace& c = g_ctx.cg;
    hipStream_t s = g_ctx.stream;
    if (mA > 0) {
        BH_TRY(ensure_reduced_buffers(P));
        const size_t lds = trsv_lds_bytes(mA);
        if (lds > kLdsPerCu) return fail(BH_ERR_UNSUPPORTED, "factor too large for the single-workgroup triangular solve");
        BH_TRY(ensure_trsv_lds(lds));
    }
    // (the Cauchy kernels read x, g and the bounds element by element: a device caller's vectors are used where they lie)
    if (!dev) g_ctx.notes.compact_operands_overwritten();
    if (!dev) BH_TRY(stage_vecs(c.x, {x, xlow, xupp, g}, n, c.n_pad));            // c.x, c.xlow, c.xupp, c.g are consecutive

    CauchyRun run{H, P, c, s};
    CauchyArgs& a = run.a;
    a.st = c.d_state;
    a.x = dev ? x : c.x; a.g = dev ? g : c.g; a.xlow = dev ? xlow : c.xlow; a.xupp = dev ? xupp : c.xupp;
    a.negg = c.r; a.d = c.p; a.Hd = c.Hp; a.s = c.w; a.dl = c.wl; a.du = c.wu;
    a.fixrank = P->fixrank; a.n = (int)n; a.n_pad = (int)H->ld; a.nmm = (int)(n - mA);
    a.delta = delta; a.atol = std::sqrt(2.220446049250313e-16);
    a.box = (mA == 0) ? 1 : 0;
    a.mirror = c.d_mirror; a.tag = next_mirror_tag(c);

    run.plan = cauchy_make_plan(H, P, allow_sorted);
    // (no room for the workspace of the sorted rows form: the stepwise path, without an error — on one rank.  With a communicator
    // the other ranks would go on into the exchange alone: an error, which bh_hess_set_cauchy_rows_ranks has normally raised already)
    if (run.plan.form == CAUCHY_ROWS_SORTED && !cauchy_rows_workspace(H, s)) {
        if (comm_active()) return fail(BH_ERR_HIP, "cauchy_step: no room for the workspace of the sorted rows form on this rank");
        run.plan = cauchy_make_plan(H, P, false);
    }
    const CauchyPlan& plan = run.plan;
    run.img_rows = H->d + H->q_eff;
    run.img_cap = (std::max<int64_t>(H->d + H->q, 1) + 1) / 2 * 2;
    BH_TRY(cauchy_ensure_buffers(run));
    P->active_set = false;             // device mask is authoritative until adopt_mask below
    P->mask_epoch = ++g_mask_epoch;
    hipLaunchKernelGGL(cauchy_init_kernel, dim3(1), dim3(CG_T), 0, s, a);
    if (mA > 0) BH_TRY(launch_reduced_factor(P, true, nullptr));
    MirrorWord mw{};
    if (plan.form == CAUCHY_GRAM_SORTED || plan.form == CAUCHY_ROWS_SORTED) {
        const bool rows = plan.form == CAUCHY_ROWS_SORTED;
        BH_TRY(cauchy_launch_sorted(run));
        BH_TRY(wait_mirror(c, a.tag, plan.max_pass, &mw));           // published once, by the scan kernel
        // Form 6: an exchange that timed out delivers NaN in the segments of the workgroups that gave up: behind the stop they go
        // unseen, at or before it they look like a hand-back.  Either way the call is BH_ERR_RCCL before a counter moves — not a
        // completed search, and not a stepwise re-run on a dead transport.  (The scan kernel runs behind the exchange: the word is final.)
        if (rows && comm_active()) BH_TRY(check_peer_error());
        // a non-finite g, a NaN bound of a free variable or a non-finite phi', phi'' at the stop: this call runs on the stepwise path
        // with both sorted forms off — codes and bits are that path's; it is not counted as a sorted search.  With a communicator
        // every cause is replicated or travels through the all-reduced sums, so the ranks hand back together.
        if (mw.status == kCauchyHandBack)
            return cauchy_impl(H, P, x, g, xlow, xupp, delta, s_out, fix_chunks_out, n_breakpoints, n_hmul_out, dev, false);
        (rows ? H->stats.n_jv : H->stats.n_hmul) += 1;               // one read of J, or of G
        (rows ? H->searches_rows_sorted : H->searches_sorted) += 1;
    } else if (plan.form == CAUCHY_GRAM) {
        const int launched = plan.max_pass, off = plan.sched.off;   // one launch stands for every pass; off = 0 (not the one-kernel row-space form)
        BH_TRY(launch_hmul(H, c.p, c.Hp, c.d_state, -1));           // Hd = H*d    :609  (rebuilds G first when it is stale)
        H->stats.n_hmul += 1;
        CauchyGramArgs ga{};
        ga.c = a; ga.G = H->G; ga.ld = H->ld;
        if (n <= 8 * CA_T) hipLaunchKernelGGL(cauchy_gram_kernel<true>, dim3(1), dim3(CA_T), 0, s, ga);
        else hipLaunchKernelGGL(cauchy_gram_kernel<false>, dim3(1), dim3(CA_T), 0, s, ga);
        BH_HIP(hipGetLastError());
        BH_TRY(wait_mirror(c, a.tag, launched - off, &mw));        // the kernel publishes once, when its loop has ended
    } else {
        // The launch-ahead schedule of bh_launch_ahead.h, lock-step (mirror: status field = error flag, iter field = breakpoints,
        // n_hmul = passes run).
        BH_TRY(launch_ahead(plan.sched, [&](int index) { return cauchy_launch_pass(run, index); },
                            [&](int n_hmul_target, int iter_target, MirrorWord* m) {
                                const int passes = plan.block > 0 ? cauchy_block_pass_target(n_hmul_target, plan.block) : n_hmul_target;
                                return wait_mirror(c, a.tag, passes, m, iter_target);
                            }, &mw));
    }
    // (fused form: decision j is taken by launch j+1, which writes s_c into buffer (j+1) & 1; K breakpoints per launch: the block
    // launch that took the last decision wrote it into buffer (launch mod 3))
    const double* s_final = c.w;
    if (plan.block > 0) {
        const int bl = cauchy_block_final_launch(mw.n_hmul, plan.block) % 3;
        s_final = bl == 2 ? run.sbuf3 : run.sbuf[bl];
    } else if (plan.fused) {
        s_final = run.sbuf[mw.n_hmul & 1];
    }
    BH_TRY(fetch_vec(s_out, s_final, n, dev));
    int info_host = 0;
    BH_TRY(adopt_device_mask(P, fix_chunks_out, &info_host));     // drains the stream; canonical fixrank / fixidx, P->nfix
    cauchy_account(run, mw, launches_in);
    if (!mw.done) return fail(BH_ERR_HIP, "internal: Cauchy loop did not terminate");
    if (n_breakpoints) *n_breakpoints = mw.iter;
    if (n_hmul_out) *n_hmul_out = mw.n_hmul;
    if (mw.status != 0)
        return fail(BH_ERR_PRECONDITION, "cauchy_step: no breakpoint left (the reference indexes fixvars[-1] here, src/basic_tralcnlss.jl:631)");
    if (info_host != 0)
        return fail(BH_ERR_PRECONDITION, "cauchy_step: A_free*A_free' lost positive definiteness (PosDefException in the reference)");
    return BH_OK;
}

int32_t bh_cauchy_step(bh_hess* H, bh_proj* P, const double* x, const double* g, const double* xlow, const double* xupp, double delta,
                       double* s_out, uint64_t* fix_chunks_out, int32_t* n_breakpoints, int32_t* n_hmul_out) {
    return cauchy_impl(H, P, x, g, xlow, xupp, delta, s_out, fix_chunks_out, n_breakpoints, n_hmul_out, false);
}
int32_t bh_cauchy_step_dev(bh_hess* H, bh_proj* P, const double* x_dev, const double* g_dev, const double* xlow_dev, const double* xupp_dev,
                           double delta, double* s_out_dev, uint64_t* fix_chunks_out, int32_t* n_breakpoints, int32_t* n_hmul_out) {
    return cauchy_impl(H, P, x_dev, g_dev, xlow_dev, xupp_dev, delta, s_out_dev, fix_chunks_out, n_breakpoints, n_hmul_out, true);
}

int32_t bh_cauchy_info(const bh_proj* P, int32_t* form, int32_t* n_launches) {
    BH_REQUIRE_INIT();
    if (!P) return fail(BH_ERR_INVALID_ARG, "NULL handle");
    if (P->last_cauchy_form < 0) return fail(BH_ERR_PRECONDITION, "bh_cauchy_info: no bh_cauchy_step on this handle yet");
    if (form) *form = P->last_cauchy_form;
    if (n_launches) *n_launches = P->last_cauchy_launches;
    return BH_OK;
}

int32_t bh_factor_to_boundary(const double* p, const double* w, const double* w_l, const double* w_u, int64_t n, double atol,
                              double* gamma_out) {
    BH_REQUIRE_INIT();
    if (!p || !w || !w_l || !w_u || !gamma_out || n < 0) return fail(BH_ERR_INVALID_ARG, "bad argument");
    double* buf = nullptr;
    BH_TRY(dev_alloc(&buf, 4 * std::max<int64_t>(n, 1) + 1));
    const double* src[4] = {p, w, w_l, w_u};
    for (int i = 0; i < 4; ++i)
        if (n > 0 && hipMemcpyAsync(buf + i * n, src[i], (size_t)n * sizeof(double), hipMemcpyHostToDevice, g_ctx.stream) != hipSuccess) {
            dev_free(buf);
            return fail(BH_ERR_HIP, "upload");
        }
    hipLaunchKernelGGL(f2b_kernel, dim3(1), dim3(CG_T), 0, g_ctx.stream, buf, buf + n, buf + 2 * n, buf + 3 * n, (int)n, atol, buf + 4 * n);
    hipError_t e = hipMemcpyAsync(gamma_out, buf + 4 * n, sizeof(double), hipMemcpyDeviceToHost, g_ctx.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g_ctx.stream);
    dev_free(buf);
    if (e != hipSuccess) return fail(BH_ERR_HIP, std::string("f2b: ") + hipGetErrorString(e));
    return BH_OK;
}

// ---- plumbing -------------------------------------------------------------------------------
int32_t bh_dev_alloc(void** out, int64_t bytes) {
    BH_REQUIRE_INIT();
    if (!out || bytes < 0) return fail(BH_ERR_INVALID_ARG, "bad argument");
    BH_HIP(hipMalloc(out, (size_t)std::max<int64_t>(bytes, 8)));
    return BH_OK;
}
int32_t bh_dev_free(void* p) { dev_free(p); return BH_OK; }
int32_t bh_dev_upload(void* dst_dev, const void* src_host, int64_t bytes) {
    BH_REQUIRE_INIT();
    if (bytes < 0 || (bytes > 0 && (!dst_dev || !src_host))) return fail(BH_ERR_INVALID_ARG, "bad argument");
    if (bytes == 0) return BH_OK;
    count_h2d((size_t)bytes);
    note_dma();
    BH_HIP(hipMemcpyAsync(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice, g_ctx.stream));
    BH_TRY(sync_flush());
    return BH_OK;
}
int32_t bh_dev_download(void* dst_host, const void* src_dev, int64_t bytes) {
    BH_REQUIRE_INIT();
    if (bytes < 0 || (bytes > 0 && (!dst_host || !src_dev))) return fail(BH_ERR_INVALID_ARG, "bad argument");
    if (bytes == 0) return BH_OK;
    count_d2h((size_t)bytes);
    note_dma();
    BH_HIP(hipMemcpyAsync(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost, g_ctx.stream));
    BH_TRY(sync_flush());
    return BH_OK;
}

int32_t bh_stats(bh_hess* H, bh_stats_t* out) {
    if (!H || !out) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    *out = H->stats;
    out->h2d_bytes = g_ctx.h2d_bytes; out->d2h_bytes = g_ctx.d2h_bytes;       // library-wide, since bh_init
    out->h2d_calls = g_ctx.h2d_calls; out->d2h_calls = g_ctx.d2h_calls;
    return BH_OK;
}
int32_t bh_stats_reset(bh_hess* H) {
    if (!H) return fail(BH_ERR_INVALID_ARG, "NULL argument");
    const double b = H->stats.bytes_per_hmul;
    H->stats = bh_stats_t{};
    H->stats.bytes_per_hmul = b;
    H->timed_bytes = 0.0; H->timed_n = 0;
    H->hmul_seq = 0;          // the first H*p after a reset is always sampled (BH_FLAG_PROFILE)
    return BH_OK;
}

int32_t bh_time_kernel(bh_hess* H, int32_t kind, int32_t reps, double* avg_ms) {
    BH_REQUIRE_INIT();
    if (!H || !avg_ms || reps < 1 || kind < 0 || kind > 11) return fail(BH_ERR_INVALID_ARG, "bad argument");
    BH_TRY(hess_ready(H));
    if (kind >= 9 && H->form != BH_HESS_GRAM) return fail(BH_ERR_PRECONDITION, "bh_time_kernel(9, 10, 11): the handle is not in the Gram form");
    if (kind == 11 && !gram_served(H)) return fail(BH_ERR_PRECONDITION, "bh_time_kernel(11): no lower-triangle kernel for this width");
    if (kind == 7 && !comm_active()) return fail(BH_ERR_PRECONDITION, "bh_time_kernel(7): no communicator (bh_comm_init; BH_FORCE_COMM=1 for one rank)");
    struct EventPair {          // destroyed on every way out of this function
        hipEvent_t a = nullptr, b = nullptr;
        ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } evp;
    BH_HIP(hipEventCreate(&evp.a));
    BH_HIP(hipEventCreate(&evp.b));
    const hipEvent_t e0 = evp.a, e1 = evp.b;
    if (kind >= 9) {
        // 9: a build of G (every launch a real build: gram_builds counts them); 10: the product G·v the handle performs now (all
        // of G in one launch, or the lower triangle and the slab reduction); 11: one quadratic form from G
        BH_TRY(ensure_gram(H));
        const int64_t pl = H->products_lower, qg = H->quads_from_g;       // (the counters count the library's own launches)
        struct Restore { bh_hess* H; int64_t pl, qg; ~Restore() { H->products_lower = pl; H->quads_from_g = qg; } } restore{H, pl, qg};
        auto one = [&]() -> int32_t {
            if (kind == 9) return launch_gram_build(H);
            if (kind == 11) launch_gram_quad(H, H->vpad, H->scalar);
            else if (gram_path(H, GRAM_CALL_PRODUCT) == GRAM_PATH_LOWER) launch_gram_gv_lower(H, H->vpad, H->zpad, nullptr, false, nullptr);
            else launch_gram_gv(H, H->vpad, H->zpad, nullptr, false, nullptr);
            BH_HIP(hipGetLastError());
            return BH_OK;
        };
        BH_TRY(one());                                        // warm-up
        BH_HIP(hipEventRecord(e0, g_ctx.stream));
        for (int i = 0; i < reps; ++i) BH_TRY(one());
        BH_HIP(hipEventRecord(e1, g_ctx.stream));
        BH_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        BH_HIP(hipEventElapsedTime(&ms, e0, e1));
        *avg_ms = ms / reps;
        return BH_OK;
    }
    if (kind >= 7) {
        // 7: the all-reduce of one n-vector on the active communicator path; 8: everything an H*p does after its streaming
        // kernel (slab reduction + exchange).  Back-to-back launches between two events: all ranks must call this together.
        const int cfg = multi_panel(H) ? kPanelCfg : pick_config(H->nchunks);
        const int grid = grid_for(cfg, H->d + H->q_eff);
        int32_t rc = BH_OK;
        for (int i = 0; i < 3 && rc == BH_OK; ++i) rc = (kind == 7) ? allreduce_inplace(H->zpad, H->n, nullptr) : reduce_slabs(H, grid, H->zpad, nullptr);
        if (rc == BH_OK && hipEventRecord(e0, g_ctx.stream) != hipSuccess) rc = fail(BH_ERR_HIP, "hipEventRecord");
        for (int i = 0; i < reps && rc == BH_OK; ++i) rc = (kind == 7) ? allreduce_inplace(H->zpad, H->n, nullptr) : reduce_slabs(H, grid, H->zpad, nullptr);
        if (rc == BH_OK && hipEventRecord(e1, g_ctx.stream) != hipSuccess) rc = fail(BH_ERR_HIP, "hipEventRecord");
        if (rc == BH_OK && hipEventSynchronize(e1) != hipSuccess) rc = fail(BH_ERR_HIP, "hipEventSynchronize");
        float ms = 0.f;
        if (rc == BH_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = fail(BH_ERR_HIP, "hipEventElapsedTime");
        if (rc == BH_OK) rc = check_peer_error();
        if (rc != BH_OK) return rc;
        *avg_ms = ms / reps;
        return BH_OK;
    }
    if (kind >= 3) {
        // read-only stream probe over the (d + q) x ld image: 1, 2, 4 or 8 workgroups per CU
        const int grid = g_ctx.n_cu * (1 << (kind - 3));
        const int64_t nchunks_total = (H->d + H->q) * (H->ld / 2);
        if (grid > H->g_cap * (int)H->ld) return fail(BH_ERR_UNSUPPORTED, "probe output does not fit the slab buffer");
        double total = 0.0;
        for (int i = -1; i < reps; ++i) {           // i = -1: warm-up
            BH_HIP(hipEventRecord(e0, g_ctx.stream));
            hipLaunchKernelGGL(read_probe_kernel, dim3(grid), dim3(256), 0, g_ctx.stream, (const double*)H->Jd, nchunks_total, H->partials);
            BH_HIP(hipEventRecord(e1, g_ctx.stream));
            BH_HIP(hipEventSynchronize(e1));
            float ms = 0.f;
            BH_HIP(hipEventElapsedTime(&ms, e0, e1));
            if (i >= 0) total += ms;
        }
        *avg_ms = total / reps;
        return BH_OK;
    }
    if (multi_panel(H)) return fail(BH_ERR_UNSUPPORTED, "bh_time_kernel: single-panel handles only (n <= 16384)");
    int cfg = pick_config(H->nchunks);
    RowStreamArgs a{};
    a.J = H->Jd; a.ld = H->ld; a.d_rows = H->d; a.nchunks = H->nchunks; a.mu = H->mu; a.state = nullptr;
    a.v = H->vpad; a.u = H->upad; a.partials = H->partials;
    if (kind == 0 && H->fi.present && g_ctx.opt_free_image != 0) {
        // the image the handle's H*p launches stream now: the compact one, at its live width
        a.J = H->Jf; a.ld = H->fi.ldf; a.nchunks = (int)(round_up(H->fi.nfree, 16) / 2);
        cfg = pick_config(a.nchunks);
    }
    a.nrows = (kind == 0) ? H->d + H->q_eff : H->d;
    a.t_out = (kind == 1) ? H->upad : nullptr;
    const int mode = kind == 0 ? MODE_FUSED : (kind == 1 ? MODE_JV : MODE_JTV);
    const int grid = grid_for(cfg, a.nrows);
    launch_row_stream(cfg, mode, a, grid, g_ctx.stream);   // warm-up
    double total = 0.0;
    for (int i = 0; i < reps; ++i) {
        BH_HIP(hipEventRecord(e0, g_ctx.stream));
        launch_row_stream(cfg, mode, a, grid, g_ctx.stream);
        BH_HIP(hipEventRecord(e1, g_ctx.stream));
        BH_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        BH_HIP(hipEventElapsedTime(&ms, e0, e1));
        total += ms;
    }
    *avg_ms = total / reps;
    return BH_OK;
}

// Self-test of the wave reduction network; returns BH_OK when sum and min agree with a host computation.
int32_t bh_selftest(void) {
    BH_REQUIRE_INIT();
    double host_in[256], host_out[512];
    for (int i = 0; i < 256; ++i) host_in[i] = (double)((i * 37) % 101) - 50.0 + 1.0 / (double)(i + 3);
    note_dma();
    BH_HIP(hipMemcpyAsync(g_ctx.scratch_dev, host_in, sizeof(host_in), hipMemcpyHostToDevice, g_ctx.stream));
    hipLaunchKernelGGL(selftest_wave_kernel, dim3(1), dim3(256), 0, g_ctx.stream, g_ctx.scratch_dev, g_ctx.scratch_dev + 256);
    BH_HIP(hipMemcpyAsync(host_out, g_ctx.scratch_dev + 256, sizeof(host_out), hipMemcpyDeviceToHost, g_ctx.stream));
    BH_TRY(sync_flush());
    for (int w = 0; w < 4; ++w) {
        double mn = host_in[64 * w];
        long double s = 0;
        for (int l = 0; l < 64; ++l) { s += host_in[64 * w + l]; mn = std::min(mn, host_in[64 * w + l]); }
        for (int l = 0; l < 64; ++l) {
            if (std::fabs(host_out[64 * w + l] - (double)s) > 1e-11) return fail(BH_ERR_HIP, "wave_sum self-test mismatch");
            if (host_out[64 * w + l] != host_out[64 * w]) return fail(BH_ERR_HIP, "wave_sum lanes disagree");
            if (host_out[256 + 64 * w + l] != mn) return fail(BH_ERR_HIP, "wave_min self-test mismatch");
        }
    }
    // tri_inv_small_kernel (the explicit inverse behind the three-kernel equality iteration): L Linv = I, Linv' stored
    // transposed, zeros above the diagonal and beyond m — every block boundary of the recursion (16 / 32 / 64) and odd sizes
    double *Ld = nullptr, *Wd = nullptr;
    BH_TRY(dev_alloc(&Ld, 64 * 64 + 64));
    int32_t rc = dev_alloc(&Wd, 2 * 4096);
    std::vector<double> L(64 * 64 + 64), W(2 * 4096);
    for (int m : {1, 2, 7, 15, 16, 17, 31, 32, 33, 48, 63, 64}) {
        if (rc != BH_OK) break;
        std::fill(L.begin(), L.end(), std::nan(""));                    // the upper triangle must never be read
        for (int k = 0; k < m; ++k)
            for (int i = k; i < m; ++i)
                L[(size_t)i + (size_t)k * m] = (i == k) ? 1.5 + 0.01 * i : 0.3 * std::sin(1.0 + 0.7 * i + 1.3 * k) / (1.0 + 0.1 * (i - k));
        for (int i = 0; i < m; ++i) L[(size_t)m * m + i] = 1.0 / L[(size_t)i + (size_t)i * m];
        if (hipMemcpy(Ld, L.data(), ((size_t)m * m + m) * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { rc = fail(BH_ERR_HIP, "self-test upload"); break; }
        hipLaunchKernelGGL(tri_inv_small_kernel, dim3(1), dim3(256), 0, g_ctx.stream, (const double*)Ld, m, Wd);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(g_ctx.stream) != hipSuccess ||
            hipMemcpy(W.data(), Wd, W.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(BH_ERR_HIP, "tri_inv self-test launch"); break; }
        for (int i = 0; i < 64 && rc == BH_OK; ++i)
            for (int k = 0; k < 64; ++k) {
                const double x = W[(size_t)k * 64 + i];                 // Linv[i][k]
                if (W[4096 + (size_t)i * 64 + k] != x) { rc = fail(BH_ERR_HIP, "tri_inv self-test: the transposed copy differs"); break; }
                if ((i >= m || k >= m || k > i) && x != 0.0) { rc = fail(BH_ERR_HIP, "tri_inv self-test: non-zero outside the triangle"); break; }
                if (i < m && k <= i) {
                    long double acc = 0;                                 // (L Linv)[i][k]
                    for (int l = k; l <= i; ++l) acc += (long double)L[(size_t)i + (size_t)l * m] * (long double)W[(size_t)k * 64 + l];
                    if (std::fabs((double)acc - (i == k ? 1.0 : 0.0)) > 1e-13) { rc = fail(BH_ERR_HIP, "tri_inv self-test: L Linv != I at m = " + std::to_string(m)); break; }
                }
            }
    }
    dev_free(Ld); dev_free(Wd);
    return rc;
}

}  // extern "C"
