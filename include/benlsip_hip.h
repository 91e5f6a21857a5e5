/*
 * benlsip_hip.h — C ABI of the MI355X (gfx950) backend for BEnlsip.jl's
 * trust-region subproblem hot path.
 *
 * The reference (pure Julia, /root/reference) has no FFI; its seam is Julia
 * multiple dispatch on two concrete types and one function.
 * Every entry point below names the reference method it replaces
 * (path:line relative to the reference root).  julia/BEnlsipHIP.jl holds the
 * `ccall` stubs a maintainer would load next to the unchanged package
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - every function returns int32: 0 = BH_OK, negative = error (bh_strerror);
 *     nothing throws, nothing aborts.
 *   - host pointers are BORROWED for the duration of the call (Julia's GC pins
 *     ccall array arguments exactly that long); anything kept is copied.
 *   - matrices handed over by the host are COLUMN-MAJOR (Julia) with an explicit
 *     leading dimension; indices are 0-based on the C side.
 *   - the only arithmetic type is IEEE fp64.
 *   - one process drives one GPU; handles are not thread-safe (the reference is
 *     single-threaded); every export that takes or returns HOST data is
 *     synchronous unless its name ends _async.
 *   - functions with the suffix _dev take DEVICE pointers (vectors already
 *     resident in HBM; used by bench.py and by callers that keep s, g, w on the
 *     device between calls).  Their device-side results are ordered on the
 *     library stream: they return once the host has what it is owed (status
 *     words, scalars), not necessarily after the stream has drained — see the
 *     option "final_sync" (1 restores a full drain per call).
 *   - multi-GPU: rows of J are sharded over ranks (one process per GPU); each
 *     rank passes its own row block to bh_hess_create*.  After bh_comm_init every
 *     J'·(…) product ends in ONE RCCL all-reduce of n doubles.
 *     Call bh_comm_init BEFORE creating handles (rank 0 alone applies the replicated C rows).
 */
#ifndef BENLSIP_HIP_H
#define BENLSIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------- */
#define BH_OK                 0
#define BH_ERR_INVALID_ARG   -1   /* NULL handle/pointer, negative size, bad leading dimension */
#define BH_ERR_NOT_INIT      -2   /* bh_init has not been called */
#define BH_ERR_HIP           -3   /* a HIP runtime call failed (bh_last_error_detail) */
#define BH_ERR_RCCL          -4   /* an RCCL call failed or librccl could not be loaded */
#define BH_ERR_PRECONDITION  -5   /* reference @assert violated: mpp <= n, mA < mpp when fixed, ... */
#define BH_ERR_SHAPE         -6   /* handle shapes disagree (H.n != P.n, ...) */
#define BH_ERR_NO_DEVICE     -7   /* no gfx950 device visible */
#define BH_ERR_UNSUPPORTED   -8

/* ---- CG_status — src/basic_tralcnlss.jl:12, plus Julia's `nothing` ------ */
#define BH_CG_SOLVED              0
#define BH_CG_BOUND_HIT           1
#define BH_CG_NEGATIVE_CURVATURE  2
#define BH_CG_MAX_ITER_REACHED    3
#define BH_CG_NONE                4   /* reference returns `nothing` */

/* ---- bh_init flags ------------------------------------------------------ */
#define BH_FLAG_PROFILE   1   /* record hipEvents around every H*p launch (bh_stats) */

typedef struct bh_hess bh_hess;   /* device image of AlHessian  — src/basic_tralcnlss.jl:6-10 */
typedef struct bh_proj bh_proj;   /* device image of MixedConstraints — src/polyhedral_constraints.jl:1-7 */

typedef struct bh_stats_t {
    int64_t n_hmul;          /* H*p products executed (fused J'(Jp) launches)            */
    int64_t n_jv;            /* stand-alone J·v launches                                 */
    int64_t n_jtv;           /* stand-alone J'·u launches                                */
    int64_t n_proj;          /* projections applied                                      */
    int64_t n_pcg;           /* bh_pcg calls                                             */
    int64_t n_cg_iter;       /* CG iterations over all bh_pcg calls                      */
    int64_t n_allreduce;     /* RCCL all-reduces issued                                  */
    double  hmul_ms;         /* sum of hipEvent durations of the H*p kernel (BH_FLAG_PROFILE) */
    int64_t hmul_timed;      /* number of H*p launches contributing to hmul_ms           */
    double  bytes_per_hmul;  /* algorithmic bytes of one H*p launch on this rank (8*(d+q)*n + 16*n); once launches have been
                              * sampled (hmul_timed > 0): the mean over those launches of the bytes of the image each one
                              * streamed — 8*(d+q)*nfree + 16*nfree for a launch on the compact image of option "free_image" */
    /* library-wide (all handles), since bh_init: host <-> device copies the library has issued — vectors staged for the
     * host-pointer entry points, masks, factors, traces, J uploads; 8-byte scalars coming back through pinned memory are
     * included.  The *_dev entry points move none of the n-vectors they work on (tests check the difference of these counters). */
    int64_t h2d_bytes, d2h_bytes, h2d_calls, d2h_calls;
    /* launch shape of the last bh_pcg on this handle: kernels per CG iteration in the fused forms, the collective not counted
     * (box constraints 2, on one rank and over either transport; equalities 3 through the explicit factor inverse — 4 with
     * cg_fused = 2 — on one rank and over the peer buffers, one more over RCCL: the slab reduction in front of ncclAllReduce);
     * 0 = the separate-kernel forms (three kernels for box constraints, seven with equalities; option "cg_fused").
     * On a handle in the Gram form: 0 (G·v + single-workgroup step kernel; six launches with equalities) unless option
     * "gram_cg_fused" is on, then 2 (box constraints) or 3 (up to 64 equalities in the reduced projection form), 0 otherwise. */
    int64_t cg_kernels;
} bh_stats_t;

/* ---- library / device --------------------------------------------------- */

/* Select HIP device `device` for this process, create the stream and workspaces. */
int32_t bh_init(int32_t device, int32_t flags);
int32_t bh_shutdown(void);
/* Use a caller-owned hipStream_t (e.g. torch's current stream) for all launches; NULL restores the library stream. */
int32_t bh_set_stream(void* hip_stream);
int32_t bh_synchronize(void);
const char* bh_strerror(int32_t code);
const char* bh_last_error_detail(void);
/* Name, CU count and arch string of the selected device (diagnostics). */
int32_t bh_device_info(char* name_out, int64_t name_cap, int32_t* n_cu, char* arch_out, int64_t arch_cap);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) --------------------- */
#define BH_UNIQUE_ID_BYTES 128
/* rank 0 creates the id, the host runtime (torch.distributed, MPI, a Julia Distributed channel) broadcasts it. */
int32_t bh_comm_unique_id(void* id_out /* BH_UNIQUE_ID_BYTES */);
/* Two interchangeable transports for the one exchange on the path (the sum over ranks of an n-vector per J'·), chosen by the
 * environment variable BH_COMM when the communicator is created:
 *   "rccl" (default)  ncclAllReduce(n doubles, sum) on the library stream.
 *   "ipc"             one-shot exchange over peer-mapped buffers (hipIpc; ranks of ONE node, <= 8): every rank pushes its
 *                     partial into all inboxes and sums what it received in rank order — one hop instead of a ring, fused
 *                     into the kernel that reduces the per-workgroup slabs, bit-identical on all ranks by construction, and
 *                     skipped on the device by over-launched (already finished) CG iterations.  Needs no librccl.
 *   "both"            both are brought up; bh_set_option("comm_path", 0|1) switches (default RCCL).
 * Both return BH_ERR_PRECONDITION while any bh_hess handle is alive: a handle records at creation whether THIS rank applies
 * the replicated C rows (rank 0 does), so the rank must not change under it.  Order: bh_init, bh_comm_init, create handles,
 * ..., destroy handles, bh_comm_destroy.  (nranks == 1 creates no communicator and is always accepted.)
 * BH_RCCL_LIB (environment) names the librccl to load; default: the copy already mapped into the process, else the system one.
 * With the peer-buffer transport bh_comm_init ends with a REACHABILITY CHECK: one real exchange of a known vector through every
 * mapped inbox (timeout BH_PEER_ECHO_TIMEOUT_S, default 5 s).  If it fails on any rank — the mappings opened but a peer's stores
 * do not land — it fails on EVERY rank (BH_ERR_RCCL, "reachability check failed"), no communicator is left behind, and the caller
 * may call bh_comm_init again with BH_COMM=rccl.  (BH_PEER_TIMEOUT_S, default 20 s: how long a later exchange waits for a peer
 * before it poisons its result with NaN and raises the transport's error state.  BH_PEER_ECHO_SKIP_RANK=r: test hook, rank r
 * stays away from the check.) */
int32_t bh_comm_init(int32_t rank, int32_t nranks, const void* id /* BH_UNIQUE_ID_BYTES */);
int32_t bh_comm_destroy(void);
int32_t bh_comm_info(int32_t* rank, int32_t* nranks);

/* ---- AlHessian ---------------------------------------------------------- */

/* Replaces the constructor AlHessian(Jx,Cx,mu) at src/basic_tralcnlss.jl:46,84: uploads this
 * rank's row block of J (d x n, column-major, leading dimension ldJ >= d) and C (q x n; may be
 * NULL when q == 0; replicated on every rank) and lays them out for the kernels. */
int32_t bh_hess_create(bh_hess** out, const double* J, int64_t d, int64_t n, int64_t ldJ,
                       const double* C, int64_t q, int64_t ldC, double mu);
/* The same for a Jacobian that already lives in HBM (a device-side jac_res): J_dev is a DEVICE pointer,
 * column-major d x n with leading dimension ldJ; only the transpose into the kernels' layout happens (no PCIe traffic for J).
 * C (q x n) stays a host pointer. */
int32_t bh_hess_create_dev(bh_hess** out, const double* J_dev, int64_t d, int64_t n, int64_t ldJ,
                           const double* C, int64_t q, int64_t ldC, double mu);
/* Asynchronous ingest: like bh_hess_create, but returns as soon as the upload has been started.  A worker
 * thread streams J in column chunks (option "upload_chunk_mb", default 64 MiB) through two device staging buffers: the PCIe
 * copy of chunk k+1 overlaps the device transpose of chunk k, and both overlap whatever the caller does next on the host
 * (the reference evaluates the residuals and the constraints of the next point there, src/basic_tralcnlss.jl:352).
 * J must stay valid and unchanged until bh_hess_wait — or the first use of the handle, which waits implicitly — returns;
 * C is small and is copied before the call returns.  With a communicator every rank must call bh_hess_wait (or make its
 * first use of the handle) at the same point of its call sequence.
 * With option "gram_ingest" = 1 (read at this call; one rank, n <= 16384) the handle is born in the Gram form (BH_HESS_GRAM below)
 * and G is built while J arrives: behind the transpose of every chunk the worker launches, on one more stream, the 64 x 64 lower
 * blocks of G whose columns are all in the image by then (gn_gram_panel_kernel over row slabs + gn_gram_panel_reduce_kernel; no
 * atomics, fixed order: G bitwise symmetric, a repeated ingest bit-identical).  When bh_hess_wait (or the implicit wait of the
 * first use) returns, G is valid for the mu of this call, bh_hess_get_form reports BH_HESS_GRAM and one build, and the first
 * product launches none.  A bh_hess_set_mu before that leaves G stale (rebuilt at the next use, as ever); d = 0: no upload, G
 * comes from the C rows through the ordinary build at first use; a failed allocation of G fails the call.  bh_hess_destroy and
 * bh_hess_set_form(H, BH_HESS_IMPLICIT) while the upload runs first wait for it and its builds. */
int32_t bh_hess_create_async(bh_hess** out, const double* J, int64_t d, int64_t n, int64_t ldJ,
                             const double* C, int64_t q, int64_t ldC, double mu);
int32_t bh_hess_wait(bh_hess* H);
/* Benchmark constructor: rows [row0, row0+d) of the d_total x n synthetic Jacobian of SURVEY.md §8(d),
 * element (i,j) = u(seed, i + j*d_total)/sqrt(d_total) * (colscale ? colscale[j] : 1), generated in HBM. */
int32_t bh_hess_create_synthetic(bh_hess** out, int64_t d, int64_t n, int64_t row0, int64_t d_total,
                                 uint64_t seed, const double* colscale /* n or NULL */, double mu);
/* Changing mu of the Gram form marks G stale (rebuilt before the next product that reads it); the same mu is a no-op. */
int32_t bh_hess_set_mu(bh_hess* H, double mu);
int32_t bh_hess_destroy(bh_hess* H);
/* Form of the Gauss-Newton Hessian behind a handle.  Opt-in per handle; a new handle is BH_HESS_IMPLICIT.
 *   BH_HESS_IMPLICIT  every product H*v = J'(Jv) + C'(mu C v) streams the whole image of J once (the default).
 *   BH_HESS_GRAM      the explicit Gram matrix G = J'J + mu C'C (ld x ld doubles, exactly symmetric) is built on the fp64 matrix
 *                     cores (gn_gram_mfma_kernel) before the first product that needs it — after an asynchronous ingest has
 *                     finished, on the library stream, without a host synchronisation — and every such product is ONE G·v launch
 *                     (8 n ld bytes instead of 8 (d+q) n; no slab reduction).  A new mu (bh_hess_set_mu) rebuilds it once.
 *   Reading G in the Gram form: Base.:*(H, v) — src/basic_tralcnlss.jl:102-106 (bh_hmul, bh_hmul_dev), bh_hmul_add(_dev) and
 *   bh_step_accumulate_dev, the H*p of projected_cg(...) — src/basic_tralcnlss.jl:690-764 (bh_pcg*, bh_minor_iterate*: by default the
 *   separate-kernel CG shape, stats.cg_kernels = 0, pHp = dot(p, H*p) as the reference forms it at :723; with option
 *   "gram_cg_fused" = 1 the fused shape, stats.cg_kernels = 2 or 3, the same dot(p, H*p) summed per workgroup) and the H*d form of
 *   cauchy_step(...) — src/basic_tralcnlss.jl:574-639 (cauchy_image = 0, or more linear equalities than its row-space form takes);
 *   with option "cauchy_gram" = 1 also the whole box-constrained search of cauchy_step(...) (no linear equalities, one rank):
 *   Hd = G d once, then one row of G per breakpoint inside ONE launch (cauchy_gram_kernel); with option "cauchy_gram_eq" = 1 the
 *   search with 1..64 linear equalities (one rank): Hd = -a - B y from a = G D g (n) and B = G D A' (n x mA), one row of G per
 *   breakpoint, a and B formed again from G every 128th pass (cauchy_gram_eq_kernel; bh_cauchy_info form 4).
 *   Still reading J: vthv(H, v) — src/basic_tralcnlss.jl:92-96 and bh_linesearch (||Jv||^2_W, never negative; from G instead only
 *   under BH_GRAM_READ_LOWER_QUAD, bh_hess_set_gram_read below), bh_jv, bh_jtv,
 *   bh_grad, and the row-space Cauchy search (cauchy_image = 1; with box constraints only while "cauchy_gram" = 0, with up to
 *   64 equalities only while "cauchy_gram_eq" = 0).
 * bh_hess_set_form: setting the current form is a no-op; BH_HESS_IMPLICIT frees G; BH_ERR_INVALID_ARG for another value;
 * BH_ERR_UNSUPPORTED for n > 16384 (G would exceed 2 GiB) or while a communicator with more than one rank is active; a failed
 * allocation returns BH_ERR_HIP and leaves the handle in the implicit form.  While the Gram form is on, stats.bytes_per_hmul is
 * 8 n ld + 16 n (the full read).  bh_hess_get_form: the current form and how many times G has been built on this handle. */
#define BH_HESS_IMPLICIT 0
#define BH_HESS_GRAM     1
int32_t bh_hess_set_form(bh_hess* H, int32_t form);
int32_t bh_hess_get_form(const bh_hess* H, int32_t* form, int64_t* gram_builds);
/* How a handle in the Gram form reads G, which is bitwise symmetric.  Opt-in per handle, next to bh_hess_set_form; no option key.
 *   BH_GRAM_READ_FULL        the default: every path, launch, counter and bit is what it is without this switch.
 *   BH_GRAM_READ_LOWER       every product G·v that goes through the one product launcher (bh_hmul*, bh_hmul_add*, the sweep path of
 *                            bh_step_accumulate_dev, the separate-kernel CG loop, the G d of "cauchy_gram", the a = G D g of
 *                            "cauchy_gram_eq", the H*d form of the Cauchy search) reads the elements G_ij, j <= i, only: one launch
 *                            over the lower triangle (gram_symv_kernel: row sums t_i = sum_{j<=i} G_ij v_j and the transposed
 *                            contributions v_i G_ij, one slab per workgroup) and the slab reduction — two launches, every sum in a
 *                            fixed order, no atomics.  The operator is the same, its rounding moves (other summation order).
 *                            stats.bytes_per_hmul becomes 16 * (number of 16-byte chunks 0 .. i/2 of the rows i < n) + 16 n; the
 *                            slab traffic is not counted.  gram_cg_kernel ("gram_cg_fused"), cauchy_gram_kernel and
 *                            cauchy_gram_eq_kernel need contiguous whole rows and keep reading them: G stays stored in full.
 *   BH_GRAM_READ_LOWER_QUAD  ... and the calls that end in vthv's weighted square sum — bh_vthv, bh_linesearch(_dev),
 *                            bh_minor_iterate* with ls_from_cg = 0, bh_model_reduction_dev where it would sweep — take v'Gv from ONE
 *                            launch over the lower triangle (q_i = v_i (2 sum_{j<i} G_ij v_j + G_ii v_i), one partial per
 *                            workgroup, folded in index order) instead of a sweep over J: stats.n_jv does not grow on them,
 *                            quads_from_g does.  The value is used exactly where vthv's was; no branch is added.  What is lost:
 *                            ||Jv||^2_W is a sum of squares and never negative, while v'Gv is the same number rounded differently
 *                            and can come out <= 0 where the true value is near zero (a direction almost in the null space of J).
 *                            That is why this is a mode of its own and not part of BH_GRAM_READ_LOWER.
 * bh_hess_set_gram_read may be called in either form: the mode is remembered and takes effect while the handle is in the Gram form.
 * It never rebuilds G and raises no event on the step-chain notes.  NULL handle or a mode outside 0..2: BH_ERR_INVALID_ARG, the
 * handle keeps its mode.  bh_hess_get_gram_read: the mode; served = 1 when the handle's width has a lower-triangle kernel (n <= 8192:
 * for 8192 < n <= 16384 the product kernel does not fit the register file; a handle that is not served keeps the full read and the sweep over J under every mode, both counters stay 0);
 * products_lower / quads_from_g = launches of the two lower-triangle forms since the handle was created.  Any pointer may be NULL. */
#define BH_GRAM_READ_FULL        0
#define BH_GRAM_READ_LOWER       1
#define BH_GRAM_READ_LOWER_QUAD  2
int32_t bh_hess_set_gram_read(bh_hess* H, int32_t mode);
int32_t bh_hess_get_gram_read(const bh_hess* H, int32_t* mode, int32_t* served, int64_t* products_lower, int64_t* quads_from_g);
/* Which box-constrained Cauchy search a handle in the Gram form runs.  Opt-in per handle, next to bh_hess_set_gram_read; no option key.
 *   BH_CAUCHY_STEPWISE  the default: every path, launch, counter and bit is what it is without this switch.
 *   BH_CAUCHY_SORTED    bh_cauchy_step(_dev) on a Gram-form handle, no linear equalities, one rank: the search from ONE sorted sweep over
 *                       G (bh_cauchy_info form 5).  With box constraints d_i = -g_i while variable i is free, so every breakpoint time
 *                       T_i = b_i / d_i is known before the first pass and the variables are fixed in the order of (T_i, i); phi' and
 *                       phi'' of every segment follow from one read of the free rows of G plus prefix and true suffix sums.  Three
 *                       launches behind the initial one (cauchy_sort_rank_kernel, cauchy_sort_rows_kernel, cauchy_sort_scan_kernel),
 *                       the same for every search length; no host round trip before the final progress word.  It goes ahead of option
 *                       "cauchy_gram" and is independent of every Cauchy option.  *n_hmul of bh_cauchy_step(_dev) is the number of
 *                       decisions k* + 1 (the reference's H*d products, as in every other form), n_breakpoints = k*; stats.n_hmul
 *                       grows by 1 (one read of G), stats.n_jv by nothing.  The step agrees with the other forms to rounding (same
 *                       active set, same counts; bit for bit on exactly representable data); a repeated search is bit-identical.
 *                       BH_GRAM_READ_LOWER does not apply: the form reads whole contiguous rows, like forms 3 and 4.
 *                       Any other handle or constraint set (implicit form, linear equalities, several ranks) takes the path it takes
 *                       without the switch, silently and bit for bit.
 *                       Hand-back: a non-finite g or a NaN bound on a free variable, or a non-finite phi' or phi'' at the stop, makes
 *                       the library run that call again on the path the handle takes with BH_CAUCHY_STEPWISE — return codes and
 *                       bits are that path's; searches_sorted does not count such a call.  "No breakpoint left" is decided by the
 *                       same rule as in the other forms and returns the same BH_ERR_PRECONDITION.
 * bh_hess_set_cauchy_search may be called in either form: the mode is remembered and takes effect while the handle is in the Gram form.
 * It never rebuilds G and raises no event on the step-chain notes.  NULL handle or a mode outside 0..1: BH_ERR_INVALID_ARG, the
 * handle keeps its mode.  bh_hess_get_cauchy_search: the mode; served = 1 for n <= 16384 (the Gram form's own limit);
 * searches_sorted = searches the sorted form completed since the handle was created.  Any pointer may be NULL. */
#define BH_CAUCHY_STEPWISE 0
#define BH_CAUCHY_SORTED   1
int32_t bh_hess_set_cauchy_search(bh_hess* H, int32_t mode);
int32_t bh_hess_get_cauchy_search(const bh_hess* H, int32_t* mode, int32_t* served, int64_t* searches_sorted);
/* Which box-constrained Cauchy search a handle in the IMPLICIT form runs.  Opt-in per handle, next to bh_hess_set_cauchy_search (whose
 * contract is unchanged: it concerns the Gram form only); no option key.
 *   BH_CAUCHY_ROWS_STEPWISE  the default: every path, launch, counter and bit is what it is without this switch.
 *   BH_CAUCHY_ROWS_SORTED    bh_cauchy_step(_dev) on an implicit handle, no linear equalities, one rank, a served width: the search
 *                       from ONE sorted sweep over J (bh_cauchy_info form 6).  The order (T_i, i) in which variables are fixed is
 *                       known before the first pass; per row of the image [J; C] the entries of the free variables are taken in
 *                       that order, J~ d of every segment is a true suffix sum and the part of J~ s_c already at its bounds a
 *                       prefix sum, and phi'' = sum w S^2, s_c'Hd = sum w P S + T phi'' of every segment follow from one read of J.
 *                       Four launches behind the initial one (cauchy_sort_rank_kernel, cauchy_rowsort_rows_kernel,
 *                       cauchy_rowsort_reduce_kernel, cauchy_rowsort_scan_kernel), the same for every search length; no host round
 *                       trip before the final progress word.  It goes ahead of, and is independent of, every Cauchy option
 *                       ("cauchy_image", "cauchy_fused", "cauchy_block", "cauchy_image_refresh").  *n_hmul of bh_cauchy_step(_dev) is
 *                       the number of decisions k* + 1 (the reference's H*d products), n_breakpoints = k*; stats.n_jv grows by 1
 *                       (one read of J), stats.n_hmul by nothing.  The step agrees with the other forms to rounding (same active
 *                       set, same counts; bit for bit on exactly representable data); a repeated search is bit-identical; the bits
 *                       may depend on the number of compute units (which rows share a partial sum), as those of H*p do.
 *                       Any other handle or constraint set (Gram form, linear equalities, an unserved width; a communicator unless
 *                       bh_hess_set_cauchy_rows_ranks, below, is on) takes
 *                       the path it takes without the switch, silently and bit for bit; so does a call for whose workspace the
 *                       device has no room.
 *                       Hand-back: as with BH_CAUCHY_SORTED — a non-finite g or a NaN bound on a free variable, or a non-finite
 *                       phi' or phi'' at the stop, makes the library run that call again on the stepwise path with both sorted
 *                       forms off; return codes and bits are that path's; searches_rows_sorted does not count such a call.  "No
 *                       breakpoint left" is decided by the same rule as in the other forms and returns the same BH_ERR_PRECONDITION.
 * The mode is remembered across bh_hess_set_form and takes effect while the handle is in the implicit form.  It never rebuilds
 * anything and raises no event on the step-chain notes.  NULL handle or a mode outside 0..1: BH_ERR_INVALID_ARG, the handle keeps its
 * mode.  bh_hess_get_cauchy_rows: the mode; served = 1 for n <= 4096 (the one geometry of the row scan: 512 threads x 8 ranks, a
 * row of the image in LDS), else 0; searches_rows_sorted = searches the form completed since the handle was created.  Any pointer may
 * be NULL. */
#define BH_CAUCHY_ROWS_STEPWISE 0
#define BH_CAUCHY_ROWS_SORTED   1
int32_t bh_hess_set_cauchy_rows(bh_hess* H, int32_t mode);
int32_t bh_hess_get_cauchy_rows(const bh_hess* H, int32_t* mode, int32_t* served, int64_t* searches_rows_sorted);
/* BH_CAUCHY_ROWS_SORTED on a ROW-SHARDED handle.  A switch of its own, 0 (the default) or 1, next to bh_hess_set_cauchy_rows, whose
 * contract is unchanged: without this switch a call with a communicator keeps the stepwise path (one all-reduce per breakpoint).
 *   on = 1   a call takes form 6 when ALL of these hold: this switch is 1, bh_hess_set_cauchy_rows is at BH_CAUCHY_ROWS_SORTED, a
 *            communicator is active, the handle is implicit, there are no linear equalities and the width is served (n <= 4096).
 *            phi''_k = sum_i w_i S_ik^2 and X_k = sum_i w_i P_ik S_ik are plain sums over the rows of [J; C], and the rows are what the
 *            ranks hold: every rank scans its own rows (the rows of C on rank 0 only), ONE all-reduce of 2 ld doubles (phi'', then X,
 *            by segment; 64 KiB at n = 4096) sums them — rank 0's value first, then += rank r, so every rank holds the same bits —
 *            and the scan runs replicated on identical inputs.  One collective per search instead of one per breakpoint; the launches
 *            of form 6 plus the exchange (one more launch on the peer-buffer transport, an ncclAllReduce otherwise), the same for
 *            every search length.  Per completed search on every rank: stats.n_allreduce + 1, stats.n_jv + 1, searches_rows_sorted + 1;
 *            *n_hmul / n_breakpoints keep form 6's meaning.  A rank without rows takes part with sums of +0.  Replicas are
 *            bit-identical; against one rank the sums are associated differently (rows meet per rank first), so the step agrees to
 *            rounding, and bit for bit on exactly representable data.
 *            Hand-back is collective: its causes (non-finite g, a NaN bound, non-finite phi', phi'' at the stop) are replicated or
 *            travel through the all-reduced sums, so all ranks re-run the stepwise path together.  An exchange that timed out is
 *            BH_ERR_RCCL — checked behind every such search, before a counter moves — not a hand-back and not a completed search.
 *            Setting 1 allocates the workspace of the form at once and returns BH_ERR_HIP when the device has no room (the switch
 *            stays 0): no rank finds out at search time that it alone must fall back.  For the same reason a search on a
 *            communicator whose workspace is missing returns BH_ERR_HIP instead of falling back quietly, as one rank does.
 *   on = 0   every call keeps the path it takes today, bit for bit.  With one process and no communicator the switch changes nothing.
 * Remembered across bh_hess_set_form.  NULL handle or a value other than 0 / 1: BH_ERR_INVALID_ARG, the state unchanged.  All ranks
 * must set the same value (like every replicated setting).  Every several-rank figure of this form is a COUNT (launches,
 * collectives) from several processes on one GPU; no several-rank time has been measured. */
int32_t bh_hess_set_cauchy_rows_ranks(bh_hess* H, int32_t on);
int32_t bh_hess_get_cauchy_rows_ranks(const bh_hess* H, int32_t* on);
int32_t bh_hess_shape(const bh_hess* H, int64_t* d, int64_t* n, int64_t* q);
/* The compact image of the free columns (option "free_image"): one row per row of the image of J, only the columns of the
 * variables that are free, dense; the box-constrained CG loop of bh_pcg* streams it instead of J.
 * bh_hess_free_image_info: state = 0 none, 1 valid, 2 stale — with `lincons` given: an image exists but describes another
 * active set than the current one of `lincons` (newly fixed variables are moved out by the next eligible call when that pays;
 * a freed variable needs a rebuild); with NULL an existing image reports 1.  width = its live columns (0: none), builds and
 * moves (columns) = since the handle was created, calls_served = bh_pcg* (and, under option "free_image_minor", bh_minor_iterate*)
 * calls whose CG loop ran on it.  Any pointer may be NULL.
 * bh_hess_free_image_read (debugging and tests): the image as it lies in memory, rows x stride doubles row-major (columns from
 * width on are zero), and the slot -> original column map (stride ints, -1 from width on).  rows / stride are always reported;
 * a NULL buffer is skipped; BH_ERR_PRECONDITION when the handle has no image, BH_ERR_INVALID_ARG when a buffer is too small. */
int32_t bh_hess_free_image_info(const bh_hess* H, const bh_proj* lincons, int32_t* state, int64_t* width, int64_t* builds, int64_t* moves,
                                int64_t* calls_served);
int32_t bh_hess_free_image_read(bh_hess* H, double* image_out, int64_t image_cap, int32_t* map_out, int64_t map_cap, int64_t* rows,
                                int64_t* stride);

/* Base.:*(H::AlHessian, v) — src/basic_tralcnlss.jl:102-106:  out = J'(Jv) + C'(mu C v). */
int32_t bh_hmul(bh_hess* H, const double* v, double* out_n);
/* vthv(H,v) — src/basic_tralcnlss.jl:92-96:  ||Jv||^2 + mu ||Cv||^2. */
int32_t bh_vthv(bh_hess* H, const double* v, double* out_scalar);
/* H.J*v — src/basic_tralcnlss.jl:93,103 (this rank's d rows). */
int32_t bh_jv(bh_hess* H, const double* v, double* out_d);
/* H.J'*u — src/basic_tralcnlss.jl:105 and g = Jx'*rx at :45,:74,:893 (u = this rank's d rows; result all-reduced). */
int32_t bh_jtv(bh_hess* H, const double* u, double* out_n);
/* Device-pointer forms (no PCIe traffic). */
int32_t bh_hmul_dev(bh_hess* H, const double* v_dev, double* out_n_dev);
int32_t bh_jv_dev(bh_hess* H, const double* v_dev, double* out_d_dev);
int32_t bh_jtv_dev(bh_hess* H, const double* u_dev, double* out_n_dev);

/* ---- MixedConstraints --------------------------------------------------- */

/* Replaces MixedConstraints(A, chol_aat; l, u) — src/polyhedral_constraints.jl:9-18: uploads lineq = A (mA x n,
 * column-major, ldA >= mA; A may be NULL when mA == 0).  xlow/xupp stay on the Julia side (only the callers use them). */
int32_t bh_proj_create(bh_proj** out, const double* A, int64_t mA, int64_t n, int64_t ldA);
/* Must be called after every change of lincons.fixvars / lincons.chol (active_bounds!, add_active!, update_chol! —
 * src/polyhedral_constraints.jl:62-68,203-261).  fix_chunks = BitVector.chunks (bit i%64 of word i/64 <=> variable i fixed).
 * L = lincons.chol factor, mpp x mpp column-major, ONLY the lower triangle (i >= j) is read;
 * mpp must equal mA + popcount(fix) (or mA when nothing is fixed).  With mA == 0 the factor is the identity and L may be NULL. */
int32_t bh_proj_set_active(bh_proj* P, const uint64_t* fix_chunks, int64_t n,
                           const double* L, int64_t mpp, int64_t ldL);
int32_t bh_proj_destroy(bh_proj* P);
int32_t bh_proj_shape(const bh_proj* P, int64_t* mA, int64_t* n, int64_t* n_fixed);
/* projection!(lincons, r, v) / projection(lincons, r) — src/polyhedral_constraints.jl:150-170
 * (projection_nullspace! :104-118 when nothing is fixed, projection_subspace! :120-136 otherwise). */
int32_t bh_project(bh_proj* P, const double* r, double* v_out);
int32_t bh_project_dev(bh_proj* P, const double* r_dev, double* v_out_dev);
/* left_mul(lincons, x) — src/polyhedral_constraints.jl:86-98:  out (mpp) = [A x ; x[fixvars]]. */
int32_t bh_left_mul(bh_proj* P, const double* x, double* out_mpp);
/* left_mul_tr(lincons, y) — src/polyhedral_constraints.jl:72-84:  out (n) = A'y[1:mA] (+ scatter y[mA+1:end]). */
int32_t bh_left_mul_tr(bh_proj* P, const double* y, double* out_n);

/* ---- projected_cg -------------------------------------------------------- */

/* projected_cg(g_minor, H, w_l, w_u, lincons, kappa2; atol) — src/basic_tralcnlss.jl:690-764, with
 * factor_to_boundary — :793-809 — evaluated on the device.  The whole loop (H*p, dots, updates, projection, branch
 * scalars, exit test) is device-resident; the host only polls a done flag.
 *   atol_negcurv = sqrt(eps) (:697),  atol_f2b = 1e-10 (:798).
 *   status: BH_CG_*;  iters: the reference's `iter` variable at exit (starts at 1);
 *   trace (optional, may be NULL): row k = {pHp, alpha, gamma, rtv} of the k-th H*p product, trace_cap rows.
 *   n_hmul (optional): number of H*p products performed. */
int32_t bh_pcg(bh_hess* H, bh_proj* P, const double* g_minor, const double* w_l, const double* w_u,
               double kappa2, double atol_negcurv, double atol_f2b,
               double* w_out, int32_t* status, int32_t* iters,
               double* trace, int64_t trace_cap, int32_t* n_hmul);
int32_t bh_pcg_dev(bh_hess* H, bh_proj* P, const double* g_minor_dev, const double* w_l_dev, const double* w_u_dev,
                   double kappa2, double atol_negcurv, double atol_f2b,
                   double* w_out_dev, int32_t* status, int32_t* iters,
                   double* trace, int64_t trace_cap, int32_t* n_hmul);
/* Tie log of the LAST projected_cg run on this handle (bh_pcg, bh_pcg_dev, bh_minor_iterate) — SURVEY.md §8(c): the loop's
 * branches (src/basic_tralcnlss.jl:725 pHp <= tol_negcurve, :727 |pHp| > tol, :735 alpha > gamma, :747 |rtv| < tol_cg) decide
 * status and iteration count, so a scalar within rounding of its threshold may legitimately flip against another
 * implementation.  tie_flags: BH_TIE_* bits of the tests that came within 1e-10 (relative) of their threshold;
 * first_tie_hmul: the H*p product at which that first happened (0 = never); min_margin / _kind / _hmul: the smallest
 * relative distance |a-b|/max(|a|,|b|) any of those tests had in the call, which test, and at which product. */
#define BH_TIE_NEGCURV      1   /* :725 */
#define BH_TIE_NEGCURV_ABS  2   /* :727 */
#define BH_TIE_BOUND        4   /* :735 */
#define BH_TIE_TOL          8   /* :747 */
int32_t bh_pcg_tie_info(const bh_hess* H, int32_t* tie_flags, int32_t* first_tie_hmul, double* min_margin,
                        int32_t* min_margin_kind, int32_t* min_margin_hmul);

/* ---- callers of projected_cg, device-resident (SURVEY.md §8 a9, a10 and "next" row f-2) ----------------- */

/* minor_iterate(x, s, g_model, H, lincons, delta, kappa2) — src/basic_tralcnlss.jl:649-675: builds w_l/w_u exactly as :660-665
 * (only the FIXED variables get finite bounds), runs projected_cg (:667) and, unless the status is
 * negative_curvature, linesearch and w .= alpha*w (:669-672) — one call, no intermediate PCIe round trips.
 * xlow/xupp = lincons.xlow/xupp.  alpha_out (optional) receives the line-search factor (NaN when it was skipped).
 * The line search's w'Hw is taken from H*w accumulated inside the CG loop (option "ls_from_cg", default 1) instead of a
 * separate vthv(H,w) sweep; same value up to rounding. */
int32_t bh_minor_iterate(bh_hess* H, bh_proj* P, const double* x, const double* s, const double* g_model,
                         const double* xlow, const double* xupp, double delta, double kappa2,
                         double atol_negcurv, double atol_f2b, double* w_out, int32_t* status, int32_t* iters,
                         int32_t* n_hmul, double* alpha_out);
/* linesearch(g_model, H, w, w_l, w_u, lincons.fixvars) — src/basic_tralcnlss.jl:766-791. */
int32_t bh_linesearch(bh_hess* H, bh_proj* P, const double* g_model, const double* w, const double* w_l, const double* w_u,
                      double* alpha_out);
/* cauchy_step(x, g, H, chol_aat, lincons, delta) — src/basic_tralcnlss.jl:574-639 (with next_breakpoint :536-562 and the
 * initial active_bounds!, src/polyhedral_constraints.jl:203-215), device-resident ("next" row f-3).  Per breakpoint: one
 * H*d, one projection, and a rank-one Gram downdate + mA x mA Cholesky on the device in place of the reference's O(p^3)
 * add_active! -> cholesky_aug_aat rebuild.  Needs the reduced projection form (default).  On return the handle holds the
 * final active set; fix_chunks_out (ceil(n/64) words, optional) receives it in BitVector.chunks layout so the caller can
 * update lincons.fixvars (and its own factor, if it still needs one). */
int32_t bh_cauchy_step(bh_hess* H, bh_proj* P, const double* x, const double* g, const double* xlow, const double* xupp,
                       double delta, double* s_out, uint64_t* fix_chunks_out, int32_t* n_breakpoints, int32_t* n_hmul);
/* Form and launch count of the last bh_cauchy_step(_dev) on this bh_proj:
 *   form 0 = one H*d per breakpoint, 1 = row space of J (box), 2 = row space of J with equalities, 3 = from G in one launch,
 *   form 4 = from G with linear equalities (option "cauchy_gram_eq")
 *   form 5 = from G in one sorted sweep (bh_hess_set_cauchy_search at BH_CAUCHY_SORTED): the same few launches for every search length
 *   form 6 = from J in one sorted sweep (bh_hess_set_cauchy_rows at BH_CAUCHY_ROWS_SORTED): the same few launches for every search length;
 *            on a row-sharded handle only with bh_hess_set_cauchy_rows_ranks, one all-reduce per search (over the peer buffers the
 *            exchange is one launch more, counted in n_launches)
 *   n_launches = kernels enqueued by that call (over-launched prologue-only passes included).
 * BH_ERR_PRECONDITION before the first search on the handle. */
int32_t bh_cauchy_info(const bh_proj* P, int32_t* form, int32_t* n_launches);
/* g = Jx'*rx + Cx'*y_bar — src/basic_tralcnlss.jl:45 (new_point), :74 (first_derivatives); r = this rank's d rows, y_bar has q entries. */
int32_t bh_grad(bh_hess* H, const double* r, const double* ybar, double* g_out);
/* dot(rx,rx) of the augmented-Lagrangian value mx = 0.5*dot(rx,rx) + dot(y,cx) + 0.5*mu*dot(cx,cx) — src/basic_tralcnlss.jl:44
 * (new_point) and :58 (evaluate_al).  r = this rank's d rows of the residual; the ranks' partial sums are all-reduced in rank
 * order, so out is the GLOBAL squared norm, bit-identical on every rank (with one rank: plain dot(r,r)).  Row-sharded callers
 * need it to keep the replicated trust-region control flow (rho = ared/pred, :353-358) in lock-step. */
int32_t bh_resid_sqnorm(const double* r, int64_t d, double* out);
/* g_minor = H*s + g — src/basic_tralcnlss.jl:412,:437. */
int32_t bh_hmul_add(bh_hess* H, const double* s, const double* g, double* out_n);

/* ---- the minor loop of inner_step with its vectors resident in HBM --------------------------------
 * src/basic_tralcnlss.jl:410-458: s = cauchy_step(...); g_minor = H*s+g; while ...: w = minor_iterate(...); s .+= w;
 * g_minor = H*s+g; active_bounds / add_active!; norm_reduced_gradient x 2; ...; model_reduction.  Every *_dev entry point takes
 * and returns DEVICE pointers for the n-vectors (x, s, g, g_minor, w, xlow, xupp); only scalars, counts and the n/8-byte
 * BitVector image of the active set cross PCIe (bh_stats' h2d/d2h counters let a caller check that).  A caller that owns the
 * loop (julia/BEnlsipHIP.jl's inner_step method; tests/hip_ops.py::DeviceResidentInnerStep) uploads x, g and the bounds once
 * per trust-region iteration and downloads s once. */
int32_t bh_cauchy_step_dev(bh_hess* H, bh_proj* P, const double* x_dev, const double* g_dev, const double* xlow_dev,
                           const double* xupp_dev, double delta, double* s_out_dev, uint64_t* fix_chunks_out /* host, optional */,
                           int32_t* n_breakpoints, int32_t* n_hmul);
int32_t bh_minor_iterate_dev(bh_hess* H, bh_proj* P, const double* x_dev, const double* s_dev, const double* g_model_dev,
                             const double* xlow_dev, const double* xupp_dev, double delta, double kappa2, double atol_negcurv,
                             double atol_f2b, double* w_out_dev, int32_t* status, int32_t* iters, int32_t* n_hmul, double* alpha_out);
int32_t bh_linesearch_dev(bh_hess* H, bh_proj* P, const double* g_model_dev, const double* w_dev, const double* w_l_dev,
                          const double* w_u_dev, double* alpha_out);
/* r_dev = this rank's d residual rows in HBM (a device-side residual callback); y_bar (q entries) stays a host vector. */
int32_t bh_grad_dev(bh_hess* H, const double* r_dev, const double* ybar, double* g_out_dev);
int32_t bh_hmul_add_dev(bh_hess* H, const double* s_dev, const double* g_dev, double* out_n_dev);
/* s .+= w ; g_minor = H*s + g — src/basic_tralcnlss.jl:436-437 (s_dev is updated in place).
 * Under options "step_from_cg" and "free_image_chain", right behind a bh_minor_iterate_dev that was served from the compact image of
 * the free columns, g_minor_out_dev holds H*s + g on the FREE variables only afterwards: its entries on the fixed variables keep the
 * value they had (see "free_image_chain" below). */
int32_t bh_step_accumulate_dev(bh_hess* H, double* s_dev, const double* w_dev, const double* g_dev, double* g_minor_out_dev);
/* src/basic_tralcnlss.jl:439-453 on the device-side active set:
 *     active_indx = active_bounds(lincons, x, s, delta)                      src/polyhedral_constraints.jl:219-237 (atol = sqrt(eps))
 *     if mA + |active_indx| <= n:  add_active!(lincons, chol_aat, active_indx)    poly:252-261      -> *branch = 0
 *     else:                        active_bounds!(lincons, x+s, chol_aat)         poly:203-215      -> *branch = 1
 * Newly fixed variables leave A_free A_free' through a Gram DOWNDATE over their columns followed by the mA x mA factorisation
 * (the reference rebuilds the (mA+p) x (mA+p) augmented factor from scratch, O(p^3)).  n_at_bound = |active_indx|,
 * n_fixed = count(fixvars) afterwards; fix_chunks_out (host, optional, ceil(n/64) words) receives the new lincons.fixvars.chunks. */
int32_t bh_proj_update_active_dev(bh_proj* P, const double* x_dev, const double* s_dev, const double* xlow_dev, const double* xupp_dev,
                                  double delta, double atol, int32_t* n_at_bound, int32_t* n_fixed, int32_t* branch,
                                  uint64_t* fix_chunks_out);
/* norm_reduced_gradient(g, lincons) = norm(projection(lincons, -g)) — src/basic_tralcnlss.jl:869-875 (also criticality_measure :839). */
int32_t bh_reduced_gradient_norm_dev(bh_proj* P, const double* g_dev, double* out);
/* model_reduction = dot(g,s) + 0.5*vthv(H,s) — src/basic_tralcnlss.jl:458. */
int32_t bh_model_reduction_dev(bh_hess* H, const double* g_dev, const double* s_dev, double* out);

/* factor_to_boundary(p, w, w_l, w_u; atol) — src/basic_tralcnlss.jl:793-809, stand-alone (tests). */
int32_t bh_factor_to_boundary(const double* p, const double* w, const double* w_l, const double* w_u,
                              int64_t n, double atol, double* gamma_out);

/* ---- plumbing ------------------------------------------------------------ */
int32_t bh_dev_alloc(void** out, int64_t bytes);
int32_t bh_dev_free(void* p);
int32_t bh_dev_upload(void* dst_dev, const void* src_host, int64_t bytes);
int32_t bh_dev_download(void* dst_host, const void* src_dev, int64_t bytes);
int32_t bh_stats(bh_hess* H, bh_stats_t* out);
int32_t bh_stats_reset(bh_hess* H);
/* Tuning knobs; unknown keys return BH_ERR_INVALID_ARG.  Defaults in brackets.  (A key whose A/B experiment is decided leaves
 * this list together with the losing path, and is an unknown key from then on.)
 *   "proj_form"      [1] 1 = reduced mA x mA projection (factor built on the device), 0 = the reference's augmented form
 *                        (needs the caller's factor in bh_proj_set_active).  Any non-zero value is 1.  Environment: BH_PROJ_FORM
 *                        (read by bh_init, likewise)
 *   "pcg_batch"      [0] CG iterations enqueued per launch-ahead batch; 0 = by problem size (1 when an H*p streams >= 100 us).
 *                        A negative value is 0.  Environment: BH_PCG_BATCH (read by bh_init, likewise)
 *   "fold_init"      [1] box constraints: fold projected_cg's initialisation into the first H*p / step launches
 *   "cg_fused"       [1] shape of a CG iteration.  1 (default): box constraints in two kernels (the H*p launch forms p and takes the
 *                        exit test, one kernel reduces the slabs — exchanging them between the ranks of a peer-buffer communicator —
 *                        and updates w, r, v; over RCCL: two kernels + the collective, the update of the previous iteration
 *                        living in the prologue of the H*p launch); linear equalities (reduced form, mA <= 64, one rank) in
 *                        three kernels (H*p, reduce/update, projection with the explicit inverse of the reduced factor).
 *                        2: linear equalities in four kernels (triangular solves in a launch of their own); box as 1.
 *                        0: the round-1 shapes (three kernels box, seven with equalities; p'Hp = dot(p, H*p) exactly as the
 *                        reference forms it, where 1 and 2 form it as sum_i w_i (Jp)_i^2).  Another value: BH_ERR_INVALID_ARG.
 *                        Environment: BH_CG_FUSED (read by bh_init; a value outside 0..2 is taken to its nearest end)
 *   "final_sync"     [0] device-pointer entry points (*_dev): 1 = always drain the library stream before returning, as the
 *                        host-pointer entry points do.  0 = return as soon as everything the HOST is owed has arrived; results
 *                        that stay in HBM are ordered on the library stream (later calls see them; bh_synchronize, or sharing
 *                        the caller's stream through bh_set_stream, orders them for anybody else):
 *                        - bh_pcg_dev: when the caller's device vectors are used in place and the loop was stopped by its exit
 *                          test (solved / iterations exhausted), w was complete before the launch that reported the stop began,
 *                          and only prologue-only launches that write nothing are still in flight (saves ~10 us per call);
 *                        - bh_minor_iterate_dev, bh_reduced_gradient_norm_dev, bh_model_reduction_dev, bh_proj_update_active_dev,
 *                          bh_cauchy_step_dev: counts, norms, alpha and the BitVector image come back through a host-mapped
 *                          mailbox page the kernels write and seal with a sequence number (no DMA per scalar, no stream
 *                          synchronize: 84 -> 28 us for bh_proj_update_active_dev, 25 -> 11 us for a reduced-gradient norm);
 *                        - bh_hmul_dev, bh_hmul_add_dev, bh_step_accumulate_dev, bh_jv_dev, bh_jtv_dev, bh_project_dev owe the
 *                          host nothing and return once their work is enqueued.
 *                        A caller's device vector is read where it lies when it needs no padding (n a multiple of 16, 16-byte
 *                        aligned); every other case, and every host-pointer entry point, behaves as before.
 *                        Any non-zero value is 1.  Environment: BH_FINAL_SYNC (read by bh_init, likewise)
 *   "host_copy_kernels" [1] host-pointer entry points: the caller's vectors travel between the pinned arena and HBM by a small
 *                        copy kernel on the mapped arena instead of a DMA engine transfer, and the call ends with a mailbox seal +
 *                        poll instead of hipStreamSynchronize (bh_pcg 0.660 -> 0.652 ms, bh_minor_iterate 0.693 -> 0.665 ms,
 *                        bh_project 31 -> 21 us on the config-3 instance); 0 = DMA + synchronize (round 1).  Any non-zero value
 *                        is 1.  Environment: BH_HOST_COPY_KERNELS (read by bh_init, likewise)
 *   "ls_from_cg"     [1] bh_minor_iterate: w'Hw of the line search from the H*w the CG loop accumulated (0: explicit vthv)
 *   "step_from_cg"   [0] opt-in (the resident inner-step mirrors set it around their loop): bh_step_accumulate_dev called right
 *                        behind the bh_minor_iterate_dev that produced its w (same handle,
 *                        w_dev = that call's w_out_dev, g_minor_out_dev = that call's g_model_dev, which holds H*s + g as in
 *                        src/basic_tralcnlss.jl:412,:434-437): g_minor += H*w with the H*w that CG loop accumulated instead of a
 *                        fresh sweep H*(s + w) + g over J (same value, rounded differently; one H-product less per minor
 *                        iterate).  It trusts the caller's invariant that g_minor_out_dev holds H*s + g for the CURRENT s.
 *                        Under the same option bh_model_reduction_dev(H, g, s) takes s'Hs = s.(g_minor - g) from the g_minor the
 *                        library last wrote for exactly these H, s, g (bh_hmul_add_dev / bh_step_accumulate_dev) instead of a J v sweep.
 *                        0, or any other calling pattern: the explicit product.  Needs "ls_from_cg" = 1.
 *                        After a bh_hess_set_mu that changes mu, the next bh_step_accumulate_dev and bh_model_reduction_dev on that
 *                        handle recompute from J.
 *   "chol_downdate"  [0] bh_cauchy_step, per breakpoint: 0 = downdate the Gram matrix and refactor (as accurate as the reference's
 *                        from-scratch rebuild), 1 = for mA > 64 only: rank-one downdate of the factor itself (O(mA^2)), rebuilt from
 *                        scratch every 8th breakpoint (errors accumulate in between; up to 64 rows the refactoring path is as fast)
 *   "cauchy_image"   [1] bh_cauchy_step with box constraints on one rank: search in the row space of J (J d and J s_c maintained by
 *                        one-column updates; d'Hd = ||J d||^2_W, s'Hd = (J s).(J d)_W: the same numbers as dot(d, H*d), dot(s, H*d),
 *                        rounded differently): one J v sweep at the start instead of one H*d sweep per breakpoint.  0: as the reference
 *   "cauchy_image_max_ma" [64] ... and with up to this many linear equalities (0..64): there the row-space form keeps a = J D g and
 *                        B = J D A' (rows x mA) next to J d, J s_c — two sweeps over J up front (a: J v; B: "cauchy_gemm"), one
 *                        column of J per breakpoint afterwards; above this value and up to 64 rows the form is used when the
 *                        previous search on the same bh_proj took more than 4 (1 + mA) passes
 *   "cauchy_fused"   [1] that search (box constraints, one rank) with ONE kernel per breakpoint: every workgroup of the row kernel redoes the
 *                        previous pass's decision in its prologue (s_c and the loop state are ping-pong buffers); 0: two kernels per pass
 *   "cauchy_image_refresh" [0] that row-space search ("cauchy_image", with or without equalities) on one rank: R >= 1 forms the carried images
 *                        again from J and the device-side state at every pass index that is a positive multiple of R (the reference forms
 *                        a fresh H*d at every breakpoint; the carried J d keeps an absolute error of k eps ||J d_0|| while ||d|| shrinks
 *                        by orders of magnitude).  0 = never: every path, launch, counter and bit is what it is without the option.
 *                        "cauchy_fused" = 1: a decision-only launch of cauchy_fused_kernel + cauchy_reform_kernel (J d and J s_c in ONE
 *                        sweep, two right-hand sides; n <= 16384 — a wider J keeps its carried images); "cauchy_fused" = 0: two gated
 *                        J v sweeps; with equalities: a (J v), B (the GEMM of "cauchy_gemm", else mA sweeps) and J s_c (J v).
 *                        Not a change of the search: same decisions rule, same passes; a fresh product is rounded differently from the
 *                        carried one, hence opt-in.  Re-formations enqueued behind the end of the loop are gated off and not counted:
 *                        with m = floor((passes - 1) / R), stats.n_jv of a search grows by 1 + m ("cauchy_fused" = 1), 1 + 2 m
 *                        ("cauchy_fused" = 0), with equalities 1 + 2 m ("cauchy_gemm" = 1) or 1 + mA + (2 + mA) m; n_hmul of the call
 *                        (the passes) and n_breakpoints keep their meaning, bh_cauchy_info's form too (its launch count includes the
 *                        extra launches).  Several ranks: ignored, the path is exactly the one without the option.
 *                        A negative value: BH_ERR_INVALID_ARG
 *   "cauchy_block"   [0] that search with "cauchy_fused" = 1 (box constraints, one rank, "cauchy_image_refresh" = 0, n <= 4096): K = 2, 4,
 *                        8 or 16 breakpoints per launch.  With box constraints the row update of a pass needs only theta and the index
 *                        fixed, which follow from the n-vectors; the two sums merely decide whether the search stops there.  So a
 *                        launch runs K advances ahead (cauchy_block_kernel<K>: K column updates of its rows from registers, K pairs of
 *                        partial sums) and the next launch checks the K decisions in order; at most K - 1 advances are thrown away,
 *                        once, at the end.  Same operations in the same order per row and per sum: the step, the active set, n_hmul
 *                        (passes), n_breakpoints and stats.n_jv (+ 1) are those of 0, bit for bit; bh_cauchy_info reports form 1 and
 *                        about passes / K + 2 launches of the search instead of passes + 1.  0, 1 = one breakpoint per launch; any
 *                        other case (equalities, several ranks, "cauchy_fused" = 0, a re-formation interval, n > 4096, a Gram-form
 *                        search) takes exactly the path it takes with 0.  Any other value: BH_ERR_INVALID_ARG, the option keeps its
 *                        value.  Environment: BH_CAUCHY_BLOCK (read by bh_init; a value outside the list is ignored)
 *   "cauchy_gram"    [0] bh_cauchy_step(_dev) on a handle in the Gram form (bh_hess_set_form), no linear equalities, one rank: the whole
 *                        search in ONE launch from G (init -> G d -> cauchy_gram_kernel: Hd downdated by one row of G per breakpoint, the
 *                        loop runs on the device; the launch count does not depend on the number of breakpoints).  Any other handle or
 *                        constraint set takes the path it takes with 0.  bh_cauchy_info tells which form ran
 *   "cauchy_gram_eq" [0] bh_cauchy_step(_dev) on a handle in the Gram form with 1..64 linear equalities, one rank, lineq image with the
 *                        handle's leading dimension: the linear-equality search in the column space of G (form 4) — a = G D g and
 *                        B = G D A' from one G v launch and one GEMM over n rows, one contiguous row of G per breakpoint, three launches
 *                        per pass, a and B formed again every 128th pass; stats.n_hmul grows by those G v launches, n_jv by nothing.
 *                        Values 0 / 1 (another value: BH_ERR_INVALID_ARG).  Independent of "cauchy_gram", "cauchy_image" and
 *                        "cauchy_image_max_ma".  Any other handle or constraint set takes the path it takes with 0
 *   "gram_cg_fused"  [0] bh_pcg*, bh_minor_iterate* on a handle in the Gram form (one rank by construction), independent of "cg_fused":
 *                        TWO kernels per CG iteration with box constraints (gram_cg_kernel: G·v with p_j, beta and the exit test formed
 *                        in its prologue, H*p stored as one vector next to per-workgroup partials of dot(p, H*p); then
 *                        cg_reduce_update_kernel), THREE with up to 64 linear equalities in the reduced projection form (+
 *                        proj_apply_linv_kernel).  Any other case (mA > 64, proj_form = 0, nothing free, g not readable to the padded
 *                        length) and every call with 0 takes the separate-kernel shape.  stats.cg_kernels tells which shape ran.
 *                        Switching it on needs bh_init (BH_ERR_NOT_INIT otherwise); values other than 0 / 1: BH_ERR_INVALID_ARG
 *   "linv_refine"    [1] three-kernel CG iteration with linear equalities (cg_fused = 1): one step of iterative refinement behind the
 *                        explicit inverse of the factor (rho = t - A_free A_free' y, y += L^-T L^-1 rho), so that A_free v stays at the level
 *                        of the reference's two triangular solves also for ill-conditioned A_free A_free' (0: plain explicit inverse;
 *                        not applied with a single equality, where the factor is a scalar)
 *   "cauchy_gemm"    [1] B = J D A' in ONE sweep over J on the fp64 matrix cores (a tall-skinny GEMM: M = rows of J, N = mA, K = n);
 *                        0: mA J v sweeps over the masked rows of A
 *   "gram_mfma"      [1] A_free A_free' on fp64 MFMA when mA > 96 (2: always, 0: never)
 *   "blocks_per_cu"  [0] workgroups per CU of the row-streaming kernels (0: per-geometry default).  Accepts 0..8 (the partial-slab
 *                        buffers hold 8 workgroups per CU); anything else is BH_ERR_INVALID_ARG.  Environment: BH_BLOCKS_PER_CU (read by
 *                        bh_init; a value outside the range is taken to its nearest end)
 *   "comm_path"      [0 with BH_COMM=rccl|both, 1 with BH_COMM=ipc] which communicator carries the all-reduces: 0 = RCCL,
 *                        1 = the one-shot peer-buffer exchange fused into the slab reduction (needs BH_COMM=ipc or both)
 *   "profile"        [flags of bh_init] 1 = hipEvents around every profile_stride-th H*p launch (bh_stats: hmul_ms / hmul_timed)
 *   "image_pool"     [2] Jacobian images of destroyed handles kept for the next bh_hess_create* of a similar size (0..8; 0 frees at
 *                        once).  The reference builds a new AlHessian per accepted step and drops the old one: recycling the
 *                        2 GiB image avoids the driver's background scrub of freed VRAM and a ~4 ms hipMalloc per step.
 *   "upload_chunk_mb" [64] bh_hess_create_async: MiB of J per pipelined column chunk (1..4096)
 *   "free_image"     [1] bh_pcg*, box constraints (no linear equalities) on one rank, implicit form, two-kernel iteration ("cg_fused"),
 *                        n <= 16384, atol_f2b > 0: the CG loop streams a compact image of the FREE columns of J instead of J — every p_j is
 *                        zero on the fixed variables and their entries of H*p are used for nothing, so nfix / n of every sweep is saved.
 *                        The image belongs to the handle ((d + q) x (n - nfix) doubles from the image pool) and follows an active set
 *                        that grows by moving single columns; a freed variable makes it stale until it is built again.
 *                        1 = by a policy: every eligible call earns n_hmul * nfix / n sweeps of credit, the image is built at the start
 *                        of the next eligible call once the credit has reached the cost of a build, and newly fixed variables are moved
 *                        out when that costs less than the saving predicted from the previous call (else that call streams J);
 *                        2 = built at the first eligible call, moves always applied (tests, A/B runs); 0 = off.  A failed allocation
 *                        leaves the handle on the full image without an error.  status, iters, n_hmul, the trace and the tie log keep
 *                        their meaning; w is exactly 0 on the fixed variables; p'Hp and r.v are summed in the order of the compact
 *                        columns (another rounding than on the full image).  A non-finite g on a fixed variable: the call runs on the
 *                        full image.  Linear equalities, several ranks and the Gram form are never eligible; bh_minor_iterate* with
 *                        "ls_from_cg" = 1 (it wants H*w) is eligible only under "free_image_minor".  bh_hess_free_image_info reports
 *                        what the handle holds.  Another value: BH_ERR_INVALID_ARG.
 *                        (The environment variable BH_FREE_IMAGE, read by bh_init, sets the initial value.)
 *   "free_image_minor" [0] 1 = a bh_minor_iterate* call with "ls_from_cg" = 1 is considered for the compact image by the rules and the
 *                        policy of "free_image" (0 off, 1 by the policy, 2 always), provided "step_from_cg" = 0 at the time of the call:
 *                        the line search's w'Hw is then the only reader of the accumulated H*w, and w is zero on the fixed variables,
 *                        so the CG loop accumulates the FREE part of H*w in slot order and the line search (free_image_linesearch_kernel)
 *                        runs on the compact operands, delivering the scaled w through the slot -> column map.  g.w and w'Hw are summed in
 *                        the order of the compact columns.  w stays +0 on the fixed variables whatever alpha is (on the full image a
 *                        negative or non-finite alpha leaves alpha * 0 = -0 or NaN there).  After such a call bh_step_accumulate_dev
 *                        always recomputes H*s + g (the fixed part of H*w was never formed), also when "step_from_cg" is switched on
 *                        in between.  A call handed back to the full image (non-finite g on a fixed variable) is today's in every bit.
 *                        With "step_from_cg" = 1 (the resident inner-step chain) the call stays on the full image
 *                        (unless "free_image_chain" is on).  calls_served of
 *                        bh_hess_free_image_info counts these calls too.  0 = bh_minor_iterate* with "ls_from_cg" = 1 never touches the
 *                        image.  Another value: BH_ERR_INVALID_ARG.
 *   "free_image_chain" [0] 1 = the same for a bh_minor_iterate* call made with "step_from_cg" = 1 (the resident inner-step chain), by
 *                        the same rules, policy and hand-back: the line search (free_image_linesearch_scale_hw_kernel) also keeps the
 *                        FREE part of H*w scaled with w, and the bh_step_accumulate_dev right behind a bh_minor_iterate_dev that was
 *                        served from the image adds it to g_minor through the slot -> column map
 *                        (free_image_step_accumulate_kernel): no sweep over J, stats.n_hmul and n_jv unchanged.
 *                        DEVIATION: after such a call g_minor_out_dev holds H*s + g ON THE FREE VARIABLES ONLY; its entries on the
 *                        fixed variables keep the value they had.  Nothing inside an inner step reads them (the next CG loop and
 *                        bh_reduced_gradient_norm_dev mask them; the active set only grows while one J lives).  The model value
 *                        g.s + s'Hs / 2 cannot be taken from such a g_minor, so it is carried from step to step on the device
 *                        (q(s + w) = q(s) + w.g_minor + w'Hw / 2 over the free slots, started from the g_minor the library wrote by
 *                        bh_hmul_add_dev for exactly these H, s, g) and bh_model_reduction_dev returns the carried value without a
 *                        launch over J; where no value could be carried (g_minor was not the library's own) it takes its J v sweep.
 *                        A full-image minor iterate inside such a chain (the policy refused a move) keeps today's two vector
 *                        launches and carries q by one small launch in front of them.  Any other calling pattern (another w, a second
 *                        accumulate, a bh_pcg* or a minor iterate on any handle in between) recomputes H*s + g over all variables.
 *                        Independent of "free_image_minor".  0 = every path, launch, counter and bit is what it is without the
 *                        option.  Another value: BH_ERR_INVALID_ARG.
 *   "free_image_eq"  [0] 1 = a bh_pcg* call with linear equalities is considered for the compact image by the rules and the policy of
 *                        "free_image" (0 off, 1 by the policy, 2 always) when it takes the three-kernel iteration ("cg_fused" = 1, the
 *                        reduced projection form, mA <= 64) on one rank in the implicit form with atol_f2b > 0 and no H*w wanted.  The
 *                        handle then also keeps Af, the mA x ldf image of the lineq matrix in the slot order of the compact image,
 *                        formed again by one launch whenever the constraint handle or its active set is another than the one it was
 *                        formed for (never moved; its launch is not part of the policy's costs).  The loop is the one of the full
 *                        image on compact operands: in every bit the call a fresh pair of handles makes on the columns of the free
 *                        variables in slot order, nothing fixed.  w is exactly 0 on the fixed variables.  A non-finite g on a fixed
 *                        variable: the call runs on the full image.  bh_minor_iterate* with an H*w buffer, "cg_fused" = 2, the
 *                        seven-kernel shape, mA > 64, the augmented form, the Gram form and several ranks stay on the full image.
 *                        stats.bytes_per_hmul, bh_time_kernel kind 0 and bh_hess_free_image_info report these calls as they report
 *                        box-constrained ones.  0 = every path, launch, counter and bit is what it is without the option.
 *                        Another value: BH_ERR_INVALID_ARG.  (The environment variable BH_FREE_IMAGE_EQ, read by bh_init, sets
 *                        the initial value.)
 *   "gram_ingest"    [0] bh_hess_create_async on one rank with n <= 16384: 1 = the handle is born in the Gram form and G is built during
 *                        the upload, block rows of G as their columns land (see bh_hess_create_async).  Several ranks or n > 16384: the
 *                        call is what it is with 0 (an implicit handle).  Read when the handle is created; no effect on
 *                        bh_hess_create, bh_hess_create_dev, bh_hess_create_synthetic, bh_hess_set_form or bh_hess_set_mu.
 *                        Values 0 / 1 (another value: BH_ERR_INVALID_ARG)
 *   "profile_stride" [8] >= 1; an event pair costs ~10 us of stream time, so 1 is for short runs only (at most 512 samples per call) */
int32_t bh_set_option(const char* key, int64_t value);
/* Time `reps` back-to-back launches of one kernel class with hipEvents on the launch stream.
 * kind: 0 = fused J'(Jp) over the image the handle's CG loop streams now (the compact image of option "free_image" once the handle
 * holds one, else J), 1 = J·v, 2 = J'·u; 3..6 = read-only stream probe over the same image (nothing but 16-byte
 * non-temporal loads and adds) with 1, 2, 4, 8 workgroups per CU: the practical single-read ceiling the kernels are
 * quoted against; 7 = the all-reduce of one n-vector on the active communicator path (every rank must call it together);
 * 8 = everything an H*p does after its streaming kernel (slab reduction + all-reduce; without a communicator: the slab
 * reduction alone); 9 = a build of the Gram matrix G (each one counted by bh_hess_get_form), 10 = the product G·v the handle
 * performs now (one launch over all of G, or under BH_GRAM_READ_LOWER the lower-triangle launch and the slab reduction),
 * 11 = one quadratic form v'Gv from the lower triangle of G with its scalar reduction (whatever the handle's read mode;
 * BH_ERR_PRECONDITION when the width is not served) — all three BH_ERR_PRECONDITION unless the handle is in the Gram form
 * (bh_hess_set_form); the counters of bh_hess_get_gram_read do not move.  Returns the average milliseconds per launch. */
int32_t bh_time_kernel(bh_hess* H, int32_t kind, int32_t reps, double* avg_ms);
/* Device self-test of the wave64 DPP/permlane reduction network (sum and NaN-propagating min). */
int32_t bh_selftest(void);

#ifdef __cplusplus
}
#endif
#endif /* BENLSIP_HIP_H */
