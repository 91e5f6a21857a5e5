// bh_cgfuse_body.hip.h — the statements of cg_reduce_update_kernel, included INSIDE a kernel's braces (bh_cgfuse.hip.h; no
// include guard on purpose).  The including kernel provides: CgUpdArgs a, PeerArgs pa, constexpr bool GEN, PEER, SCAT.
    CgState* st = a.st;
    if (st->stop_at != 0 && a.j > st->stop_at) return;
    if (a.reroute != nullptr && *a.reroute == a.reroute_seq) return;
    __shared__ double2 sm[16][17];
    __shared__ double rvs[16];
    __shared__ double2 rsm[16];                  // GEN: the masked new r of this workgroup's 16 chunks
    const int tid = threadIdx.x, cl = tid & 15, rl = tid >> 4;
    const int c = blockIdx.x * 16 + cl;
    const bool valid = c < a.nchunks;
    const int64_t ld2 = a.ld >> 1;
    const double QNAN = __longlong_as_double(0x7ff8000000000000ll);

    // ---- every load the kernel needs goes out first: the iteration's partial sums, this workgroup's slab rows, its vector
    //      entries.  The kernel is latency-bound (a few hundred bytes per thread); issued one reduction at a time the same
    //      loads cost ~15 dependent memory round trips, issued together ~2.
    const bool upd = (rl == 0) && valid;                       // the 16 threads that update this workgroup's 16 chunks
    const bool from_g = (a.j == 1 && !a.init_in_memory);      // r = g_minor (:705), w = 0 (:702)
    double2 pk = make_double2(0.0, 0.0), wk = pk, hwk = pk, rk = pk;
    int2 fr = make_int2(-1, -1);
    if (upd) {
        pk = reinterpret_cast<const double2*>(a.p)[c];
        if (from_g) {
            rk = reinterpret_cast<const double2*>(a.g)[c];
        } else {
            rk = reinterpret_cast<const double2*>(a.r)[c];
            wk = reinterpret_cast<const double2*>(a.w)[c];
            if (a.hw != nullptr) hwk = reinterpret_cast<const double2*>(a.hw)[c];
        }
    }
    TieRegs tr;                                                // (uniform: every thread holds the log, one of them commits it)
    tr.load(st);
    const int max_iter = st->max_iter;
    const double rtv_state = st->rtv;                          // j == 1: written by the H*p launch
    LaneBatch<8> b_sq, b_gp, b_rv;
    b_sq.issue(a.sqpart, a.Gq);
    b_gp.issue(a.gpart, a.G);
    b_rv.issue(a.rvpart_in, a.nrv);                            // (j == 1: addressable, not used)
    const double2* P2 = reinterpret_cast<const double2*>(a.partials);
    const int cc = min(c, a.nchunks - 1);                      // out-of-range threads load a valid chunk and drop the result:
    SlabBatch sb;                                              // no branch around the loads (see LaneBatch::issue)
    sb.issue(P2, ld2, cc, rl, a.Gs);
    // GEN: this thread's entries of A for the partials of A_free r below (rows rl, rl + 16, ...; up to 64 rows), asked for now
    double2 arow[4];
    if (GEN) {
        const double2* A2 = reinterpret_cast<const double2*>(a.A);
        const int64_t ldA2 = a.ldA >> 1;
#pragma unroll
        for (int k = 0; k < 4; ++k) arow[k] = A2[(int64_t)min(rl + 16 * k, a.mA - 1) * ldA2 + cc];
    }
    int2 mp = make_int2(-1, -1);
    if (SCAT && upd && a.map != nullptr) mp = reinterpret_cast<const int2*>(a.map)[c];
    if (upd && a.fixrank != nullptr) fr = reinterpret_cast<const int2*>(a.fixrank)[c];   // last: its compare is scheduled next to it

    // ---- this workgroup's 32 columns of Hp = sum of the slabs (fixed order) --------------------------------------------
    const double2 acc = sb.fold(P2, ld2, cc, rl, a.Gs);
    sm[rl][cl] = acc;

    // ---- the iteration's scalars, recomputed by every wave from the partials (identical bits everywhere) -----------------
    double pHp = wave_sum(b_sq.fold_sum(a.sqpart, a.Gq));                               // :723 (this rank's rows)
    if (PEER) {
        __shared__ int s_timeout;
        __shared__ double2 xs[kMaxPeers][16];
        __shared__ double ps[kMaxPeers];
        if (tid == 0) s_timeout = 0;
        __syncthreads();                                    // sm[][] is complete
        // this rank's slab sum for the workgroup's 16 chunks
        if (rl == 0) {
            double2 t = sm[0][cl];
#pragma unroll
            for (int q = 1; q < 16; ++q) { t.x += sm[q][cl].x; t.y += sm[q][cl].y; }
            sm[15][cl] = t;
        }
        __syncthreads();
        const double2 mine = sm[15][cl];
        const unsigned long long seq = *pa.seq;
        const int par = (int)(seq & 1ull);
        const int64_t slot = ((int64_t)par * kMaxPeers + pa.rank) * pa.cap;
        const int64_t fidx = ((int64_t)par * kMaxPeers + pa.rank) * pa.nblk_cap + blockIdx.x;
        // push (write-through), drain, meet, raise the flags — as reduce_exchange_kernel
        if (rl < pa.nranks && valid) sys_store_f64x2(pa.slots[rl] + slot + 2 * (int64_t)c, mine);
        if (rl < pa.nranks && cl == 0) __hip_atomic_store(pa.scal[rl] + fidx, pHp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (rl < pa.nranks && cl == 0) __hip_atomic_store(pa.flags[rl] + fidx, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (rl < pa.nranks && cl == 0) {
            const unsigned long long* f = pa.flags[pa.rank] + ((int64_t)par * kMaxPeers + rl) * pa.nblk_cap + blockIdx.x;
            const unsigned long long t0 = wall_clock64();
            const bool dead = __hip_atomic_load(pa.dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
            if (dead) s_timeout = 1;
            while (!dead && __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != seq) {
                __builtin_amdgcn_s_sleep(8);
                if (wall_clock64() - t0 > pa.timeout_ticks) {
                    s_timeout = 1;
                    __hip_atomic_store(pa.err, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(pa.dead, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
        }
        asm volatile("" ::: "memory");
        __syncthreads();
        if (rl < pa.nranks) {
            double2 got = make_double2(0.0, 0.0);
            if (valid) got = sys_load_f64x2(pa.slots[pa.rank] + ((int64_t)par * kMaxPeers + rl) * pa.cap + 2 * (int64_t)c);
            xs[rl][cl] = got;
            if (cl == 0) ps[rl] = __hip_atomic_load(pa.scal[pa.rank] + ((int64_t)par * kMaxPeers + rl) * pa.nblk_cap + blockIdx.x,
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
        // sums over ranks in rank order; sm[0] then holds the global H*p columns and rows 1.. are zero for the code below
        double2 t = xs[0][cl];
        double ph = ps[0];
        for (int r = 1; r < pa.nranks; ++r) { t.x += xs[r][cl].x; t.y += xs[r][cl].y; ph += ps[r]; }
        if (s_timeout) { ph = __longlong_as_double(0x7ff8000000000000ll); }
        pHp = ph;
        __syncthreads();
        sm[rl][cl] = (rl == 0) ? t : make_double2(0.0, 0.0);
        // the last workgroup to get here advances the exchange counter (nobody reads it again in this launch)
        if (tid == 0) {
            const unsigned done = atomicAdd(pa.arrive, 1u) + 1u;
            if (done == gridDim.x) { *pa.arrive = 0u; *pa.seq = seq + 1ull; }
        }
    }
    const double gamma = wave_min(b_gp.fold_min(a.gpart, a.G));                        // :728 / :734
    const double rtv = (a.j == 1) ? rtv_state : wave_sum(b_rv.fold_sum(a.rvpart_in, a.nrv));   // :732
    int cont = 0, neg = 0, outside = 0;
    double step = 0.0, alpha = QNAN;
    bool add_w = true;
    if (pHp <= a.atol_neg) {                        // :725
        neg = 1;
        if (fabs(pHp) > a.atol_neg) step = gamma;   // :727-729
        else add_w = false;
    } else {
        alpha = __ddiv_rn(rtv, pHp);                // :733
        outside = alpha > gamma;                    // :735
        if (outside) step = gamma;                  // :737
        else { step = alpha; cont = 1; }            // :739
    }
    __syncthreads();

    // ---- update this workgroup's entries ----------------------------------------------------------------------------------
    double rv_part = 0.0;
    if (rl == 0 && valid) {
        double2 hp = sm[0][cl];
#pragma unroll
        for (int q = 1; q < 16; ++q) { hp.x += sm[q][cl].x; hp.y += sm[q][cl].y; }
        // Every vector here is either the caller's buffer with n == 2*nchunks or a zero-padded workspace vector: whole 16-byte
        // chunks are always addressable.  Elements at or beyond n are kept at exactly 0 (never updated: Inf*0 would poison them).
        const bool e0 = 2 * c < a.n, e1 = 2 * c + 1 < a.n;
        if (add_w) {
            wk.x = __dadd_rn(wk.x, __dmul_rn(step, pk.x));           // :729 / :737 / :739
            wk.y = __dadd_rn(wk.y, __dmul_rn(step, pk.y));
            hwk.x = __dadd_rn(hwk.x, __dmul_rn(step, hp.x));
            hwk.y = __dadd_rn(hwk.y, __dmul_rn(step, hp.y));
        }
        double2 vk = make_double2(0.0, 0.0);
        if (cont) {
            rk.x = __dadd_rn(rk.x, __dmul_rn(alpha, hp.x));          // :740
            rk.y = __dadd_rn(rk.y, __dmul_rn(alpha, hp.y));
            vk.x = (fr.x >= 0) ? 0.0 : rk.x;                         // projection!, box case (:741)
            vk.y = (fr.y >= 0) ? 0.0 : rk.y;
        }
        if (!e0) { wk.x = 0.0; hwk.x = 0.0; rk.x = 0.0; vk.x = 0.0; }
        if (!e1) { wk.y = 0.0; hwk.y = 0.0; rk.y = 0.0; vk.y = 0.0; }
        if (cont && !GEN) rv_part = fma(rk.y, vk.y, rk.x * vk.x);    // :743 (this chunk)
        if (add_w || a.j == 1) {
            reinterpret_cast<double2*>(a.w)[c] = wk;
            if (a.hw != nullptr) reinterpret_cast<double2*>(a.hw)[c] = hwk;
            if (SCAT && mp.x >= 0) a.w_full[mp.x] = wk.x;            // (slots at or beyond the live width map to -1)
            if (SCAT && mp.y >= 0) a.w_full[mp.y] = wk.y;
        }
        if (cont || a.j == 1) {
            reinterpret_cast<double2*>(a.r)[c] = rk;
            if (!GEN) reinterpret_cast<double2*>(a.v)[c] = vk;
        }
        if (GEN) rsm[cl] = vk;                                       // mask(r_new): what A_free multiplies
    } else if (GEN && rl == 0) {
        rsm[cl] = make_double2(0.0, 0.0);
    }
    if (!GEN) {
        if (rl == 0) rvs[cl] = rv_part;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) t += rvs[q];
            a.rvpart_out[blockIdx.x] = t;
        }
    } else {
        // left_mul, reduced form (src/polyhedral_constraints.jl:86-98 with the fixed components masked out): this workgroup's
        // share of A_free r for every row of A — thread (rl, cl) takes rows rl, rl+16, ... and chunk cl; the 16 chunk-lanes of a
        // row are one DPP row
        __syncthreads();
        if (cont) {
            const double2 rm = rsm[cl];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = rl + 16 * k;
                if (i < a.mA) {                                   // (uniform per 16-lane row)
                    double prod = valid ? fma(arow[k].y, rm.y, arow[k].x * rm.x) : 0.0;
                    prod = row16_sum(prod);
                    if (cl == 0) a.tpart[(int64_t)blockIdx.x * a.mA + i] = prod;
                }
            }
        }
    }

    // ---- workgroup 0 commits the iteration ----------------------------------------------------------------------------------
    if (blockIdx.x == 0 && tid == 0) {
        st->pHp = pHp; st->gamma = gamma; st->alpha = alpha; st->n_hmul = a.j; st->rtv = rtv;
        st->neg_curvature = neg; st->outside_region = outside; st->need_proj = 0; st->iter = a.j;
        tr.note_step_a(pHp, a.atol_neg, alpha, gamma, a.j);
        tr.store(st);
        if (a.trace != nullptr && a.j <= a.trace_cap) {
            double* row = a.trace + 4 * (int64_t)(a.j - 1);
            row[0] = pHp; row[1] = alpha; row[2] = (neg && !add_w) ? QNAN : gamma; row[3] = rtv;   // [3]: r.v after :746 follows in the next launch
        }
        int status = 4;                          // (a progress word: the host reads the status of a finished loop only)
        if (!cont) {
            status = cg_status_of(0, outside, neg, a.j, max_iter);
            st->approx_solved = 0; st->done = 1; st->stop_at = a.j;
            st->status = status;
        }
        publish_word(a.mirror, a.tag, status, cont ? 0 : 1, a.j, a.j, tr);      // progress (n_hmul = j) or the final state
    }
