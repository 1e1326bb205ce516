// kernels_batch.inc -- batches: one workgroup per LP (k_batch_solve, k_batch_block).
// Part of simplex_kernels.hip (ONE translation unit: included there, in this order, inside namespace mi355x).

// ------------------------------------------------------------------ batch: one workgroup per LP
// BASELINE config 4 is many SMALL independent LPs (257 x 769 doubles = 1.6 MB each).  Advancing
// them in lockstep with the launch pairs above makes every LP wait for the slowest one (78..199
// pivots per LP in the benchmark batch) and pays 2-3 launch boundaries per pivot.  Here ONE
// 1024-thread workgroup owns one LP and runs its whole n-solve-tableau loop
// (src/simplex.lisp:453-461) inside a single launch: the snapshot of the entering column and
// the normalised pivot row live in LDS, the phases are separated by workgroup barriers only,
// LPs progress independently and the hardware schedules waiting LPs onto free CUs.  Same
// arithmetic, same lexicographic reductions => same bits as the lockstep path and the oracle.
constexpr int kLpThreads = 1024;
constexpr int64_t kBatchLaunchCap = 4096;   // pivots per LP and launch of the per-LP kernels (a bounded launch: see mi355x_batch_cancel)
constexpr int kLpUnroll  = 4;   // measured at 128 / 1024 LPs of 257x513: 2 -> 1.76 / 1.49, 4 -> 1.76 / 2.13, 8 -> 1.22 / 1.33 M pivots/s

__global__ __launch_bounds__(kLpThreads) void k_batch_solve(TabView t, double sgn, double price_tol,
                                                           double ratio_thr)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double    s_v[kLpThreads / 64];
    __shared__ long long s_i[kLpThreads / 64];
    t = lp_slice(t);
    Ctl *ctl = t.ctl;
    const Ctl c0 = *ctl;                            // one load of the whole control block
    if (c0.status != kRunning) return;
    const int64_t rows = t.rows, m = rows - 1, vc = t.cols - 1, ld = t.ld, ldv = ld >> 1;
    double  *s_prow = lds;                          // ld doubles (16-byte aligned)
    double  *s_col  = lds + ld;                     // rows doubles
    vec2d   *M2 = reinterpret_cast<vec2d *>(t.M);
    const int64_t total = rows * ldv;               // tableau size in 16-byte pairs
    const int64_t dr = kLpThreads / ldv, dp = kLpThreads % ldv;   // flat-index stride as (row, pair)
    Ctl cl = c0;                                    // running copy (n_pivots / trace_n advance)
    int64_t n_pivots = c0.n_pivots;
    const int64_t max_pivots = c0.max_pivots;

    ValIdx e = block_price(t.M + m * ld, vc, sgn, s_v, s_i, t.p2l, t.col_bias);
    for (;;) {
        if (price_says_optimal(e, price_tol)) {
            if (threadIdx.x == 0) ctl->status = 0;  // MI_OPTIMAL
            break;
        }
        if (max_pivots > 0 && n_pivots >= max_pivots) {
            if (threadIdx.x == 0) ctl->status = 3;  // MI_MAX_PIVOTS
            break;
        }
        // a launch is bounded (the host can then honour a cancel between launches; the reference's
        // loop has no cap and no anti-cycling rule): still kRunning, the host launches again
        if (n_pivots - c0.n_pivots >= kBatchLaunchCap) break;
        const int64_t ec   = e.i;                   // LOGICAL column
        const int64_t slot = e.s;                   // its physical column
        // gather the entering column into LDS + ratio test
        ValIdx best; best.v = 0.0; best.i = -1; best.s = 0;
        ValIdx first; first.v = 0.0; first.i = -1; first.s = 0;   // this thread's first eligible row
        int bad = 0, nanq = 0;
        for (int64_t r = threadIdx.x; r < rows; r += kLpThreads) {
            const double a = t.M[r * ld + slot];
            s_col[r] = a;
            bad |= !(fabs(a) <= 1.7976931348623157e308);
            if (r < m && ratio_thr < a) {
                ValIdx c; c.v = t.M[r * ld + vc] / a; c.i = r; c.s = 0;
                if (first.i < 0) first.i = r;
                if (c.v != c.v) nanq = 1;            // no candidate, unless its row is the first eligible one
                else best = vi_min(best, c);
            }
        }
        ValIdx q = block_reduce_min(best, s_v, s_i);           // barriers: s_col complete
        if (__syncthreads_or(nanq)) {                          // the first-eligible-row rule: see block_gather_ratio
            first = block_reduce_min(first, s_v, s_i);
            if (first.i >= 0) {
                const double q0 = t.M[first.i * ld + vc] / s_col[first.i];
                if (q0 != q0) { q.v = q0; q.i = first.i; }
            }
        }
        if (t.p2l && __syncthreads_or(bad)) {                  // see kNeedDense
            if (threadIdx.x == 0) ctl->status = kNeedDense;
            break;
        }
        if (q.i < 0) {
            if (threadIdx.x == 0) ctl->status = 1;  // MI_UNBOUNDED
            break;
        }
        const int64_t cr = q.i;
        const double row_scale = s_col[cr];
        // normalised pivot row into LDS
        for (int64_t p = threadIdx.x; p < ldv; p += kLpThreads) {
            const double2 v = reinterpret_cast<const double2 *>(t.M + cr * ld)[p];
            reinterpret_cast<double2 *>(s_prow)[p] = scale_pair(t, p, v, row_scale, t.p2l ? slot : -1);
        }
        if (t.p2l) {                                // compact: the slot takes over the leaving column
            __syncthreads();                        // row cr has been read
            for (int64_t r = threadIdx.x; r < rows; r += kLpThreads)
                t.M[r * ld + slot] = (r == cr) ? 1.0 : 0.0;
            if (threadIdx.x == 0) swap_columns(t, ec, cr, slot);
        }
        __syncthreads();
        // rank-1 update of the whole tableau, kLpUnroll independent 16-byte accesses in flight per thread
        // (one workgroup streams at bytes-in-flight / latency: 8 x 16 B x 1024 threads per ~2 us);
        // the threads that write the objective row price it for the next iteration
        best.v = 0.0; best.i = -1; best.s = 0;
        int64_t idx = threadIdx.x, r = threadIdx.x / ldv, p = threadIdx.x % ldv;
        while (idx < total) {
            vec2d   v[kLpUnroll];
            int64_t ri[kLpUnroll], pi[kLpUnroll], ii[kLpUnroll];
            int     n = 0;
#pragma unroll
            for (int u = 0; u < kLpUnroll; ++u) {
                if (idx < total) {
                    ri[u] = r; pi[u] = p; ii[u] = idx;
                    v[u] = M2[idx];
                    n = u + 1;
                    idx += kLpThreads; r += dr; p += dp;
                    if (p >= ldv) { p -= ldv; r += 1; }
                }
            }
#pragma unroll
            for (int u = 0; u < kLpUnroll; ++u) {
                if (u < n) {
                    const double s = s_col[ri[u]];
                    const double2 pp = reinterpret_cast<const double2 *>(s_prow)[pi[u]];
                    const double m0 = s * pp.x;
                    const double m1 = s * pp.y;
                    vec2d o;
                    o.x = v[u].x - m0;
                    o.y = v[u].y - m1;
                    if (ri[u] == cr) { o.x = pp.x; o.y = pp.y; }
                    M2[ii[u]] = o;
                    if (ri[u] == m) {
                        const int64_t c0 = 2 * pi[u];
                        if (c0 < vc)     { ValIdx c = price_cand(o.x * sgn, t.p2l ? t.p2l[c0] : c0, c0, t.p2l ? 0 : t.col_bias);     best = vi_min(best, c); }
                        if (c0 + 1 < vc) { ValIdx c = price_cand(o.y * sgn, t.p2l ? t.p2l[c0 + 1] : c0 + 1, c0 + 1, t.p2l ? 0 : t.col_bias); best = vi_min(best, c); }
                    }
                }
            }
        }
        if (threadIdx.x == 0) record_pivot(t, cl, ec, cr);
        cl.n_pivots += 1; cl.trace_n += 1;
        n_pivots += 1;
        e = block_reduce_min(best, s_v, s_i);       // barrier: the update is complete and visible
    }
}

// ---- the same with blocked pivoting (compact representation) --------------------------------
// One workgroup streams its LP at (bytes in flight) / (memory latency) ~ 30 GB/s, so a pivot of a
// 1 MB tableau costs ~70 us however the loop is written.  Blocked as in k_la_block / k_sweep (every
// chain link in its general form: la_link / la_link2, kernels_la_common.inc), but
// with everything inside the one workgroup: the look-ahead state of up to KB pending pivots
// (col_i, prow_i), the running objective row, RHS column and column map live in LDS, a look-ahead
// step is two memory round trips (one strided column, one row) and two workgroup reductions, and
// the tableau itself is read and written once per KB pivots.
// 512 threads: the look-ahead never has more than a few hundred elements to spread, and the sweep
// wants 256 VGPRs per thread (16 prow pairs + four rows in flight; at 1024 threads it spilled).
constexpr int kBbThreads = 512, kRowPhases = kBbThreads / 256;

// Reduction of the per-LP kernel: wave arg-min (wave_argmin: v_min_f64 butterfly, the tree when a
// NaN or a tie is involved), one LDS slot per wave, ONE barrier, then every thread folds the
// wave winners in wave order -- the order of block_reduce_min.  `buf` alternates between the
// pricing and the ratio reduction of a step, so the slots of one are never rewritten before every
// thread has passed the other's barrier.
struct BbMsg { ValIdx c; unsigned flag; unsigned pad; };
__device__ __forceinline__ ValIdx bb_reduce(ValIdx mine, unsigned myflag, BbMsg *buf, unsigned &flag)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Cand c; c.v = mine.v; c.i = (int)mine.i;
    int src;
    c = wave_argmin(c, src);
    const int64_t cs = lane_pick(mine.s, src);
    const unsigned wf = __any(myflag != 0u) ? 1u : 0u;
    if (lane == 0) { buf[wave].c.v = c.v; buf[wave].c.i = c.i; buf[wave].c.s = cs; buf[wave].flag = wf; }
    __syncthreads();
    ValIdx r = buf[0].c;
    flag = buf[0].flag;
#pragma unroll
    for (int w = 1; w < kBbThreads / 64; ++w) { r = vi_min(r, buf[w].c); flag |= buf[w].flag; }
    return r;
}

template <int KB, bool SPLIT>
__global__ __launch_bounds__(kBbThreads) void k_batch_block(TabView t, double sgn, double price_tol,
                                                           double ratio_thr)
{
    // SPLIT == false: the whole solve of the LP in this launch, look-ahead and sweeps alternating.
    // SPLIT == true: the look-ahead of ONE block only; col_i / prow_i / masks / pending list go to
    // the LP's global block state and the sweep is a separate launch over ALL LPs (k_sweep with
    // grid.z = LP), which uses every CU of the chip instead of one per LP.  (A template parameter:
    // the look-ahead-only form carries neither the code nor the registers of the in-kernel sweep.)
    constexpr bool split = SPLIT;
    static_assert(KB % 4 == 0 && KB <= 16, "chains in groups of four links; 16 + 16 mask bits per pair");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ BbMsg s_wp[kBbThreads / 64], s_wr[kBbThreads / 64];
    t = lp_slice(t);
    Ctl *ctl = t.ctl;
    const Ctl c0 = *ctl;
    if (c0.status != kRunning) {
        if (split && threadIdx.x == 0) t.blk->n_pending = 0;   // nothing for the sweep that follows
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t rows = t.rows, m = rows - 1, vc = t.cols - 1, ld = t.ld, ldv = ld >> 1;
    const int64_t rp = (rows + 1) & ~(int64_t)1;
    double    *s_prow = lds;                                   // KB x ld
    double    *s_col  = s_prow + (int64_t)KB * ld;             // KB x rp
    double    *s_z    = s_col + (int64_t)KB * rp;              // ld: objective row through all pending pivots
    double    *s_b    = s_z + ld;                              // rp: RHS column, through all but the last one
    long long *s_p2l  = reinterpret_cast<long long *>(s_b + rp);   // ld: logical column of a slot
    long long *s_bas  = s_p2l + ld;                            // rp: basis (the leaving column of a pivot)
    unsigned  *s_rm   = reinterpret_cast<unsigned *>(s_bas + rp);  // rp: row -> pending pivots whose row it is
    unsigned  *s_sm   = s_rm + rp;                             // ldv: pair -> pending pivots whose slot it holds
    vec2d *M2 = reinterpret_cast<vec2d *>(t.M);

    // Ownership, fixed for the whole solve: a thread owns the rows r = tid, tid + T, ... (their
    // s_b / s_col / s_rm entries) and the column pairs p = tid, tid + T, ... (their s_z / s_prow /
    // s_p2l / s_sm entries): what a thread writes of these only it reads before the next barrier.
    for (int64_t c = tid; c < ld; c += kBbThreads) {
        s_z[c] = t.M[m * ld + c];
        s_p2l[c] = c < vc ? t.p2l[c] : -1;
    }
    for (int64_t r = tid; r < rp; r += kBbThreads) {
        s_b[r] = r < rows ? t.M[r * ld + vc] : 0.0;
        s_bas[r] = r < m ? t.basis[r] : -1;
    }
    int64_t n_pivots = c0.n_pivots, trace_n = c0.trace_n;
    int term = -1;                                             // status that ends the solve
    __syncthreads();

    while (term < 0) {
        for (int64_t r = tid; r < rp; r += kBbThreads) s_rm[r] = 0u;
        for (int64_t p = tid; p < ldv; p += kBbThreads) s_sm[p] = 0u;
        int k = 0, b_done = 0;                                 // pending pivots; how many of them s_b has seen
        int64_t v_cr = -1, v_sl = -1;                          // lane i: pivot row / slot of pending pivot i
        for (int J = 0; J < KB && term < 0; ++J) {
#ifdef MI355X_LA_TIMING
            const bool tm = blockIdx.z == 0 && tid == 0;
            unsigned long long T0 = wall_clock64(), T1 = T0, T2 = T0, T3 = T0, T4 = T0, T5 = T0;
#endif
            // ---- find-entering-column on the running objective row (my pairs)
            ValIdx best; best.v = 0.0; best.i = -1; best.s = 0;
            for (int64_t p = tid; p < ldv; p += kBbThreads) {
                const double2 z = reinterpret_cast<const double2 *>(s_z)[p];
                if (2 * p < vc)     { ValIdx x = price_cand(z.x * sgn, s_p2l[2 * p], 2 * p);     best = vi_min(best, x); }
                if (2 * p + 1 < vc) { ValIdx x = price_cand(z.y * sgn, s_p2l[2 * p + 1], 2 * p + 1); best = vi_min(best, x); }
            }
            unsigned fl;
#ifdef MI355X_LA_TIMING
            T1 = wall_clock64();
#endif
            const ValIdx e = bb_reduce(best, 0u, s_wp, fl);     // barrier: prow_{J-1}, s_z, masks of step J-1 complete
#ifdef MI355X_LA_TIMING
            T2 = wall_clock64();
#endif
            if (price_says_optimal(e, price_tol)) { term = 0; break; }          // MI_OPTIMAL
            if (c0.max_pivots > 0 && n_pivots >= c0.max_pivots) { term = 3; break; }   // MI_MAX_PIVOTS
            const int64_t ec = e.i, slot = uniform64(e.s);
            // ---- entering column through the pending chain, ratio test.  Uniform operands of the
            // chain: lane i holds prow_i[slot]; bit i of slmask: pending pivot i gave up this slot
            const double v_pa = lane < J ? s_prow[(int64_t)lane * ld + slot] : 0.0;
            const unsigned slmask = (unsigned)__ballot((lane < J) & (v_sl == slot));
            const double pb = J > 0 ? s_prow[(int64_t)(J - 1) * ld + vc] : 0.0;   // RHS entry of prow_{J-1}
            ValIdx q; q.v = 0.0; q.i = -1; q.s = 0;
            unsigned bad = 0u;
            for (int64_t r = tid; r < rows; r += kBbThreads) {
                double a = t.M[r * ld + slot];
                const unsigned rmb = s_rm[r];
                double b = s_b[r];
                if (J > 0) {                                   // RHS entry brought up to date with pivot J-1
                    b = pend(b, false, (rmb >> (J - 1)) & 1u, s_col[(int64_t)(J - 1) * rp + r], pb);
                    s_b[r] = b;
                }
#pragma unroll
                for (int i0 = 0; i0 < KB; i0 += 4) {
                    if (i0 < J) {
                        double prod[4], pa[4];
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) {
                            const double ci = (i0 + kk < J) ? s_col[(int64_t)(i0 + kk) * rp + r] : 0.0;
                            pa[kk] = lane_value(v_pa, i0 + kk);
                            prod[kk] = ci * pa[kk];                    // rounded product
                        }
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk)                     // every link in the general form
                            a = la_link(a, (slmask >> (i0 + kk)) & 1u, (rmb >> (i0 + kk)) & 1u, prod[kk], pa[kk]);
                    }
                }
                s_col[(int64_t)J * rp + r] = a;
                if (split) t.bk_col[(int64_t)J * t.bk_stride + r] = a;   // for the sweep launch
                bad |= !(fabs(a) <= 1.7976931348623157e308);
                if (r < m && ratio_thr < a) {
                    ValIdx x; x.v = b / a; x.i = r; x.s = __double_as_longlong(a);
                    if (x.v != x.v) bad = 1;         // a NaN quotient: decided by the lockstep select (kNeedDense)
                    else q = vi_min(q, x);
                }
            }
            b_done = J;
#ifdef MI355X_LA_TIMING
            T3 = wall_clock64();
#endif
            q = bb_reduce(q, bad, s_wr, fl);                   // barrier: s_col[J] complete
#ifdef MI355X_LA_TIMING
            T4 = wall_clock64();
#endif
            if (fl) { term = kNeedDense; break; }
            if (q.i < 0) { term = 1; break; }                  // MI_UNBOUNDED
            const int64_t cr = uniform64(q.i);
            const double piv = __longlong_as_double(q.s);
            // ---- pivot row through the chain -> prow_J; objective row through pivot J
            const double cmj = s_col[(int64_t)J * rp + m];
            const double v_ccr = lane < J ? s_col[(int64_t)lane * rp + cr] : 0.0;
            const unsigned crmask = (unsigned)__ballot((lane < J) & (v_cr == cr));
            for (int64_t p = tid; p < ldv; p += kBbThreads) {
                const vec2d y0 = M2[cr * ldv + p];
                double2 y = make_double2(y0.x, y0.y);
                const unsigned smb = s_sm[p];
#pragma unroll
                for (int i0 = 0; i0 < KB; i0 += 4) {
                    if (i0 < J) {
                        double2 pii[4], prod[4];
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) {
                            pii[kk] = (i0 + kk < J) ? reinterpret_cast<const double2 *>(s_prow + (int64_t)(i0 + kk) * ld)[p]
                                                    : make_double2(0.0, 0.0);
                            const double ccr = lane_value(v_ccr, i0 + kk);
                            prod[kk].x = ccr * pii[kk].x;              // rounded products
                            prod[kk].y = ccr * pii[kk].y;
                        }
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk)
                            y = la_link2(y, (smb >> (i0 + kk)) & 1u, (smb >> (16 + i0 + kk)) & 1u,
                                         (crmask >> (i0 + kk)) & 1u, prod[kk], pii[kk]);
                    }
                }
                const double2 pr = scale_pair(t, p, y, piv, slot);
                reinterpret_cast<double2 *>(s_prow + (int64_t)J * ld)[p] = pr;
                if (split) reinterpret_cast<double2 *>(t.bk_prow + (int64_t)J * ld)[p] = pr;
                double2 z = reinterpret_cast<double2 *>(s_z)[p];
                z.x = pend(z.x, 2 * p     == slot, false, cmj, pr.x);
                z.y = pend(z.y, 2 * p + 1 == slot, false, cmj, pr.y);
                reinterpret_cast<double2 *>(s_z)[p] = z;
                if (p == (slot >> 1)) {                        // the slot changes hands: its owner keeps the books
                    const int64_t leaving = s_bas[cr];
                    s_p2l[slot] = leaving;
                    s_sm[p] = smb | (1u << (J + 16 * (int)(slot & 1)));
                    t.p2l[slot] = leaving;
                    t.l2p[leaving] = slot;
                    t.l2p[ec] = -1;
                    t.basis[cr] = ec;                          // src/simplex.lisp:358
                    s_bas[cr] = ec;                            // (next read: after the next barrier)
                }
            }
            for (int64_t r = tid; r < rows; r += kBbThreads)
                if (r == cr) s_rm[r] |= 1u << J;
            if (tid == 0) {
                if (split) { t.blk->cr[J] = cr; t.blk->slot[J] = slot; }
                if (t.trace_ec && trace_n < t.trace_cap) { t.trace_ec[trace_n] = ec; t.trace_cr[trace_n] = cr; }
            }
            if (lane == J) { v_cr = cr; v_sl = slot; }
            n_pivots += 1; trace_n += 1;
            k = J + 1;
#ifdef MI355X_LA_TIMING
            T5 = wall_clock64();
            if (tm) {
                double *d = t.col;                              // (unused by this kernel)
                d[0] += 1.0; d[1] += (double)(T1 - T0); d[2] += (double)(T2 - T1); d[3] += (double)(T3 - T2);
                d[4] += (double)(T4 - T3); d[5] += (double)(T5 - T4);
            }
#endif
        }
        __syncthreads();                                       // prow / col / masks of the block complete
        if (split) {                                           // hand the block over to the sweep launch
            for (int64_t r = tid; r < t.bk_stride; r += kBbThreads) t.bk_rmask[r] = r < rp ? s_rm[r] : 0u;
            for (int64_t p = tid; p < ldv; p += kBbThreads) t.bk_smask[p] = s_sm[p];
            if (tid == 0) {
                t.blk->n_pending = k;
                if (term >= 0) ctl->status = term;
                ctl->n_pivots = n_pivots;
                ctl->trace_n = trace_n;
            }
            return;
        }
        if (k > b_done) {                                      // RHS column through the last pending pivot
            const double pb = s_prow[(int64_t)(k - 1) * ld + vc];
            for (int64_t r = tid; r < rows; r += kBbThreads)
                s_b[r] = pend(s_b[r], false, (s_rm[r] >> (k - 1)) & 1u, s_col[(int64_t)(k - 1) * rp + r], pb);
        }
        // ---- the sweep: the k pending pivots applied to every stored element.  Full strips of
        // 256 column pairs: a thread owns one pair (its prow entries of the pending pivots in
        // registers) and every fourth row; the row's col values come out of LDS as broadcasts.
        // The pairs left over beyond the last full strip: flat, operands from LDS.
        if (k > 0) {
            constexpr int kSU = KB >= 16 ? 2 : 4;                  // rows in flight per thread (16 pending pivots: 64 VGPRs of prow pairs)
            const int pp = tid & 255, rq = tid >> 8;               // pair within the strip, row phase
            const int64_t full = ldv & ~(int64_t)255;
            for (int64_t s0 = 0; s0 < full; s0 += 256) {
                const int64_t p = s0 + pp;
                double2 pr[KB];
#pragma unroll
                for (int i = 0; i < KB; ++i)
                    pr[i] = reinterpret_cast<const double2 *>(s_prow + (int64_t)i * ld)[p];
                const unsigned sm = s_sm[p];
                vec2d x[kSU], nx[kSU];
#pragma unroll
                for (int u = 0; u < kSU; ++u)
                    if (rq + kRowPhases * u < rows) nx[u] = M2[(rq + kRowPhases * u) * ldv + p];
                for (int64_t r = rq; r < rows; r += kRowPhases * kSU) {
#pragma unroll
                    for (int u = 0; u < kSU; ++u) x[u] = nx[u];
#pragma unroll
                    for (int u = 0; u < kSU; ++u)                  // the next rows travel during the chain
                        if (r + kRowPhases * (kSU + u) < rows) nx[u] = M2[(r + kRowPhases * (kSU + u)) * ldv + p];
#pragma unroll
                    for (int u = 0; u < kSU; ++u) {
                        const int64_t rr = r + kRowPhases * u;
                        if (rr < rows) {
                            const unsigned rm = s_rm[rr];
                            vec2d v = x[u];
                            if ((rm | sm) == 0u) {             // the bare chain
#pragma unroll
                                for (int i = 0; i < KB; ++i) {
                                    if (i < k) {
                                        const double s = s_col[(int64_t)i * rp + rr];
                                        const double m0 = s * pr[i].x, m1 = s * pr[i].y;
                                        v.x = v.x - m0;
                                        v.y = v.y - m1;
                                    }
                                }
                            } else {
#pragma unroll
                                for (int i = 0; i < KB; ++i) {
                                    if (i < k) {
                                        const double s = s_col[(int64_t)i * rp + rr];
                                        const bool is_cr = (rm >> i) & 1u;
                                        v.x = pend(v.x, (sm >> i) & 1u, is_cr, s, pr[i].x);
                                        v.y = pend(v.y, (sm >> (i + 16)) & 1u, is_cr, s, pr[i].y);
                                    }
                                }
                            }
                            M2[rr * ldv + p] = v;
                        }
                    }
                }
            }
            const int64_t rem = ldv - full, total_rem = rows * rem;   // < 256 pairs per row
            for (int64_t idx = tid; idx < total_rem; idx += kBbThreads) {
                const int64_t r = idx / rem, p = full + (idx - r * rem);
                const unsigned rm = s_rm[r], sm = s_sm[p];
                vec2d v = M2[r * ldv + p];
                for (int i = 0; i < k; ++i) {
                    const double  s = s_col[(int64_t)i * rp + r];
                    const double2 pi = reinterpret_cast<const double2 *>(s_prow + (int64_t)i * ld)[p];
                    const bool is_cr = (rm >> i) & 1u;
                    v.x = pend(v.x, (sm >> i) & 1u, is_cr, s, pi.x);
                    v.y = pend(v.y, (sm >> (i + 16)) & 1u, is_cr, s, pi.y);
                }
                M2[r * ldv + p] = v;
            }
            __syncthreads();                                   // tableau consistent before the next block reads it
        }
        // a launch is bounded (see k_batch_solve): still kRunning, the host launches again
        if (term < 0 && n_pivots - c0.n_pivots >= kBatchLaunchCap) term = kRunning;
    }
    if (tid == 0) {
        ctl->status = term;
        ctl->n_pivots = n_pivots;
        ctl->trace_n = trace_n;
    }
}
