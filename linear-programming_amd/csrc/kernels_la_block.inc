// kernels_la_block.inc -- the look-ahead of a whole block as ONE persistent launch (k_la_block)
// and its hand-off protocol.  The chains, the record format, the workgroup record's front half and
// the bookkeeping it shares with k_shard_la_block: kernels_la_common.inc.
// Part of simplex_kernels.hip (ONE translation unit: included there, in this order, inside namespace mi355x).

// ---- the look-ahead of a whole block as ONE launch ------------------------------------------
// Two launches per look-ahead step are two kernel boundaries (2.5 us each) plus cold caches at
// every start.  For tableaux whose rows and column pairs fit a few workgroups (config 3: 16 x 256
// threads cover 4096 constraint rows and 4096 pairs of non-RHS columns) the steps of a block run inside
// one launch instead: thread g owns row g (entering-column / RHS side) AND column pair g (pivot-row /
// objective-row side); its col_i[r], prow_i[pair], RHS entry and objective-row pair stay in registers / LDS from
// step to step, and the two reductions of a step go through a message exchange between the
// workgroups.  All workgroups reduce the same records with the same comparisons, so they take
// every decision (entering column, pivot row, termination) identically without further
// communication.
//
// The hand-off protocol.  gfx950: a CU's vector L1 is never refreshed by another CU's stores, the
// eight XCDs' L2s are not coherent with each other, and a workgroup barrier does NOT wait for the
// other waves' outstanding stores.  Hence:
//   * a record is eight self-validating 8-byte granules {tag = epoch, 32 bits of payload}, each
//     written by ONE store and polled with L1-bypassing (sc1) loads until all tags match: no
//     fence, no release/acquire pair, no read-modify-write;
//   * what a step has just produced and the next half-step needs at once travels IN the records
//     (the pivot-row entry of the winning candidate, the RHS entry of the winning row);
//   * everything else another workgroup reads inside the launch (col_i, prow_i of the older
//     pending pivots, basis) is stored WRITE-THROUGH (sc1: relaxed agent-scope atomic stores) and
//     read with sc1 loads, and every wave drains its stores (s_waitcnt vmcnt(0)) half a step
//     after issuing them -- before the barrier of the NEXT exchange, which is the first one whose
//     records anybody takes as evidence that those stores have landed.  (Round 1 published behind
//     a plain __syncthreads(), i.e. possibly before the other waves' col / prow stores had left
//     the CU: a reader on another XCD could chain a stale value -- the one-in-thousands
//     pivot-trace mismatch recorded in round 1's DESIGN.md.)
//   * words that only LATER launches read but that several workgroups write in turn (column
//     maps, basis) go write-through as well (two L2s holding different dirty versions of one word
//     are written back in an unspecified order); the control block, the pending list and the
//     trace have ONE writer, the leader thread; a mask word is written by its owner only.
//   * one-XCD mode (a pure speed option): the launch is 8x as wide and only every eighth block
//     takes part, which is where the dispatcher puts one XCD's blocks.  Nothing RELIES on that:
//     the first exchange of a launch (write-through, valid anywhere) carries every workgroup's
//     HW_REG_XCC_ID, and only if they all agree do the later stores become plain stores that stay
//     in the one shared L2 (where the sc1 loads find them a fabric round trip sooner).
struct LaMsg { ValIdx c; unsigned flag, same; double u; };

template <class T> __device__ __forceinline__ void st_wt(T *p, T v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one untorn store; local == true: all readers share this XCD's L2, the line may stay there
template <class T> __device__ __forceinline__ void st_x(T *p, T v, bool local)
{
    if (local) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else       __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T> __device__ __forceinline__ T ld_l2(const T *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// this wave's outstanding loads and stores have completed -- inline asm: the compiler neither
// moves nor drops it
__device__ __forceinline__ void drain_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ unsigned xcc_id()
{
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & 0xfu;
}

// a 16-byte aligned pair of granules as ONE 16-byte access (every granule is validated on its own,
// and a naturally aligned 16-byte access never tears an aligned 8-byte half)
typedef unsigned v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned long long pair_lo(const v4u &v) { return ((unsigned long long)v.y << 32) | v.x; }
__device__ __forceinline__ unsigned long long pair_hi(const v4u &v) { return ((unsigned long long)v.w << 32) | v.z; }
// one or two whole records (64 bytes each) per lane: four 16-byte loads per record, all in flight,
// L1 bypassed (sc1: what ld_l2 compiles to), the wait inside the statement (the compiler does not
// count these loads).  Half the requests of eight 8-byte loads per record -- and a wave's poll is
// bound by its requests: the lanes are a record (a 64-byte line) apart.
__device__ __forceinline__ void load_record(unsigned long long (&g)[8], const ExchRec *r)
{
    v4u q0, q1, q2, q3;
    asm volatile("global_load_dwordx4 %0, %4, off sc1\n\t"
                 "global_load_dwordx4 %1, %4, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %2, %4, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %3, %4, off offset:48 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3) : "v"(r) : "memory");
    g[0] = pair_lo(q0); g[1] = pair_hi(q0); g[2] = pair_lo(q1); g[3] = pair_hi(q1);
    g[4] = pair_lo(q2); g[5] = pair_hi(q2); g[6] = pair_lo(q3); g[7] = pair_hi(q3);
}
__device__ __forceinline__ void load_records2(unsigned long long (&g)[8], unsigned long long (&h)[8],
                                              const ExchRec *r, const ExchRec *r2)
{
    v4u q0, q1, q2, q3, p0, p1, p2, p3;
    asm volatile("global_load_dwordx4 %0, %8, off sc1\n\t"
                 "global_load_dwordx4 %1, %8, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %2, %8, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %3, %8, off offset:48 sc1\n\t"
                 "global_load_dwordx4 %4, %9, off sc1\n\t"
                 "global_load_dwordx4 %5, %9, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %6, %9, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %7, %9, off offset:48 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3), "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p3)
                 : "v"(r), "v"(r2) : "memory");
    g[0] = pair_lo(q0); g[1] = pair_hi(q0); g[2] = pair_lo(q1); g[3] = pair_hi(q1);
    g[4] = pair_lo(q2); g[5] = pair_hi(q2); g[6] = pair_lo(q3); g[7] = pair_hi(q3);
    h[0] = pair_lo(p0); h[1] = pair_hi(p0); h[2] = pair_lo(p1); h[3] = pair_hi(p1);
    h[4] = pair_lo(p2); h[5] = pair_hi(p2); h[6] = pair_lo(p3); h[7] = pair_hi(p3);
}

// (round 5) the records TRANSPOSED: granule j of record R at G[j][R] (G = the same 8 KB buffer seen as
// 8 x kMaxLaRecords granules).  The collecting wave's lane l fetches records l and l + 64: with a record
// per 64-byte line that was a request per LANE and load -- 1 024 requests of one CU per pass over 68
// records, about half a microsecond in which a record that has just landed goes unseen; transposed,
// consecutive lanes read consecutive granules: 16 loads of 512 contiguous bytes per pass.  A granule is
// still ONE untorn 8-byte store validated by its own tag, so nothing else changes.
static_assert(kMaxLaRecords == 128, "the offsets below: 1024 bytes from granule j to granule j + 1");
__device__ __forceinline__ void load_granules(unsigned long long (&g)[8], const unsigned long long *b0)
{
    const unsigned long long *b1 = b0 + 4 * kMaxLaRecords;
    asm volatile("global_load_dwordx2 %0, %8, off sc1\n\t"
                 "global_load_dwordx2 %1, %8, off offset:1024 sc1\n\t"
                 "global_load_dwordx2 %2, %8, off offset:2048 sc1\n\t"
                 "global_load_dwordx2 %3, %8, off offset:3072 sc1\n\t"
                 "global_load_dwordx2 %4, %9, off sc1\n\t"
                 "global_load_dwordx2 %5, %9, off offset:1024 sc1\n\t"
                 "global_load_dwordx2 %6, %9, off offset:2048 sc1\n\t"
                 "global_load_dwordx2 %7, %9, off offset:3072 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3]), "=&v"(g[4]), "=&v"(g[5]), "=&v"(g[6]), "=&v"(g[7])
                 : "v"(b0), "v"(b1) : "memory");
}
// records l (g) and l + 64 (h): 512 bytes further along every granule row
__device__ __forceinline__ void load_granules2(unsigned long long (&g)[8], unsigned long long (&h)[8], const unsigned long long *b0)
{
    const unsigned long long *b1 = b0 + 4 * kMaxLaRecords;
    asm volatile("global_load_dwordx2 %0, %16, off sc1\n\t"
                 "global_load_dwordx2 %1, %16, off offset:1024 sc1\n\t"
                 "global_load_dwordx2 %2, %16, off offset:2048 sc1\n\t"
                 "global_load_dwordx2 %3, %16, off offset:3072 sc1\n\t"
                 "global_load_dwordx2 %4, %17, off sc1\n\t"
                 "global_load_dwordx2 %5, %17, off offset:1024 sc1\n\t"
                 "global_load_dwordx2 %6, %17, off offset:2048 sc1\n\t"
                 "global_load_dwordx2 %7, %17, off offset:3072 sc1\n\t"
                 "global_load_dwordx2 %8, %16, off offset:512 sc1\n\t"
                 "global_load_dwordx2 %9, %16, off offset:1536 sc1\n\t"
                 "global_load_dwordx2 %10, %16, off offset:2560 sc1\n\t"
                 "global_load_dwordx2 %11, %16, off offset:3584 sc1\n\t"
                 "global_load_dwordx2 %12, %17, off offset:512 sc1\n\t"
                 "global_load_dwordx2 %13, %17, off offset:1536 sc1\n\t"
                 "global_load_dwordx2 %14, %17, off offset:2560 sc1\n\t"
                 "global_load_dwordx2 %15, %17, off offset:3584 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3]), "=&v"(g[4]), "=&v"(g[5]), "=&v"(g[6]), "=&v"(g[7]),
                   "=&v"(h[0]), "=&v"(h[1]), "=&v"(h[2]), "=&v"(h[3]), "=&v"(h[4]), "=&v"(h[5]), "=&v"(h[6]), "=&v"(h[7])
                 : "v"(b0), "v"(b1) : "memory");
}

// Exchange of one reduction between the workgroups.  `mine` is this thread's candidate.  Every
// WAVE reduces its 64 candidates (tree of wave_reduce_min) and publishes its winner at once as
// record 4 w + wave -- together with one double it picks out of its lanes' registers
// (extra(winner, lane that holds it, u)) -- so nothing waits for a workgroup barrier on the
// way out; the first wave of every workgroup collects all records (lane l: record l and, beyond 64
// records, l + 64), reduces them (tree again) and hands the winner to the other waves through LDS, with
// the double of the winner's own record.  Nothing else rides in a record: what a step needs of the RHS
// column and of the objective row it has on the side that decides (k_la_block below).
// The record's format: pack_rec / decode_rec (kernels_la_common.inc); the second double of a PRICE record
// and granule 7 of a RATIO record are 0 here.
// false: a record did not arrive within max_spins polls.
// true: every wave collects the records itself (no LDS hop, no workgroup barrier left in the
// kernel; four times the poll traffic on the one L2).  With a record per 64-byte line that lost
// (rounds 2 - 4: 149 us per block of 16 at config 3 against 122 us with the first wave of a workgroup
// collecting and broadcasting through LDS); with the records transposed (round 5: a pass over them is
// 16 loads of 512 contiguous bytes) it wins: 166 us per block of 24 against 174 us, 84.6 - 85.0 k
// pivots/s against 81.9 k.
constexpr bool kLaEveryWavePolls = true;

// The collecting half: poll until every record carries `tag`, reduce, winner and its double into `out`.
// TWO: more than 64 records -- lane l also takes record l + 64 and folds the two before the tree; without
// it the second record's loads, tag tests, decode and fold do not exist.  want_same (uniform; the launch's
// first exchange): do all records carry the same double?  (the XCC ids)
template <bool PRICE, bool TWO>
__device__ __forceinline__ void la_collect(const ExchRec *recs, int nrec, unsigned tag, unsigned max_spins,
                                           bool want_same, LaMsg &out, unsigned long long *ts)
{
    const int lane = threadIdx.x & 63;
    const bool v0 = lane < nrec, v1 = TWO && lane + 64 < nrec;
    const unsigned long long *gl = reinterpret_cast<const unsigned long long *>(recs) + lane;   // granule 0 of record `lane`
    unsigned long long g0[8], g1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) g1[k] = 0ull;
    unsigned spins = 0;
    bool fine = true;
    for (;;) {
        // (records past nrec exist in the buffer -- kMaxLaRecords of them -- and are never validated)
        if (TWO) load_granules2(g0, g1, gl);
        else     load_granules(g0, gl);
        bool ok0 = true, ok1 = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            ok0 &= (unsigned)(g0[k] >> 32) == tag;
            if (TWO) ok1 &= (unsigned)(g1[k] >> 32) == tag;
        }
        if (__all((ok0 | !v0) & (ok1 | !v1))) break;
        if (++spins > max_spins) { fine = false; break; }
    }
#ifdef MI355X_LA_TIMING
    if (ts) { ts[1] = wall_clock64(); ts[3] = spins; }
#endif
    Cand xl;
    int64_t sl;
    unsigned fl_l;
    double ul, u1 = 0.0, unused;
    decode_rec<PRICE>(g0, v0, xl, sl, fl_l, ul, unused);
    const double u0 = ul;
    if (TWO) {
        // lane-local fold of the two records (= the 64-apart level of a 128-wide tree)
        Cand x1;
        int64_t s1;
        unsigned f1;
        decode_rec<PRICE>(g1, v1, x1, s1, f1, u1, unused);
        const Cand x01 = cand_min(xl, x1);
        const bool hi = x01.i != xl.i;                            // record l + 64 won (indices are unique)
        xl = x01; sl = hi ? s1 : sl; ul = hi ? u1 : ul; fl_l |= f1;
    }
    int src;
    const Cand x = wave_argmin(xl, src);                          // uniform
    const unsigned fl = __any(fl_l != 0u) ? 1u : 0u;
    out.c.v = x.v; out.c.i = x.i;
    out.c.s = lane_pick(sl, src);
    out.u = lane_pick(ul, src);                                   // the winner's own record
    out.flag = fine ? fl : 2u;
    out.same = 0u;
    if (want_same) {
        const unsigned long long ref = dbits(lane_value(u0, 0));
        out.same = __all(((dbits(u0) == ref) || !v0) && ((dbits(u1) == ref) || !v1)) ? 1u : 0u;
    }
}

// WGR (more than kLaWaveRecordsMaxNw workgroups): ONE record per workgroup -- the four waves' winners meet in
// LDS and the first wave reduces them (wg_record), publishes record w, collects the nw (<= 64) records and
// hands the result on through s_res.  The double that rides along is the winning wave's.
template <bool PRICE, bool WGR = false, class Extra>
__device__ __forceinline__ bool la_exchange(ValIdx mine, unsigned myflag, ExchRec *recs, int nw, int w,
                                            unsigned tag, unsigned max_spins, bool mute, bool local,
                                            bool want_same, LaMsg *s_res, LaMsg &out, Extra extra,
                                            unsigned long long *ts, double *dbg = nullptr,
                                            bool give_up = false, LaWaveRec *s_wv = nullptr)
{
    constexpr bool kEvery = kLaEveryWavePolls && !WGR;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nrec = WGR ? nw : nw * kLaWaves;
    {   // ---- this wave's winner -> its record
        Cand c; c.v = mine.v; c.i = (int)mine.i;
        int src;
        c = wave_argmin(c, src);
        int64_t cs = lane_pick(mine.s, src);
        unsigned wf = __any(myflag != 0u) ? 1u : 0u;
        double u = 0.0, x2 = 0.0;
        ValIdx win; win.v = c.v; win.i = c.i; win.s = cs;
        extra(win, src, u);
        bool pub = !mute;
        if (WGR) {
            wg_record<PRICE, true>(s_wv, c, wf, cs, u, x2, false, 0);   // (one barrier)
            pub = pub && wave == 0;
        }
        if (pub) {
            const unsigned val = pack_rec<PRICE>(c, wf, cs, u, x2, lane);
            // granule `lane` of record w * 4 + wave: G[lane][record] (transposed layout, see load_granules)
            if (lane < 8) st_x(reinterpret_cast<unsigned long long *>(recs) + lane * kMaxLaRecords + (WGR ? w : w * kLaWaves + wave),
                               ((unsigned long long)tag << 32) | val, local);
        }
#ifdef MI355X_LA_TIMING
        if (dbg && lane == 0) dbg[w * kLaWaves + wave] = (double)wall_clock64();   // when this wave published
#endif
    }
#ifdef MI355X_LA_TIMING
    if (ts) ts[0] = wall_clock64();
#endif
    if (give_up) { out.flag = 2u; return false; }               // test hook (workgroup-uniform): published, then "timed out"
    auto collect = [&](LaMsg &o) {
        if (!WGR && nrec > 64) la_collect<PRICE, true>(recs, nrec, tag, max_spins, want_same, o, ts);    // (uniform)
        else                   la_collect<PRICE, false>(recs, nrec, tag, max_spins, want_same, o, ts);
    };
    if (kEvery) collect(out);                                   // every wave has the result in registers
    else {
        if (tid < 64) {
            LaMsg res;
            collect(res);
            if (lane == 0) *s_res = res;
        }
        __syncthreads();
        out = *s_res;
    }
#ifdef MI355X_LA_TIMING
    if (ts) ts[2] = wall_clock64();
#endif
    return out.flag != 2u;
}

// The steps are a run-time loop (fully unrolled the kernel was 300 KB of straight-line code and
// ran at the speed of instruction-cache misses): per-thread col_i[row] / prow_i[pair] of the
// pending pivots live in LDS ([pivot][thread]: conflict-free), everything else in registers.
// The chains through the pending pivots: la_chain_col / la_chain_row (kernels_la_common.inc).
// one_xcd: see above.  fault > 0 (test hook): the last workgroup stops publishing from step
// `fault - 1` on, as a workgroup that is not resident would.
// WGR: the form for more than kLaWaveRecordsMaxNw workgroups (records per workgroup, one polling wave; never one XCD).
template <int KMAX, bool WGR = false>
__global__ __launch_bounds__(kLaThreads) void k_la_block(TabView t, int ksteps, double sgn,
                                                        double price_tol, double ratio_thr,
                                                        unsigned epoch_base, unsigned max_spins,
                                                        int one_xcd, int fault)
{
    static_assert(KMAX % 4 == 0 && KMAX <= 24, "groups of four links; 32 + 32 bits of my_sm; 6 KB of LDS per pending pivot");
    __shared__ double    s_ci[KMAX][kLaThreads];                 // 32 KB (KMAX 16) / 48 KB (24)
    __shared__ double2   s_pi[KMAX][kLaThreads];                 // 64 KB / 96 KB
    __shared__ LaMsg     s_res;
    __shared__ LaWaveRec s_wv[kLaWaves];
    __shared__ int       s_left;                                 // fewest steps a wave of this workgroup completed (leave)
    int nw = gridDim.x, w = blockIdx.x;
    if (one_xcd) {                                               // only every eighth block takes part
        if (w & 7) return;
        w >>= 3; nw >>= 3;
    }
    Ctl *ctl = t.ctl;
    const Ctl c0 = *ctl;
    BlockCtl *blk = t.blk;
    const int tid = threadIdx.x;
    const bool leader = w == 0 && tid == 0;
    const int lane = tid & 63;
    const int64_t m = t.rows - 1, vc = t.cols - 1, ld = t.ld, ldv = ld >> 1;
    const int64_t g = (int64_t)w * kLaThreads + tid;
    // Rows below the objective row and pairs that hold a non-RHS column have an owner (the launch is
    // la_launch_workgroups() wide).  The objective row and the RHS column need none: their entries of a step are
    // already in the other side's registers, bit for bit --
    //   col_J[m] is z[slot] (the objective row goes through the same reset-or-subtract, on the same operands,
    //   in the same order, whether it is chained as a row entry of the entering column or kept up to date as
    //   z), and z[slot] is the pricing winner's key;
    //   prow_J[vc] is b[cr] / pivot (the same for the RHS column and b), and b[cr] rides in the ratio record.
    // With vc odd the last owned pair holds the RHS next to a real column; its owner chains and stores that
    // entry as any other (the same bits once more).
    const int64_t npair = (vc + 1) >> 1;
    const bool has_row = g < m, has_pair = g < npair;
    const int64_t r = g, p = g;
    const double2 *M2 = reinterpret_cast<const double2 *>(t.M);
    // who stores what has no owner, for the sweeps (not the leader's wave: it commits the pivot): col_J[m]; prow_J
    // from column 2 npair on -- the RHS entry if vc is even, then ld padding (+0.0: scale_pair)
    const bool stores_cm = w == 0 && tid == 64, stores_tail = w == 0 && (tid >> 6) == 2;

    unsigned my_rm = 0u;                 // bit i: my row is pivot row i
    unsigned long long my_sm = 0ull;     // bits i, 32 + i: my pair's even / odd column is the slot pivot i gave up
    la_block_begin(t, c0, leader, g, epoch_base);
    {   // the mask words past the last owner (objective row, row padding; RHS pair, ld padding): zero as everybody's
        const int64_t n_own = (int64_t)nw * kLaThreads, n_mask = t.bk_stride > ldv ? t.bk_stride : ldv;
        for (int64_t g2 = g + n_own; g2 < n_mask; g2 += n_own) la_zero_masks(t, g2);
    }
    // every way out of the launch records how many steps this workgroup COMPLETED (its col_i /
    // prow_i entries stored): the sweep applies no pivot that some workgroup did not finish
    // Where every WAVE polls for itself (up to kLaWaveRecordsMaxNw workgroups) a wave can time out on its own:
    // it has then completed fewer steps than the workgroup's other waves, which may still have seen the
    // late record arrive (round-5 advisor finding: the workgroup's one `done` entry, written by thread 0,
    // would claim a step whose prow / col entries that wave never stored).  Every wave leaves through here
    // exactly once, so they can meet: the entry is the MINIMUM over the waves.
    auto leave = [&](int steps) {
        if (lane == 0) atomicMin(&s_left, steps);
        __syncthreads();
        if (tid == 0) st_wt(&blk->done[w], (int64_t)(((unsigned long long)epoch_base << 8) | (unsigned)s_left));
    };
    if (c0.status != kRunning) return;       // (nothing pending; behind a lost exchange `done` belongs to that launch)
    if (tid == 0) s_left = 0x7fffffff;
    la_zero_pending(s_ci, s_pi);
    __syncthreads();                                             // (s_left: the launch's only barrier outside leave / the WGR exchanges)

    double  b = has_row ? t.M[r * ld + vc] : 0.0;                // RHS entry of my row
    double2 z = has_pair ? M2[m * ldv + p] : make_double2(0.0, 0.0);   // objective row, my pair
    int64_t l0 = has_pair ? t.p2l[2 * p] : -1;                   // logical columns of my pair
    int64_t l1 = (has_pair && 2 * p + 1 < vc) ? t.p2l[2 * p + 1] : -1;
    int64_t v_cr = -1, v_sl = -1;                                // lane i: pivot row / slot of pivot i
    unsigned wave_rm = 0u, wave_sm = 0u;                         // bit i: SOME lane of my wave is on pivot row i / holds slot i
    double2 pr = make_double2(0.0, 0.0);                         // my pair of the last normalised pivot row
    bool local = false;                                          // all workgroups on one XCD (verified)
    const double my_xcc = (double)xcc_id();
    unsigned long long *ts_p = nullptr, *ts_r = nullptr;
#ifdef MI355X_LA_TIMING
    unsigned long long tsp[4] = {0, 0, 0, 0}, tsr[4] = {0, 0, 0, 0};
    if (leader) { ts_p = tsp; ts_r = tsr; }
#endif

#ifndef MI355X_TEST_HOOKS
    fault = 0;                                                   // fault injection exists in the test build only
#endif
#pragma unroll 1
    for (int J = 0; J < ksteps; ++J) {
        const unsigned e_price = epoch_base + 2 * J + 1, e_ratio = epoch_base + 2 * J + 2;
        const bool mute = fault > 0 && J >= fault - 1 && w == nw - 1;
        // fault < 0 (test hook): the last workgroup publishes its ratio record of step -fault - 1 and
        // then gives up as if its polls had run out -- while every other workgroup sees all records,
        // the leader commits that pivot, and nobody gets past the next exchange
        // fault <= -1000 (test hook, the every-wave-polls form only): ONE wave of the last workgroup -- the second --
        // does that at step -fault - 1001 while the workgroup's other waves see all records and go on
        const bool quit = (fault < 0 && fault > -1000 && J == -fault - 1 && w == nw - 1 && nw > 1) ||
                          (!WGR && fault <= -1000 && J == -fault - 1001 && w == nw - 1 && (tid >> 6) == 1);
        double *dbg_p = nullptr, *dbg_r = nullptr;
#ifdef MI355X_LA_TIMING
        unsigned long long T0 = wall_clock64(), T2, T3, T5, T6;
        dbg_p = t.rhs + 512 + (2 * J) * 72;                      // publish times of the last block, per record
        dbg_r = t.rhs + 512 + (2 * J + 1) * 72;
#endif
        // ---- pricing: my pair's candidates -> wave winner -> record -> everybody's winner.
        // The record also carries the winner's entry of prow_{J-1}: what the chain below needs of the
        // row that was stored last.
        ValIdx best; best.v = 0.0; best.i = -1; best.s = 0;
        if (has_pair)                   { ValIdx c = price_cand(z.x * sgn, l0, 2 * p);     best = vi_min(best, c); }
        if (has_pair && 2 * p + 1 < vc) { ValIdx c = price_cand(z.y * sgn, l1, 2 * p + 1); best = vi_min(best, c); }
        LaMsg e;
        if (!la_exchange<true, WGR>(best, 0u, t.la_px, nw, w, e_price, max_spins, mute, local, J == 0, &s_res, e,
                [&](const ValIdx &c, int src, double &u) {
                    if (J == 0) { u = my_xcc; return; }
                    u = lane_pick((c.s & 1) ? pr.y : pr.x, src);            // prow_{J-1}[winner's slot]
                }, ts_p, dbg_p, false, s_wv)) {
            if (lane == 0) st_wt(&ctl->status, kSyncLost);       // same word, same value from every wave that gives up
            leave(J);
            return;
        }
        if (J == 0) local = one_xcd != 0 && e.same != 0u;        // same records, same decision everywhere
#ifdef MI355X_LA_TIMING
        T2 = wall_clock64();
#endif
        if (price_says_optimal(e.c, price_tol)) {
            if (leader) ctl->status = 0;                         // MI_OPTIMAL
            leave(J);
            return;
        }
        if (c0.max_pivots > 0 && c0.n_pivots + J >= c0.max_pivots) {
            if (leader) ctl->status = 3;                         // MI_MAX_PIVOTS
            leave(J);
            return;
        }
        const int64_t ec = e.c.i, slot = uniform64(e.c.s);
        // col_J[m] = z[slot]: the winner's key with the sign taken back (sgn is +-1: exact)
        const double cmj = e.c.v * sgn;
        const bool bad_m = !(fabs(cmj) <= 1.7976931348623157e308);   // (uniform) as for every entry of the column below
        // ---- entering column through the pending chain
        double a = has_row ? t.M[r * ld + slot] : 0.0;
        double v_pa = (lane < J - 1) ? ld_l2(&t.bk_prow[(int64_t)lane * ld + slot]) : 0.0;
        double ci_all[KMAX];           // my row's entries of the pending columns: they travel with the loads above
        la_prefetch(ci_all, s_ci, J);
        drain_vmem();                  // the loads -- and what this wave stored in the previous half-step
        if (lane == J - 1) v_pa = e.u;
        // pending pivots whose given-up slot is the entering column's slot (uniform)
        a = la_chain_col<KMAX>(a, ci_all, v_pa, J, my_rm, (unsigned)__ballot((lane < J) & (v_sl == slot)), wave_rm);
        s_ci[J][tid] = a;
        ValIdx q; q.v = 0.0; q.i = -1; q.s = 0;
        unsigned bad = 0u;
        if (has_row) {
            st_x(&t.bk_col[(int64_t)J * t.bk_stride + r], a, local);
            bad = !(fabs(a) <= 1.7976931348623157e308);
            if (ratio_thr < a) {
                const double qv = b / a;
                if (qv != qv) bad = 1u;                        // a NaN quotient: decided on the dense path (kNeedDense)
                else { q.v = qv; q.i = r; q.s = __double_as_longlong(a); }
            }
        }
#ifdef MI355X_LA_TIMING
        T3 = wall_clock64();
#endif
        if (stores_cm) st_x(&t.bk_col[(int64_t)J * t.bk_stride + m], cmj, local);
        // ---- ratio test; a record carries the RHS entry of its candidate's row
        LaMsg qq;
        if (!la_exchange<false, WGR>(q, bad, t.la_rx, nw, w, e_ratio, max_spins, mute, local, false, &s_res, qq,
                [&](const ValIdx &, int src, double &u) { u = lane_pick(b, src); },
                ts_r, dbg_r, quit, s_wv)) {
            if (lane == 0) st_wt(&ctl->status, kSyncLost);
            leave(J);
            return;
        }
#ifdef MI355X_LA_TIMING
        T5 = wall_clock64();
#endif
        if (qq.flag != 0u || bad_m) {                            // inf / NaN in the column: see kNeedDense
            if (leader) ctl->status = kNeedDense;
            leave(J);
            return;
        }
        if (qq.c.i < 0) {
            if (leader) ctl->status = 1;                         // MI_UNBOUNDED
            leave(J);
            return;
        }
        const int64_t cr = uniform64(qq.c.i);
        const double piv = __longlong_as_double(qq.c.s);
        // prow_J[vc] = b[cr] / pivot (scale_pair's division); my RHS entry through pivot J right away -- off
        // the pricing path, operands in registers
        const double prj_vc = qq.u / piv;
        b = pend(b, false, has_row && r == cr, a, prj_vc);
        // ---- pivot row through the chain -> prow_J; objective row through pivot J
        double2 y = has_pair ? M2[cr * ldv + p] : make_double2(0.0, 0.0);
        const double v_ccr = (lane < J) ? ld_l2(&t.bk_col[(int64_t)lane * t.bk_stride + cr]) : 0.0;
        const bool own = has_pair && (p == (slot >> 1));
        const int64_t leaving = own ? ld_l2(&t.basis[cr]) : -1;
        double2 pi_all[KMAX];          // my pair's entries of the pending rows: as ci_all above
        la_prefetch(pi_all, s_pi, J);
        drain_vmem();                  // the loads -- and the col_J entry stored above
        // pending pivots whose pivot row is the new pivot row (uniform)
        y = la_chain_row<KMAX>(y, pi_all, v_ccr, J, my_sm, (unsigned)__ballot((lane < J) & (v_cr == cr)), wave_sm);
        pr = make_double2(0.0, 0.0);
        if (has_pair) {
            pr = scale_pair(t, p, y, piv, slot);
            st_x(&t.bk_prow[(int64_t)J * ld + 2 * p], pr.x, local);
            st_x(&t.bk_prow[(int64_t)J * ld + 2 * p + 1], pr.y, local);
            z.x = pend(z.x, 2 * p     == slot, false, cmj, pr.x);
            z.y = pend(z.y, 2 * p + 1 == slot, false, cmj, pr.y);
        }
        s_pi[J][tid] = pr;
        if (stores_tail)
            for (int64_t c = 2 * npair + lane; c < ld; c += 64)
                st_x(&t.bk_prow[(int64_t)J * ld + c], c == vc ? prj_vc : 0.0, local);
        if (own) {                                               // the slot changes hands
            if (2 * p == slot) l0 = leaving; else l1 = leaving;
            st_x(&t.p2l[slot], leaving, local);
            st_x(&t.l2p[leaving], slot, local);
            st_x(&t.l2p[ec], (int64_t)-1, local);
            st_x(&t.basis[cr], ec, local);                       // src/simplex.lisp:358
            my_sm |= 1ull << (J + 32 * (int)(slot & 1));
            la_store_slot_mask(t, p, my_sm, J);
        }
        if (has_row && r == cr) {
            my_rm |= 1u << J;
            t.bk_rmask[r] = my_rm;
        }
        if (__any(has_row && r == cr)) wave_rm |= 1u << J;
        if (__any(own))                wave_sm |= 1u << J;
        if (leader) la_commit(t, c0, J, ec, cr, slot);           // the one writer of these words
        if (lane == J) { v_cr = cr; v_sl = slot; }
#if defined(MI355X_LA_TIMING) && MI355X_LA_TIMING != 2       // (2: publish stamps only, the leader is not slowed down)
        T6 = wall_clock64();
        if (leader) {
            double *d = t.rhs + J * 24;
            d[0] += 1.0; d[1] += (double)(T2 - T0); d[2] += (double)(T3 - T2);
            d[3] += (double)(T5 - T3); d[4] += (double)(T6 - T5);
            // inside the exchanges: entry -> own record published -> all records in -> result in every thread
            d[5] += (double)(tsp[0] - T0); d[6] += (double)(tsp[1] - tsp[0]); d[7] += (double)(tsp[2] - tsp[1]); d[8] += (double)tsp[3];
            d[9] += (double)(tsr[0] - T3); d[10] += (double)(tsr[1] - tsr[0]); d[11] += (double)(tsr[2] - tsr[1]); d[12] += (double)tsr[3];
        }
#endif
    }
    leave(ksteps);
}

// Pivots of the pending list that a sweep may apply: those EVERY workgroup of the persistent
// look-ahead launch `stamp` completed (BlockCtl::done).  All of n_pending in every run in which no
// exchange was lost; one fewer when a workgroup gave up on the ratio exchange of the last step while
// the leader's workgroup still saw all records and committed the pivot.
__device__ __forceinline__ int committed_pivots(const BlockCtl *__restrict__ blk, int k, unsigned stamp, int la_nw)
{
    for (int w = 0; w < la_nw; ++w) {
        const int64_t d = blk->done[w];
        const int dw = (unsigned)((unsigned long long)d >> 8) == stamp ? (int)(d & 0xff) : 0;
        k = dw < k ? dw : k;
    }
    return k;
}

// The same for a whole wave at once (the sweeps: every wave of every workgroup asks): lane l reads the
// records of workgroups l, l + 64, l + 128, l + 192 -- ONE round trip instead of la_nw dependent scalar loads
// (single tableaux have at most kMaxLaWorkgroups = 64 workgroups: one load; a column shard's k_shard_la_block
// up to kMaxShardLaWorkgroups = 256: the loads beyond the first are skipped by a uniform branch).  Uniform result.
__device__ __forceinline__ int done_steps(int64_t d, unsigned stamp)
{
    return (unsigned)((unsigned long long)d >> 8) == stamp ? (int)(d & 0xff) : 0;
}
__device__ __forceinline__ int committed_pivots_wave(const BlockCtl *__restrict__ blk, int k, unsigned stamp, int la_nw)
{
    const int lane = (int)(threadIdx.x & 63u);
    int dw = k;
    if (lane < la_nw) dw = done_steps(blk->done[lane], stamp);
    if (la_nw > 64) {                                            // (uniform)
        int64_t d1 = 0, d2 = 0, d3 = 0;
        const bool h1 = lane + 64 < la_nw, h2 = lane + 128 < la_nw, h3 = lane + 192 < la_nw;
        if (h1) d1 = blk->done[lane + 64];
        if (h2) d2 = blk->done[lane + 128];
        if (h3) d3 = blk->done[lane + 192];
        int o;
        if (h1) { o = done_steps(d1, stamp); dw = o < dw ? o : dw; }
        if (h2) { o = done_steps(d2, stamp); dw = o < dw ? o : dw; }
        if (h3) { o = done_steps(d3, stamp); dw = o < dw ? o : dw; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(dw, off, 64);
        dw = o < dw ? o : dw;
    }
    dw = __builtin_amdgcn_readfirstlane(dw);
    return dw < k ? dw : k;
}

// After a lost exchange: the sweep applied committed_pivots() of the n_pending pivots the leader
// recorded; take the bookkeeping of the others (at most one) back, newest first, so that the
// handle describes the tableau as it is -- the host then continues on the two-launch look-ahead.
// (The list and its stamp are those of the launch that lost the exchange: the launches enqueued
// behind it find the status kSyncLost and leave both alone.)
__global__ void k_la_rollback(TabView t, int la_nw)
{
    BlockCtl *blk = t.blk;
    Ctl *ctl = t.ctl;
    const int n = (int)blk->n_pending;
    const unsigned stamp = (unsigned)blk->stamp;
    if (n == 0 || stamp == 0u) return;
    const int keep = committed_pivots(blk, n, stamp, la_nw);
    for (int i = n - 1; i >= keep; --i) {
        const int64_t cr = blk->cr[i], slot = blk->slot[i], ec = blk->ec[i];
        // the maps are swapped by the thread that owns the slot's column pair -- which sits in the
        // workgroup that gave up when that workgroup holds the slot: then there is nothing to undo
        if (t.basis[cr] == ec) {
            const int64_t leaving = t.p2l[slot];
            t.p2l[slot] = ec;
            t.l2p[ec] = slot;
            t.l2p[leaving] = -1;
            t.basis[cr] = leaving;
        }
        ctl->n_pivots -= 1;
        ctl->trace_n -= 1;
    }
    blk->n_pending = keep;
}
