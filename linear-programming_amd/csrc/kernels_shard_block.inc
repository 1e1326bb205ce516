// kernels_shard_block.inc -- a column shard's look-ahead of a whole block as ONE persistent launch
// (k_shard_la_block) and the roll-back of its bookkeeping after a lost exchange.  What it has in common
// with k_la_block -- chains, record format, workgroup record, bookkeeping, thread / wave constants -- is
// kernels_la_common.inc's; its stores are write-through (st_wt) where k_la_block's are st_x(.., local).
// Part of simplex_kernels.hip (ONE translation unit: included there, in this order, inside namespace mi355x).

// ---- what a shard's step was, and what it is here ------------------------------------------------
// Exchange mode 2 (the shards push self-validating granules into each other's buffers) ran a shard's
// look-ahead step as TWO launches (k_shard_p2p_step + k_shard_la_scale<J>): two kernel boundaries, cold
// caches at both starts, the chain operands re-read from memory at every step -- 18.2 us per pivot on an
// 8-GPU-sized shard of config 5 (32769 x 8193 stored), a cost that does not shrink with the number of
// GPUs (DESIGN.md 5).  k_shard_la_block is k_la_block's idea at the shard's shape: the steps of a block
// run inside ONE launch of one workgroup per 256 rows of the (whole) column -- 129 at config 5 --, thread
// g owns row g (entering column / RHS copy) and, while g < ld / 2, column pair g of the shard's slice
// (pivot row / objective row); col_i[row] / prow_i[pair] of the pending pivots stay in LDS, the RHS entry
// and the objective-row pair in registers.  Per step (src/simplex.lisp:362-389 inside 453-461):
//
//   pricing      my pair's candidates -> wave winner -> workgroup record -> LOCAL exchange (the shard's
//                workgroups that hold pairs publish, everybody polls) -> the shard's winner
//   exchange A   workgroup 0 pushes the shard's (key, global column) pair into every shard's buffer; the
//                polling wave of every workgroup collects the `world` pairs -> the global winner and its
//                owner (same lexicographic rule everywhere -> same decision everywhere)
//   column       owner: its entry of the entering column through the pending chain, pushed to the peers
//                (exchange B) row by row; everybody else: polls its row's two granules in its own buffer
//   ratio test   redundant on every shard (RHS copy) -> LOCAL exchange over all workgroups -> pivot row
//   pivot row    the shard's slice of row cr through the chain -> prow_J; objective row through pivot J
//
// While exchange A is under way every workgroup already GATHERS the column of the shard's own winner
// (speculatively: one strided DRAM burst per step is the longest memory access of the step, and the
// owner -- for whose column everybody waits -- is exactly the shard whose speculation is right).
//
// The local exchanges are k_la_block<., WGR>'s: ONE record per workgroup, the four wave winners meeting
// in LDS, one polling wave, the result handed on through LDS -- with the form the skeleton measurements
// picked for > 64 workgroups (DESIGN_experiments.md R5.16): a record is ONE 64-byte line (eight
// self-validating granules {tag, 32 bits}), polled with four 16-byte L1-bypassing loads per record, lane
// l taking records l, l + 64, l + 128, l + 192.  No fence, no atomics, no read-modify-write anywhere.
//
// Commit protocol: BlockCtl::done[w] = (stamp << 8 | steps workgroup w completed), one entry per
// workgroup (up to kMaxShardLaWorkgroups); the sweep applies min(n_pending, min done) pivots.  A lost
// LOCAL exchange, a peer's pair or column that never arrives: status kSyncLost, the host rolls the
// bookkeeping of the uncommitted pivot back (k_shard_la_rollback) and puts the handle on the two-launch
// step (capi_colpart.inc).  The FIRST pricing exchange of a launch is published and polled by ALL
// workgroups (later ones only by those that hold pairs): it is the co-residency check, and it precedes
// the shard's first push -- a shard whose workgroups are not all resident never sends anything, so that
// every shard then ends the launch with nothing committed.
struct ShMsg { double v; int i; unsigned flag; int64_t s; double u, w; };   // flag: 1 non-finite, 2 a peer's column lost, 8 timed out

// records l, l + 64, ... of a 64-byte-per-record buffer: four 16-byte loads per record, all in flight, L1
// bypassed, the wait inside the statement (the compiler does not count these loads)
__device__ __forceinline__ void sh_split(unsigned long long (&g)[8], const v4u &a, const v4u &b, const v4u &c, const v4u &d)
{
    g[0] = pair_lo(a); g[1] = pair_hi(a); g[2] = pair_lo(b); g[3] = pair_hi(b);
    g[4] = pair_lo(c); g[5] = pair_hi(c); g[6] = pair_lo(d); g[7] = pair_hi(d);
}
__device__ __forceinline__ void sh_load1(unsigned long long (&g)[4][8], const ExchRec *r)
{
    load_record(g[0], r);
}
__device__ __forceinline__ void sh_load2(unsigned long long (&g)[4][8], const ExchRec *r)
{
    load_records2(g[0], g[1], r, r + 64);
}
__device__ __forceinline__ void sh_load3(unsigned long long (&g)[4][8], const ExchRec *r)
{
    const ExchRec *r1 = r + 64, *r2 = r + 128;
    v4u a0, a1, a2, a3, b0, b1, b2, b3, c0, c1, c2, c3;
    asm volatile("global_load_dwordx4 %0, %12, off sc1\n\t"
                 "global_load_dwordx4 %1, %12, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %2, %12, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %3, %12, off offset:48 sc1\n\t"
                 "global_load_dwordx4 %4, %13, off sc1\n\t"
                 "global_load_dwordx4 %5, %13, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %6, %13, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %7, %13, off offset:48 sc1\n\t"
                 "global_load_dwordx4 %8, %14, off sc1\n\t"
                 "global_load_dwordx4 %9, %14, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %10, %14, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %11, %14, off offset:48 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(b3),
                   "=&v"(c0), "=&v"(c1), "=&v"(c2), "=&v"(c3)
                 : "v"(r), "v"(r1), "v"(r2) : "memory");
    sh_split(g[0], a0, a1, a2, a3); sh_split(g[1], b0, b1, b2, b3); sh_split(g[2], c0, c1, c2, c3);
}
__device__ __forceinline__ void sh_load4(unsigned long long (&g)[4][8], const ExchRec *r)
{
    const ExchRec *r1 = r + 64, *r2 = r + 128, *r3 = r + 192;
    v4u a0, a1, a2, a3, b0, b1, b2, b3, c0, c1, c2, c3, d0, d1, d2, d3;
    asm volatile("global_load_dwordx4 %0, %16, off sc1\n\t"
                 "global_load_dwordx4 %1, %16, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %2, %16, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %3, %16, off offset:48 sc1\n\t"
                 "global_load_dwordx4 %4, %17, off sc1\n\t"
                 "global_load_dwordx4 %5, %17, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %6, %17, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %7, %17, off offset:48 sc1\n\t"
                 "global_load_dwordx4 %8, %18, off sc1\n\t"
                 "global_load_dwordx4 %9, %18, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %10, %18, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %11, %18, off offset:48 sc1\n\t"
                 "global_load_dwordx4 %12, %19, off sc1\n\t"
                 "global_load_dwordx4 %13, %19, off offset:16 sc1\n\t"
                 "global_load_dwordx4 %14, %19, off offset:32 sc1\n\t"
                 "global_load_dwordx4 %15, %19, off offset:48 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(b3),
                   "=&v"(c0), "=&v"(c1), "=&v"(c2), "=&v"(c3), "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3)
                 : "v"(r), "v"(r1), "v"(r2), "v"(r3) : "memory");
    sh_split(g[0], a0, a1, a2, a3); sh_split(g[1], b0, b1, b2, b3); sh_split(g[2], c0, c1, c2, c3); sh_split(g[3], d0, d1, d2, d3);
}

// The polling wave: records [0, nrec) until every one carries `tag` (or max_spins polls went by), then the
// winner (same rule, same result as any other tree: the minimum is unique), its slot / payload, the first
// double of its own record, and the "from" double (PRICE: second, RATIO: first) of record rec_from.
template <bool PRICE>
__device__ __forceinline__ void sh_poll(const ExchRec *recs, int nrec, unsigned tag, unsigned max_spins, int rec_from, ShMsg &out)
{
    const int lane = (int)(threadIdx.x & 63u);
    const int ng = (nrec + 63) >> 6;                             // (uniform) 1 .. 4
    unsigned long long g[4][8];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 8; ++k) g[a][k] = 0ull;
    unsigned spins = 0;
    bool fine = true;
    for (;;) {
        if (ng == 1)      sh_load1(g, recs + lane);
        else if (ng == 2) sh_load2(g, recs + lane);
        else if (ng == 3) sh_load3(g, recs + lane);
        else              sh_load4(g, recs + lane);
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            bool oka = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) oka &= (unsigned)(g[a][k] >> 32) == tag;
            ok &= oka | !(lane + 64 * a < nrec);
        }
        if (__all(ok)) break;
        if (++spins > max_spins) { fine = false; break; }
    }
    Cand best; best.v = 0.0; best.i = -1;
    int64_t bs = 0;
    double bu = 0.0, from = 0.0;
    unsigned fl = 0u;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        if (a < ng) {                                            // (uniform)
            Cand x; int64_t xs; unsigned f; double u, w;
            decode_rec<PRICE>(g[a], lane + 64 * a < nrec, x, xs, f, u, w);
            const Cand r = cand_min(best, x);
            const bool took = r.i != best.i;                      // (indices are unique; two empty candidates: either)
            bs = took ? xs : bs;
            bu = took ? u : bu;
            best = r;
            fl |= f;
            if ((rec_from >> 6) == a) from = PRICE ? w : u;
        }
    }
    int src;
    const Cand x = wave_argmin(best, src);                        // uniform
    out.v = x.v; out.i = x.i;
    out.s = lane_pick(bs, src);
    out.u = lane_pick(bu, src);
    out.w = lane_value_dyn(from, rec_from & 63);
    unsigned f = (__any((fl & 1u) != 0u) ? 1u : 0u) | (__any((fl & 2u) != 0u) ? 2u : 0u);
    out.flag = fine ? f : 8u;
}

// The same exchange read by ALL FOUR waves of a workgroup, a quarter of the records each (wave k: records
// k Q .. k Q + Q - 1, Q = ceil(nrec / 4) <= 64: one record per lane, ONE group of four loads), the four partial
// winners meeting in LDS: the decode of three record groups by one wave was 0.5 us of the ratio exchange's 3.4.
// A partial winner is a LaWaveRec whose x2 is the "from" double and whose f also carries 8: timed out.
template <bool PRICE>
__device__ __forceinline__ LaWaveRec sh_poll_quarter(const ExchRec *recs, int nrec, unsigned tag, unsigned max_spins, int rec_from, int wave)
{
    const int lane = (int)(threadIdx.x & 63u);
    const int Q = (nrec + kLaWaves - 1) / kLaWaves;
    const int first = wave * Q;
    const int count = nrec - first < Q ? (nrec - first < 0 ? 0 : nrec - first) : Q;
    const bool have = lane < count;
    unsigned long long g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = 0ull;
    bool fine = true;
    if (count > 0) {                                             // (uniform)
        unsigned spins = 0;
        for (;;) {
            load_record(g, recs + first + (have ? lane : 0));
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) ok &= (unsigned)(g[k] >> 32) == tag;
            if (__all(ok | !have)) break;
            if (++spins > max_spins) { fine = false; break; }
        }
    }
    Cand x; int64_t xs; unsigned f; double u, w;
    decode_rec<PRICE>(g, have && fine, x, xs, f, u, w);
    int src;
    const Cand b = wave_argmin(x, src);
    LaWaveRec p;
    p.v = b.v; p.i = b.i;
    p.s = lane_pick(xs, src);
    p.u = lane_pick(u, src);
    const int fl = rec_from - first;                              // the "from" record's lane in this quarter (if it is here)
    p.x2 = (fl >= 0 && fl < count) ? lane_value_dyn(PRICE ? w : u, fl) : 0.0;
    p.f = (__any((f & 1u) != 0u) ? 1u : 0u) | (__any((f & 2u) != 0u) ? 2u : 0u) | (fine ? 0u : 8u);
    return p;
}

// One local exchange as far as the polling wave: every wave's winner -> LDS -> the first wave reduces
// them, publishes the workgroup's record (if this workgroup publishes in this exchange) and polls the
// nrec records.  `out` is valid in the FIRST WAVE only: the caller hands it on (LDS + barrier).
// myflag: bit 0 non-finite, bit 1 a peer's column was lost.  give_up (test hook, workgroup-uniform):
// published, then "timed out".
// polls == false: this workgroup only publishes (its polling wave then takes the outcome from the leader's
// decision line: sh_decision_*).
template <bool PRICE, class Extra>
__device__ __forceinline__ void sh_exchange(ValIdx mine, unsigned myflag, ExchRec *recs, int nrec, bool publishes, int w,
                                            unsigned tag, unsigned max_spins, int rec_from, int wave_from,
                                            LaWaveRec *s_wv, Extra extra, bool give_up, ShMsg &out, bool polls = true)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Cand c; c.v = mine.v; c.i = (int)mine.i;
    int src;
    c = wave_argmin(c, src);
    int64_t cs = lane_pick(mine.s, src);
    unsigned wf = (__any((myflag & 1u) != 0u) ? 1u : 0u) | (__any((myflag & 2u) != 0u) ? 2u : 0u);
    double u = 0.0, x2 = 0.0;
    ValIdx win; win.v = c.v; win.i = c.i; win.s = cs;
    extra(win, src, u, x2);
    wg_record<PRICE>(s_wv, c, wf, cs, u, x2, w == rec_from, wave_from);   // (one barrier)
    if (wave != 0) return;
    if (publishes) {
        const unsigned val = pack_rec<PRICE>(c, wf, cs, u, x2, lane);   // lane k stores granule k of record w: ONE 64-byte line
        if (lane < 8) st_wt(&recs[w].g[lane], ((unsigned long long)tag << 32) | val);
    }
    out.v = 0.0; out.i = -1; out.s = 0; out.u = out.w = 0.0; out.flag = 0u;
    if (give_up) { out.flag = 8u; return; }
    if (polls) sh_poll<PRICE>(recs, nrec, tag, max_spins, rec_from, out);
}

// The ratio exchange is polled only by the workgroups that need its result AT ONCE -- those that hold
// column pairs and chain the pivot row next (17 of 129 on an 8-GPU shard of config 5): an all-to-all's price
// on this chip grows with its readers (MI355X_MICROARCH.md, allgather row).  Everybody else needs the pivot
// row's index only for its masks, a step later: workgroup 0 writes it (and the flags) into ONE line, which
// the others' polling waves wait for while the pair holders are busy with the row.
__device__ __forceinline__ void sh_decision_publish(ExchRec *line, unsigned tag, const ShMsg &d)
{
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned val = lane == 0 ? (d.i < 0 ? 0xffffffffu : (unsigned)d.i) : d.flag;
    if (lane < 2) st_wt(&line->g[lane], ((unsigned long long)tag << 32) | val);
}
__device__ __forceinline__ void sh_decision_poll(const ExchRec *line, unsigned tag, unsigned max_spins, ShMsg &d)
{
    const int lane = (int)(threadIdx.x & 63u);
    unsigned long long g = 0ull;
    bool fine = true;
    for (unsigned spins = 0;; ++spins) {
        if (lane < 2) g = ld_l2(&line->g[lane]);
        if (__all(lane >= 2 || (unsigned)(g >> 32) == tag)) break;
        if (spins > max_spins) { fine = false; break; }
    }
    const unsigned iw = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)g, 0);
    const unsigned fl = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)g, 1);
    d.v = 0.0; d.s = 0; d.u = d.w = 0.0;
    d.i = iw == 0xffffffffu ? -1 : (int)iw;
    d.flag = fine ? fl : 8u;
}

// system-scope granules of exchange mode 2 (what k_shard_p2p_step uses; defined with the per-pivot shard steps)
//   st_sys / ld_sys

// hop: exchange A runs (world > 1, or a lone shard measured as one of several: it then pushes to and polls
// its own buffer, which is what a shard of a real partition pays minus the wire).  fault: as k_la_block's,
// applied to the last workgroup of the LAST shard of the launch.
template <int KMAX>
__global__ __launch_bounds__(kLaThreads) void k_shard_la_block(const ShardLaunch *__restrict__ shards, P2pLayout lay,
                                                              int ksteps, double sgn, double price_tol, double ratio_thr,
                                                              unsigned epoch_base, unsigned xepoch_base, unsigned max_spins,
                                                              unsigned p2p_spins, int hop, int fault)
{
    static_assert(KMAX % 4 == 0 && KMAX <= 24, "groups of four links; 32 + 32 bits of my_sm; 6 KB of LDS per pending pivot");
    __shared__ double    s_ci[KMAX][kLaThreads];
    __shared__ double2   s_pi[KMAX][kLaThreads];
    __shared__ ShMsg     s_res, s_res2;
    __shared__ LaWaveRec s_wv[kLaWaves];
    __shared__ LaWaveRec s_part[kLaWaves];
    const ShardLaunch &S = shards[blockIdx.y];
    const TabView t = S.t;
    const int w = blockIdx.x;
    const int64_t m = t.rows - 1, vcl = t.cols - 1, ld = t.ld, ldv = ld >> 1;
    const int64_t need = t.rows > ldv ? t.rows : ldv;
    const int nw = (int)((need + kLaThreads - 1) / kLaThreads);  // this shard's workgroups (the grid is the widest shard's)
    const int nwp = (int)((ldv + kLaThreads - 1) / kLaThreads);  // ... of which these hold column pairs
    if (w >= nw) return;
    Ctl *ctl = t.ctl;
    const Ctl c0 = *ctl;
    BlockCtl *blk = t.blk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool leader = w == 0 && tid == 0;
    const bool compact = t.p2l != nullptr;
    const int64_t bias = compact ? 0 : S.col_offset;             // dense shard: global index of local column 0
    const int rank = S.rank, world = lay.world;
    const int64_t g = (int64_t)w * kLaThreads + tid;
    const bool has_row = g < t.rows, has_pair = g < ldv;
    const int64_t r = g, p = g;
    const double2 *M2 = reinterpret_cast<const double2 *>(t.M);
    // thread that owns the RHS pair / the objective row: workgroup (= record), wave, lane
    const int g_vc = (int)(vcl >> 1), g_m = (int)m;
    const int rec_vc = g_vc / kLaThreads, rec_m = g_m / kLaThreads;
    const int wave_vc = (g_vc / 64) % kLaWaves, wave_m = (g_m / 64) % kLaWaves;
    const bool wave_has_vc = (int)(g / 64) == g_vc / 64, wave_has_m = (int)(g / 64) == g_m / 64;

    unsigned my_rm = 0u;
    unsigned long long my_sm = 0ull;
    la_block_begin(t, c0, leader, g, epoch_base);
    auto leave = [&](int steps) {
        if (tid == 0) st_wt(&blk->done[w], (int64_t)(((unsigned long long)epoch_base << 8) | (unsigned)steps));
    };
    if (c0.status != kRunning) return;
    la_zero_pending(s_ci, s_pi);

    double  b = (has_row && r < m) ? t.M[r * ld + vcl] : 0.0;    // my row's entry of the shard's RHS copy
    double2 z = has_pair ? M2[m * ldv + p] : make_double2(0.0, 0.0);
    int64_t l0 = -1, l1 = -1;                                     // logical (compact: global) columns of my pair
    if (has_pair && 2 * p < vcl)     l0 = compact ? t.p2l[2 * p] : 2 * p;
    if (has_pair && 2 * p + 1 < vcl) l1 = compact ? t.p2l[2 * p + 1] : 2 * p + 1;
    int64_t v_cr = -1, v_sl = -1;                                // lane i: pivot row / slot of pivot i (-1: no slot changed hands here)
    unsigned wave_rm = 0u, wave_sm = 0u;
    double2 pr = make_double2(0.0, 0.0);
    unsigned long long *const xmine = S.mine;
    unsigned long long *const *const xpeers = S.peers;

#ifndef MI355X_TEST_HOOKS
    fault = 0;
#endif
    const bool faulty_wg = (int)blockIdx.y == (int)gridDim.y - 1 && w == nw - 1;
#pragma unroll 1
    for (int J = 0; J < ksteps; ++J) {
        const unsigned e_price = epoch_base + 2 * J + 1, e_ratio = epoch_base + 2 * J + 2;
        const unsigned xe = xepoch_base + (unsigned)J + 1u, par = xe & 1u;      // exchange A / B: this pivot's tag and parity
        const unsigned long long xtg = (unsigned long long)xe << 32;
        const bool mute = fault > 0 && J >= fault - 1 && faulty_wg;
        const bool quit = fault < 0 && J == -fault - 1 && faulty_wg && nw > 1;
#ifdef MI355X_LA_TIMING
        unsigned long long T0 = wall_clock64(), T1 = T0, T1b = T0, T2 = T0, T3 = T0, T4 = T0, T5 = T0;
#endif
        // ---- pricing: the shard's winner.  The record also carries the winner's entry of prow_{J-1} and
        // (from its owner) the RHS entry of prow_{J-1}: what the chains need of the row stored last.
        ValIdx best; best.v = 0.0; best.i = -1; best.s = 0;
        if (has_pair && 2 * p < vcl)     { ValIdx c = price_cand(z.x * sgn, l0, 2 * p, bias);     best = vi_min(best, c); }
        if (has_pair && 2 * p + 1 < vcl) { ValIdx c = price_cand(z.y * sgn, l1, 2 * p + 1, bias); best = vi_min(best, c); }
        const bool all_publish = J == 0;                         // the launch's first exchange: the co-residency check
        ShMsg e;
        sh_exchange<true>(best, 0u, t.la_px, all_publish ? nw : nwp, (all_publish || w < nwp) && !mute, w, e_price, max_spins,
                          rec_vc, wave_vc, s_wv,
                          [&](const ValIdx &c, int src, double &u, double &x2) {
                              if (J == 0) return;
                              u = lane_pick((c.s & 1) ? pr.y : pr.x, src);                       // prow_{J-1}[winner's slot]
                              if (wave_has_vc) x2 = lane_value_dyn((vcl & 1) ? pr.y : pr.x, g_vc & 63);
                          }, false, e);
        // (first wave) e = the shard's winner: key, logical column (dense: local), slot, payloads
#ifdef MI355X_LA_TIMING
        T1 = wall_clock64();
#endif
        double a = 0.0;                                          // my row's entry of the entering column
        double v_pa = 0.0;
        bool mine;                                               // this shard owns the entering column
        int64_t ec, lc;                                          // global logical column; its local physical column (owner)
        if (hop) {
            if (wave == 0) {
                if (w == 0 && e.flag == 0u && !mute) {
                    // exchange A, producer: my (key, global column) pair into slot `rank` of EVERY shard's buffer
                    const double pk = e.i < 0 ? 0.0 : e.v;
                    const double pc = e.i < 0 ? -1.0 : (e.s == kNanColumn0 ? -2.0 : (double)((int64_t)e.i + bias));
                    if (lane < world) {
                        const unsigned long long kb = dbits(pk), cb = dbits(pc);
                        unsigned long long *dst = xpeers[lane] + lay.pair_off(par, rank);
                        st_sys(dst + 0, xtg | (kb & 0xffffffffull));
                        st_sys(dst + 1, xtg | (kb >> 32));
                        st_sys(dst + 2, xtg | (cb & 0xffffffffull));
                        st_sys(dst + 3, xtg | (cb >> 32));
                    }
                }
                if (lane == 0) s_res = e;
            }
            __syncthreads();
            const ShMsg el = s_res;                              // the shard's own winner, in every thread
#ifdef MI355X_LA_TIMING
            T1b = wall_clock64();
#endif
            // speculation: gather the column of the shard's OWN winner while the pairs travel
            const bool spec = el.flag == 0u && el.i >= 0 && el.s != kNanColumn0;
            const int64_t sl_spec = spec ? uniform64(el.s) : 0;
            if (spec) {
                a = has_row ? t.M[r * ld + sl_spec] : 0.0;
                v_pa = (lane < J - 1) ? ld_l2(&t.bk_prow[(int64_t)lane * ld + sl_spec]) : 0.0;
            }
            ShMsg gw;                                            // the global winner: v, i = global column, s = owner's rank
            if (wave == 0) {
                gw.v = 0.0; gw.i = -1; gw.s = 0; gw.u = 0.0; gw.w = 0.0; gw.flag = el.flag;
                if (el.flag == 0u) {
                    // exchange A, consumer: every shard's pair of this pivot (lane q: shard q)
                    const unsigned long long *src = xmine + lay.pair_off(par, lane < world ? lane : 0);
                    unsigned long long q0 = 0, q1 = 0, q2 = 0, q3 = 0;
                    unsigned spins = 0;
                    bool fine = true;
                    for (;;) {
                        bool ok = true;
                        if (lane < world) {
                            q0 = ld_sys(src + 0); q1 = ld_sys(src + 1); q2 = ld_sys(src + 2); q3 = ld_sys(src + 3);
                            ok = (unsigned)(q0 >> 32) == xe && (unsigned)(q1 >> 32) == xe && (unsigned)(q2 >> 32) == xe &&
                                 (unsigned)(q3 >> 32) == xe;
                        }
                        if (__all(ok)) break;
                        if (++spins > p2p_spins) { fine = false; break; }
                    }
                    const double key = join_bits(q0, q1), col = join_bits(q2, q3);
                    Cand c; c.v = key; c.i = (lane < world && col >= 0.0) ? (int)col : -1;
                    const bool nan0 = __any(lane < world && col == -2.0);   // some shard holds a NaN in global column 0's objective entry
                    int owner;
                    const Cand x = wave_argmin(c, owner);
                    gw.v = x.v; gw.i = nan0 ? -1 : x.i; gw.s = owner < 0 ? 0 : owner;
                    gw.flag = fine ? 0u : 8u;
                }
                if (lane == 0) s_res2 = gw;
            }
            __syncthreads();
            gw = s_res2;
            e = el;
            if (gw.flag != 0u) {                                 // a local record or a peer's pair never arrived
                if (tid == 0) st_wt(&ctl->status, kSyncLost);
                leave(J);
                return;
            }
            ValIdx ge; ge.v = gw.v; ge.i = gw.i; ge.s = 0;
            if (price_says_optimal(ge, price_tol)) {
                if (leader) ctl->status = 0;                     // MI_OPTIMAL
                leave(J);
                return;
            }
            ec = gw.i;
            mine = (int)gw.s == rank;
            lc = mine ? sl_spec : -1;                            // (the global winner of MY shard is my own winner)
        } else {
#ifdef MI355X_LA_TIMING
            T1b = T1;                                            // (no exchange A: that column of the clocks stays empty)
#endif
            if (wave == 0 && lane == 0) s_res = e;
            __syncthreads();
            e = s_res;
            if (e.flag != 0u) {
                if (tid == 0) st_wt(&ctl->status, kSyncLost);
                leave(J);
                return;
            }
            ValIdx le; le.v = e.v; le.i = e.i; le.s = e.s;
            if (price_says_optimal(le, price_tol)) {
                if (leader) ctl->status = 0;
                leave(J);
                return;
            }
            ec = (int64_t)e.i + bias;
            mine = true;
            lc = uniform64(e.s);
            a = has_row ? t.M[r * ld + lc] : 0.0;
            v_pa = (lane < J - 1) ? ld_l2(&t.bk_prow[(int64_t)lane * ld + lc]) : 0.0;
        }
        if (c0.max_pivots > 0 && c0.n_pivots + J >= c0.max_pivots) {
            if (leader) ctl->status = 3;                         // MI_MAX_PIVOTS
            leave(J);
            return;
        }
        const int64_t slot = (mine && compact) ? lc : -1;        // the slot that changes hands (compact owner only)
#ifdef MI355X_LA_TIMING
        T2 = wall_clock64();
#endif
        // ---- entering column: the owner chains its entry through the pending pivots and pushes it; the
        // others wait for their row's granules.  My RHS entry through pivot J-1 meanwhile.
        double ci_all[KMAX];
        la_prefetch(ci_all, s_ci, J);
        unsigned lost = 0u;
        if (!mine) {
            // exchange B, consumer: my row's two granules of this pivot's column, in my own buffer
            a = 0.0;
            if (has_row) {
                const unsigned long long *src = xmine + lay.col_off(par) + 2 * r;
                unsigned long long lo, hi;
                for (unsigned spins = 0;; ++spins) {
                    lo = ld_sys(src);
                    hi = ld_sys(src + 1);
                    if ((unsigned)(lo >> 32) == xe && (unsigned)(hi >> 32) == xe) break;
                    if (spins > p2p_spins) { lost = 2u; lo = hi = 0ull; break; }
                }
                a = join_bits(lo, hi);
            }
        }
        drain_vmem();                  // the loads -- and what this wave stored in the previous half-step
        if (J > 0) b = pend(b, false, (my_rm >> (J - 1)) & 1u, s_ci[J - 1][tid], e.w);
        if (mine) {
            if (lane == J - 1) v_pa = e.u;
            a = la_chain_col<KMAX>(a, ci_all, v_pa, J, my_rm, (unsigned)__ballot((lane < J) & (v_sl == lc) & (slot >= 0)), wave_rm);
            if (has_row && world > 1) {
                // exchange B, producer: my row's entry straight into the OTHER shards' buffers
                const unsigned long long vb = dbits(a);
                const int64_t off = lay.col_off(par) + 2 * r;
                for (int q = 0; q < world; ++q)
                    if (q != rank) {
                        st_sys(xpeers[q] + off, xtg | (vb & 0xffffffffull));
                        st_sys(xpeers[q] + off + 1, xtg | (vb >> 32));
                    }
            }
        }
        s_ci[J][tid] = a;
        ValIdx q; q.v = 0.0; q.i = -1; q.s = 0;
        unsigned bad = lost;
        if (has_row) {
            st_wt(&t.bk_col[(int64_t)J * t.bk_stride + r], a);
            if (compact && !(fabs(a) <= 1.7976931348623157e308)) bad |= 1u;   // compact shard: MI_NONFINITE
            if (r < m && ratio_thr < a) {
                const double qv = b / a;
                if (qv != qv) bad |= 1u;                       // a NaN quotient: MI_NONFINITE (k_shard_la_ratio)
                else { q.v = qv; q.i = r; q.s = __double_as_longlong(a); }
            }
        }
#ifdef MI355X_LA_TIMING
        T3 = wall_clock64();
#endif
        // ---- ratio test (every shard, on its RHS copy); the record of the objective row's wave carries col_J[m]
        ShMsg qq;
        const bool ratio_reader = w < nwp;                       // (uniform) holds column pairs: needs the pivot row at once
        // (the readers' polling is shared by their four waves: sh_poll_quarter; everybody else -- and a reader told to
        // give up, test hook -- goes through the first wave)
        const bool shared_poll = ratio_reader && !quit;                // (uniform)
        sh_exchange<false>(q, bad, t.la_rx, nw, !mute, w, e_ratio, max_spins, rec_m, wave_m, s_wv,
                           [&](const ValIdx &, int, double &u, double &) { if (wave_has_m) u = lane_value_dyn(a, g_m & 63); },
                           quit, qq, false);
        ExchRec *line = t.la_rx + (kMaxShardLaWorkgroups - 1);    // (the last record: nw < kMaxShardLaWorkgroups)
        if (shared_poll) {
            const LaWaveRec mp = sh_poll_quarter<false>(t.la_rx, nw, e_ratio, max_spins, rec_m, wave);
            if (lane == 0) s_part[wave] = mp;
            __syncthreads();
            Cand c;
            unsigned fl;
            const int ww = fold_waves(s_part, c, fl);
            const int Qr = (nw + kLaWaves - 1) / kLaWaves;
            qq.v = c.v; qq.i = c.i; qq.s = s_part[ww].s; qq.u = s_part[ww].u; qq.w = s_part[rec_m / Qr].x2; qq.flag = fl;
            if (w == 0 && wave == 0 && !mute) sh_decision_publish(line, e_ratio, qq);
        } else {
            if (wave == 0) {
                if (!ratio_reader && qq.flag == 0u) sh_decision_poll(line, e_ratio, max_spins, qq);
                if (lane == 0) s_res = qq;
            }
            __syncthreads();
            qq = s_res;
        }
        if (qq.flag & (8u | 2u)) {                               // a record -- or somebody's rows of the column -- never arrived
            if (tid == 0) st_wt(&ctl->status, kSyncLost);
            leave(J);
            return;
        }
        if (qq.flag & 1u) {
            if (leader) ctl->status = 6;                         // MI_NONFINITE
            leave(J);
            return;
        }
        if (qq.i < 0) {
            if (leader) ctl->status = 1;                         // MI_UNBOUNDED
            leave(J);
            return;
        }
        const int64_t cr = uniform64((int64_t)qq.i);
        const double piv = __longlong_as_double(qq.s);
        const double cmj = qq.w;                                 // col_J[m]
#ifdef MI355X_LA_TIMING
        T4 = wall_clock64();
#endif
        // ---- pivot row through the chain -> prow_J; objective row through pivot J
        double2 y = has_pair ? M2[cr * ldv + p] : make_double2(0.0, 0.0);
        const double v_ccr = (lane < J) ? ld_l2(&t.bk_col[(int64_t)lane * t.bk_stride + cr]) : 0.0;
        const bool own = has_pair && slot >= 0 && p == (slot >> 1);
        // basis[cr] has ONE reader / writer per shard and step: the thread that owns the slot (compact
        // owner: it needs the leaving column for the maps), the leader everywhere else
        const bool keeper = slot >= 0 ? own : leader;
        const int64_t leaving = keeper ? ld_l2(&t.basis[cr]) : -1;
        double2 pi_all[KMAX];
        la_prefetch(pi_all, s_pi, J);
        drain_vmem();                  // the loads -- and the col_J entry / granules stored above
        y = la_chain_row<KMAX>(y, pi_all, v_ccr, J, my_sm, (unsigned)__ballot((lane < J) & (v_cr == cr)), wave_sm);
        pr = make_double2(0.0, 0.0);
        if (has_pair) {
            pr = scale_pair(t, p, y, piv, slot);
            st_wt(&t.bk_prow[(int64_t)J * ld + 2 * p], pr.x);
            st_wt(&t.bk_prow[(int64_t)J * ld + 2 * p + 1], pr.y);
            z.x = pend(z.x, 2 * p     == slot, false, cmj, pr.x);
            z.y = pend(z.y, 2 * p + 1 == slot, false, cmj, pr.y);
        }
        s_pi[J][tid] = pr;
        if (own) {                                               // the slot changes hands
            if (2 * p == slot) l0 = leaving; else l1 = leaving;
            st_wt(&t.p2l[slot], leaving);
            st_wt(&t.l2p[leaving], slot);
            st_wt(&t.l2p[ec], (int64_t)-1);
            my_sm |= 1ull << (J + 32 * (int)(slot & 1));
            la_store_slot_mask(t, p, my_sm, J);
        }
        if (keeper) {
            st_wt(&t.basis[cr], ec);                             // src/simplex.lisp:358 (GLOBAL column indices on every shard)
            blk->prev[J] = leaving;
        }
        if (has_row && r == cr) {
            my_rm |= 1u << J;
            t.bk_rmask[r] = my_rm;
        }
        if (__any(has_row && r == cr)) wave_rm |= 1u << J;
        if (__any(own))                wave_sm |= 1u << J;
        if (leader) la_commit(t, c0, J, ec, cr, slot);           // the one writer of these words
        if (lane == J) { v_cr = cr; v_sl = slot; }
#ifdef MI355X_LA_TIMING
        T5 = wall_clock64();
        if (leader && blockIdx.y == 0) {                         // per-phase clocks of the leader, in the (otherwise unused) rhs buffer
            double *d = t.rhs + J * 8;
            d[0] += 1.0; d[1] += (double)(T1 - T0); d[2] += (double)(T1b - T1); d[3] += (double)(T2 - T1b);
            d[4] += (double)(T3 - T2); d[5] += (double)(T4 - T3); d[6] += (double)(T5 - T4);
        }
#endif
    }
    leave(ksteps);
}

// After a lost exchange (k_la_rollback for a shard): the sweep applied the pivots EVERY workgroup
// completed; the bookkeeping of the one beyond (the leader may have recorded it) is taken back.  basis[cr]
// and the column maps of a pivot are written by one thread each (`keeper` / `own` above), so what was
// written is recognised by basis[cr] == ec.
__global__ void k_shard_la_rollback(TabView t, int la_nw)
{
    BlockCtl *blk = t.blk;
    Ctl *ctl = t.ctl;
    const int n = (int)blk->n_pending;
    const unsigned stamp = (unsigned)blk->stamp;
    if (n == 0 || stamp == 0u) return;
    const int keep = committed_pivots(blk, n, stamp, la_nw);
    for (int i = n - 1; i >= keep; --i) {
        const int64_t cr = blk->cr[i], slot = blk->slot[i], ec = blk->ec[i];
        if (t.basis[cr] == ec) {
            const int64_t prev = blk->prev[i];
            if (slot >= 0 && t.p2l && t.p2l[slot] == prev) {
                t.p2l[slot] = ec;
                t.l2p[ec] = slot;
                t.l2p[prev] = -1;
            }
            t.basis[cr] = prev;
        }
        ctl->n_pivots -= 1;
        ctl->trace_n -= 1;
    }
    blk->n_pending = keep;
}
