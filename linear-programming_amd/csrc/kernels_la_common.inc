// kernels_la_common.inc -- what the look-aheads of a whole block share (k_la_block, k_shard_la_block and,
// for the chain link and the reductions, k_batch_block): the (value, index) reductions, the two chains
// through the pending pivots, the exchange record's format, the workgroup record's front half and the
// block's bookkeeping.  ONE copy each: a change to a chain link or to the wire format is made here.
// Part of simplex_kernels.hip (ONE translation unit: included there, in this order, inside namespace mi355x).

constexpr int kLaThreads = 256, kLaWaves = kLaThreads / 64;
constexpr unsigned kEmptyIdx = 0x7fffffffu;

__device__ __forceinline__ double lane_value_dyn(double v, int lane)    // lane: uniform, run-time
{
    return lane_value(v, __builtin_amdgcn_readfirstlane(lane));
}
__device__ __forceinline__ int64_t lane_value_dyn(int64_t v, int lane)
{
    return lane_value(v, __builtin_amdgcn_readfirstlane(lane));
}

__device__ __forceinline__ unsigned long long dbits(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ __forceinline__ double join_bits(unsigned long long lo, unsigned long long hi)
{
    return __longlong_as_double((long long)(((hi & 0xffffffffull) << 32) | (lo & 0xffffffffull)));
}

// The reductions of the look-ahead move (value, 32-bit index) pairs only -- half the DPP /
// ds_bpermute traffic of a ValIdx -- and fetch the winner's payload from the lane that holds it
// afterwards (indices are unique, so that lane is).  Same decision rule, same tree as
// vi_min / wave_reduce_min.
struct Cand { double v; int i; };                                // i < 0: empty
__device__ __forceinline__ Cand cand_min(Cand a, Cand b)
{
    const bool a_empty = a.i < 0, b_empty = b.i < 0;
    const bool better  = (b.v < a.v) | ((b.v == a.v) & (b.i < a.i));
    const bool take_b  = a_empty | (!b_empty & better);
    Cand r;
    r.v = take_b ? b.v : a.v;
    r.i = take_b ? b.i : a.i;
    return r;
}
template <int CTRL> __device__ __forceinline__ Cand dpp_cand(Cand x)
{
    Cand y;
    y.v = __longlong_as_double(dpp64<CTRL>(__double_as_longlong(x.v)));
    y.i = __builtin_amdgcn_update_dpp(x.i, x.i, CTRL, 0xf, 0xf, false);
    return y;
}
__device__ __forceinline__ Cand shfl_down_cand(Cand x, int off)
{
    Cand y;
    y.v = __shfl_down(x.v, off, 64);
    y.i = __shfl_down(x.i, off, 64);
    return y;
}
// winner of the wave in EVERY lane, plus the lane that holds it (-1: all empty)
__device__ __forceinline__ Cand wave_reduce_cand(Cand x, int &src)
{
    const int mine = x.i;
    x = cand_min(x, shfl_down_cand(x, 32));
    x = cand_min(x, shfl_down_cand(x, 16));
    x = cand_min(x, dpp_cand<0x108>(x));
    x = cand_min(x, dpp_cand<0x104>(x));
    x = cand_min(x, dpp_cand<0x102>(x));
    x = cand_min(x, dpp_cand<0x101>(x));
    x.v = lane_value(x.v, 0);
    x.i = __builtin_amdgcn_readfirstlane(x.i);
    const unsigned long long m = __ballot((mine == x.i) & (x.i >= 0));
    src = m ? (int)__ffsll((long long)m) - 1 : -1;
    return x;
}
__device__ __forceinline__ int64_t lane_pick(int64_t v, int src) { return lane_value_dyn(v, src < 0 ? 0 : src); }
__device__ __forceinline__ double  lane_pick(double v, int src)  { return lane_value_dyn(v, src < 0 ? 0 : src); }
__device__ __forceinline__ int     lane_pick(int v, int src)
{
    return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src < 0 ? 0 : src));
}

// The same arg-min in ~30 instead of ~140 instructions for the common case -- no NaN among the
// wave's candidates and a unique minimum: the minimum VALUE by a butterfly of v_min_f64 (gfx950's
// v_permlane32_swap / v_permlane16_swap across the rows of 16 lanes, DPP row rotations inside
// them; every lane ends up with it), then the lane that holds it by a ballot.  Without NaNs the
// lexicographic (value, index) minimum is unique and independent of the reduction order, so this
// IS the tree's winner; with a NaN candidate (vi_min is then order dependent) or an exact tie
// (lowest index decides) the tree itself runs.
typedef unsigned v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double min_f64(double a, double b)     // operands are never NaN here
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double wave_allmin_f64(double x)
{
    {   // lanes l and l ^ 32: whichever half a swap puts where, {r.x, r.y} is the pair in every lane
        const long long b = __double_as_longlong(x);
        const unsigned lo = (unsigned)b, hi = (unsigned)((unsigned long long)b >> 32);
        const v2u l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const v2u h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        x = min_f64(__longlong_as_double((long long)(((unsigned long long)h2.x << 32) | l2.x)),
                    __longlong_as_double((long long)(((unsigned long long)h2.y << 32) | l2.y)));
    }
    {   // rows 0 <-> 1, 2 <-> 3
        const long long b = __double_as_longlong(x);
        const unsigned lo = (unsigned)b, hi = (unsigned)((unsigned long long)b >> 32);
        const v2u l2 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const v2u h2 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        x = min_f64(__longlong_as_double((long long)(((unsigned long long)h2.x << 32) | l2.x)),
                    __longlong_as_double((long long)(((unsigned long long)h2.y << 32) | l2.y)));
    }
    x = min_f64(x, __longlong_as_double(dpp64<0x128>(__double_as_longlong(x))));   // row_ror:8
    x = min_f64(x, __longlong_as_double(dpp64<0x124>(__double_as_longlong(x))));   // row_ror:4
    x = min_f64(x, __longlong_as_double(dpp64<0x122>(__double_as_longlong(x))));   // row_ror:2
    x = min_f64(x, __longlong_as_double(dpp64<0x121>(__double_as_longlong(x))));   // row_ror:1
    return x;
}
__device__ __forceinline__ Cand wave_argmin(Cand x, int &src)
{
    const bool valid = x.i >= 0;
    if (__any(valid & (x.v != x.v))) return wave_reduce_cand(x, src);
    const double key = valid ? x.v : __builtin_huge_val();
    const double vmin = wave_allmin_f64(key);
    const unsigned long long mask = __ballot(valid & (key == vmin));
    if (__popcll(mask) > 1) return wave_reduce_cand(x, src);
    src = mask ? (int)__ffsll((long long)mask) - 1 : -1;
    Cand r;
    r.v = lane_pick(x.v, src);
    r.i = mask ? lane_pick(x.i, src) : -1;
    if (!mask) r.v = 0.0;
    return r;
}

// ---- the chains through the pending pivots ---------------------------------------------------
// One link in its general form, the product already rounded (pend with the multiplication taken out):
// the element sits in the slot pending pivot i gave up -> it restarts from that pivot's unit column;
// on pivot row i -> it becomes the pending row's entry; otherwise the rounded difference.  The two bits
// are VALUES, so k_batch_block's 16 + 16 and the persistent kernels' 32 + 32 mask bits both fit.
__device__ __forceinline__ double la_link(double x, bool is_slot, bool is_cr, double prod, double rowv)
{
    if (is_slot) x = is_cr ? 1.0 : 0.0;
    const double d = x - prod;                                 // rounded difference
    return is_cr ? rowv : d;
}
__device__ __forceinline__ double2 la_link2(double2 y, bool slot_x, bool slot_y, bool is_cr, double2 prod, double2 rowv)
{
    y.x = la_link(y.x, slot_x, is_cr, prod.x, rowv.x);
    y.y = la_link(y.y, slot_y, is_cr, prod.y, rowv.y);
    return y;
}

// This thread's LDS operands of a chain ([pivot][thread]: conflict-free) into registers, requested in
// ONE go so that they travel with the caller's memory loads instead of group by group inside the chain
// (at 24 pending pivots that was six dependent LDS round trips per chain).  Entries from J on are the
// launch's +0.0 (la_zero_pending); groups that start at or past J are not read at all.
template <int KMAX, class T>
__device__ __forceinline__ void la_prefetch(T (&dst)[KMAX], const T (&src)[KMAX][kLaThreads], int J)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i0 = 0; i0 < KMAX; i0 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[i0 + k] = T();
        if (i0 < J) {
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[i0 + k] = src[i0 + k][tid];
        }
    }
}

// With ONE wave per SIMD every instruction of the critical wave costs its full issue + latency,
// so the chains are written for instruction count: the product of a link does not depend on the
// chained value (four independent multiplications, then four dependent subtractions), the two rare
// exceptions of a link are bit tests on masks the thread keeps anyway (my_rm, my_sm) plus a
// wave-uniform mask over the pending pivots, and a group of four none of whose links is an exception
// for any lane of the wave runs the bare chain: ONE uniform branch per four links.  Links i >= J of a
// group are exact identities (operands +0.0: x - (+0.0) == x bit for bit).
//
// Entering column: a = my row's entry, ci = my row's entries of the pending columns, lane i of v_pa =
// prow_i[slot].  my_rm bit i: my row is pivot row i; slmask bit i (uniform): pivot i gave up the
// entering column's slot; wave_rm bit i: SOME lane of my wave is on pivot row i.
template <int KMAX>
__device__ __forceinline__ double la_chain_col(double a, const double (&ci)[KMAX], double v_pa, int J,
                                               unsigned my_rm, unsigned slmask, unsigned wave_rm)
{
    const unsigned gen = slmask | wave_rm;                             // links that need the general form
#pragma unroll
    for (int i0 = 0; i0 < KMAX; i0 += 4) {
        if (i0 < J) {
            double prod[4], pa[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                pa[k] = lane_value(v_pa, i0 + k);
                prod[k] = ci[i0 + k] * pa[k];                          // rounded product
            }
            if (((gen >> i0) & 0xfu) == 0u) {                          // (uniform)
#pragma unroll
                for (int k = 0; k < 4; ++k) a = a - prod[k];           // rounded differences
            } else {                                                   // (rare)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    a = la_link(a, (slmask >> (i0 + k)) & 1u, (my_rm >> (i0 + k)) & 1u, prod[k], pa[k]);
            }
        }
    }
    return a;
}
// Pivot row: y = my pair of the row, pi = my pair's entries of the pending rows, lane i of v_ccr =
// col_i[cr].  my_sm bits i, 32 + i: my pair's even / odd column is the slot pivot i gave up; crmask bit
// i (uniform): pivot i's row is the new pivot row; wave_sm bit i: SOME lane of my wave holds slot i.
template <int KMAX>
__device__ __forceinline__ double2 la_chain_row(double2 y, const double2 (&pi)[KMAX], double v_ccr, int J,
                                                unsigned long long my_sm, unsigned crmask, unsigned wave_sm)
{
    const unsigned gen = crmask | wave_sm;
#pragma unroll
    for (int i0 = 0; i0 < KMAX; i0 += 4) {
        if (i0 < J) {
            double2 prod[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double ccr = lane_value(v_ccr, i0 + k);
                prod[k].x = ccr * pi[i0 + k].x;                        // rounded products
                prod[k].y = ccr * pi[i0 + k].y;
            }
            if (((gen >> i0) & 0xfu) == 0u) {                          // (uniform)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    y.x = y.x - prod[k].x;
                    y.y = y.y - prod[k].y;
                }
            } else {                                                   // (rare)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    y = la_link2(y, (my_sm >> (i0 + k)) & 1ull, (my_sm >> (32 + i0 + k)) & 1ull,
                                 (crmask >> (i0 + k)) & 1u, prod[k], pi[i0 + k]);
            }
        }
    }
    return y;
}

// ---- the exchange record's format ------------------------------------------------------------
// Eight granules {tag, 32 bits of payload}.  c = the winner (value, index; i < 0: empty), cs = what
// rides with it (PRICE: its slot, 32 bits; RATIO: 64 bits), u / x2 = the two doubles of the caller.
//   PRICE: v v i s u u x2 x2          RATIO: v v i s s u u lost
// flags bit 0 (non-finite) is bit 31 of granule 2; flags bit 1 ("a peer's column was lost") is granule 7
// of a RATIO record: k_shard_la_block's only, k_la_block writes and reads 0 there.
// WHERE a granule is stored (layout, scope of the store) is the caller's business: pack_rec hands lane k
// (0 .. 7) the payload of granule k.
template <bool PRICE>
__device__ __forceinline__ unsigned pack_rec(Cand c, unsigned flags, int64_t cs, double u, double x2, int lane)
{
    const unsigned long long vb = dbits(c.v), sb = (unsigned long long)cs, ub = dbits(u), wb = dbits(x2);
    const unsigned iw = (c.i < 0 ? kEmptyIdx : (unsigned)c.i) | ((flags & 1u) ? 0x80000000u : 0u);
    const unsigned word[8] = { (unsigned)vb, (unsigned)(vb >> 32), iw, (unsigned)sb,
                               PRICE ? (unsigned)ub : (unsigned)(sb >> 32),
                               PRICE ? (unsigned)(ub >> 32) : (unsigned)ub,
                               PRICE ? (unsigned)wb : (unsigned)(ub >> 32),
                               PRICE ? (unsigned)(wb >> 32) : ((flags >> 1) & 1u) };
    unsigned val = word[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) val = lane == k ? word[k] : val;
    return val;
}
// ru: the first double; rw: the second one (PRICE only).  A record that is not `valid` decodes as empty.
template <bool PRICE>
__device__ __forceinline__ void decode_rec(const unsigned long long (&g)[8], bool valid, Cand &x, int64_t &xs,
                                           unsigned &fl, double &ru, double &rw)
{
    const unsigned iw = (unsigned)g[2];
    x.v = 0.0; x.i = -1; xs = 0; fl = 0u;
    if (valid) {
        x.v = join_bits(g[0], g[1]);
        x.i = (iw & kEmptyIdx) == kEmptyIdx ? -1 : (int)(iw & kEmptyIdx);
        xs = PRICE ? (int64_t)(g[3] & 0xffffffffull) : (int64_t)(((g[4] & 0xffffffffull) << 32) | (g[3] & 0xffffffffull));
        fl = (iw >> 31) | (PRICE ? 0u : (((unsigned)g[7] & 1u) << 1));
    }
    ru = PRICE ? join_bits(g[4], g[5]) : join_bits(g[5], g[6]);
    rw = PRICE ? join_bits(g[6], g[7]) : 0.0;
}

// ---- one record per workgroup: the front half --------------------------------------------------
// A wave's winner on its way into the workgroup's record -- and a quarter's partial winner on its way
// out of a shared poll (sh_poll_quarter: x2 is then the "from" double).
struct LaWaveRec { double v; int i; unsigned f; int64_t s; double u, x2; };

// the four entries folded in wave order (same rule; the minimum does not depend on the shape of the
// tree), their flags ORed; returns which entry won
__device__ __forceinline__ int fold_waves(const LaWaveRec *s, Cand &c, unsigned &flags)
{
    int ww = 0;
    c.v = s[0].v; c.i = s[0].i; flags = s[0].f;
#pragma unroll
    for (int k = 1; k < kLaWaves; ++k) {
        Cand o; o.v = s[k].v; o.i = s[k].i;
        const Cand r = cand_min(c, o);
        ww = (r.i != c.i) ? k : ww;                               // (indices are unique; two empty candidates: either)
        c = r;
        flags |= s[k].f;
    }
    return ww;
}
// Every wave's winner (c, wf, cs) and its two doubles -> s_wv[wave]; ONE barrier (reached by every
// thread of the workgroup); then, in the FIRST wave only, the workgroup's record: the winner of the
// four, the winner's own double from the winning wave, the "from" double (PRICE: x2, RATIO: u) from wave
// wave_from if this workgroup is the one that owns it (from_here).  The other waves' arguments are
// left as they were.  OWN_U (k_la_block's RATIO records): the first double is the winner's own, as a PRICE
// record's, and nothing rides "from" anywhere.
template <bool PRICE, bool OWN_U = false>
__device__ __forceinline__ void wg_record(LaWaveRec *s_wv, Cand &c, unsigned &wf, int64_t &cs, double &u, double &x2,
                                          bool from_here, int wave_from)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { LaWaveRec r; r.v = c.v; r.i = c.i; r.f = wf; r.s = cs; r.u = u; r.x2 = x2; s_wv[wave] = r; }
    __syncthreads();
    if (wave != 0) return;
    const int ww = fold_waves(s_wv, c, wf);
    cs = s_wv[ww].s;
    if (PRICE) { u = s_wv[ww].u; x2 = from_here ? s_wv[wave_from].x2 : 0.0; }
    else       { u = OWN_U ? s_wv[ww].u : (from_here ? s_wv[wave_from].u : 0.0); x2 = 0.0; }
}

// ---- the block's bookkeeping -------------------------------------------------------------------
// What k_la_block and k_shard_la_block write identically.  What they do NOT: every store another
// workgroup reads inside the launch (st_x(.., local) there, st_wt here) and the shard's keeper /
// blk->prev, which has no counterpart -- those stay spelled out in the two kernels.
//
// A new block starts (whatever the status): pending list, stamp (the sweep applies the list only
// under this launch's stamp -- had the leader's workgroup never run, the list would be the previous
// block's; not behind a launch that lost an exchange: the host's recovery reads that launch's list)
// and thread g's OWN mask words, which only it ever writes.  Both slot masks whatever KMAX: a wide
// sweep ORs the second one in, and a block of <= 16 pivots behind an earlier block of 24 on the same
// handle must not see that block's bits 16 .. 23.
__device__ __forceinline__ void la_zero_masks(const TabView &t, int64_t g)
{
    if (g < t.bk_stride) t.bk_rmask[g] = 0u;
    if (g < (t.ld >> 1)) { t.bk_smask[g] = 0u; if (t.bk_smask2) t.bk_smask2[g] = 0u; }
}
__device__ __forceinline__ void la_block_begin(const TabView &t, const Ctl &c0, bool leader, int64_t g, unsigned epoch_base)
{
    if (leader && c0.status != kSyncLost) { t.blk->n_pending = 0; t.blk->stamp = epoch_base; }
    la_zero_masks(t, g);
}
// My entries of the pending columns / rows start out as +0.0: a group of four links that reaches past
// the last pending pivot then multiplies (+0.0) x (+0.0) for the missing ones -- x - (+0.0) == x bit for
// bit -- without a compare and two to four selects per LINK to zero stale operands (48 LDS stores per
// thread and launch against ~3 of ~9 instructions per link of both chains of every step).
template <int KMAX>
__device__ __forceinline__ void la_zero_pending(double (&s_ci)[KMAX][kLaThreads], double2 (&s_pi)[KMAX][kLaThreads])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < KMAX; ++i) { s_ci[i][tid] = 0.0; s_pi[i][tid] = make_double2(0.0, 0.0); }
}
// pair p's slot masks in the sweeps' layout (slot_mask_set): pivots 0 .. 15 in bk_smask, 16 .. 31 in
// bk_smask2, even column in the low half, odd column in the high half; pivot J has just set its bit
__device__ __forceinline__ void la_store_slot_mask(const TabView &t, int64_t p, unsigned long long my_sm, int J)
{
    if (J < 16) t.bk_smask[p]  = (unsigned)(my_sm & 0xffffull) | ((unsigned)((my_sm >> 32) & 0xffffull) << 16);
    else        t.bk_smask2[p] = (unsigned)((my_sm >> 16) & 0xffffull) | ((unsigned)((my_sm >> 48) & 0xffffull) << 16);
}
// pivot J of the block is decided: control block, trace and pending list (the leader, their one writer)
__device__ __forceinline__ void la_commit(const TabView &t, const Ctl &c0, int J, int64_t ec, int64_t cr, int64_t slot)
{
    Ctl *ctl = t.ctl;
    BlockCtl *blk = t.blk;
    const int64_t tn = c0.trace_n + J;
    ctl->ec = ec;
    ctl->cr = cr;
    ctl->slot = slot;
    if (t.trace_ec && tn < t.trace_cap) { t.trace_ec[tn] = ec; t.trace_cr[tn] = cr; }
    ctl->trace_n  = tn + 1;
    ctl->n_pivots = c0.n_pivots + J + 1;
    blk->cr[J] = cr;
    blk->slot[J] = slot;
    blk->ec[J] = ec;
    blk->n_pending = J + 1;
}
