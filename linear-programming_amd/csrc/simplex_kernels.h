// simplex_kernels.h -- device-side data structures and launcher prototypes of the
// MI355X dense-simplex backend (host side of the launchers lives in
// simplex_kernels.hip, the C ABI in simplex_capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xwide.h"

namespace mi355x {

// Common Lisp DOUBLE-FLOAT-EPSILON = 2^-53 (1 + 2^-52)  (src/utils.lisp:84-124)
constexpr double kClEpsilon = 1.1102230246251568e-16;

// device-side status word; values >= 0 other than kRunning are the MI_* outcomes
constexpr int32_t kRunning = 100;
// compact representation only: the entering column holds an inf / NaN.  The reference would
// turn every basic column into NaNs (x - inf*0), which a representation that does not store
// basic columns cannot reproduce: the pivot is NOT applied and the host re-runs it on the dense
// tableau (single tableaux, batches) or reports MI_NONFINITE (compact column shards).
constexpr int32_t kNeedDense = 101;
// persistent look-ahead kernel only: a workgroup gave up waiting for the others' records (cannot
// happen while all its workgroups are resident; bounded so that a bug reports instead of hanging)
constexpr int32_t kSyncLost = 102;
// resident solve only: an exchange was lost AFTER the first one (the first is the co-residency
// check and ends as kSyncLost): cannot happen short of a hung GPU; nothing was written back, but
// the launch may have been partly observed -- reported as an error, never as a result
constexpr int32_t kResidentStuck = 103;

// Control block living in device memory: the whole price -> ratio -> pivot loop
// runs without host round trips, kernels communicate through this struct.
struct Ctl {
    int32_t status;       // kRunning, or MI_OPTIMAL / MI_UNBOUNDED / MI_MAX_PIVOTS
    int32_t poison;       // set by k_select_gather when it meets a non-finite column entry
    int64_t ec;           // entering column chosen by the last select
    int64_t cr;           // pivot row chosen by the last select
    int64_t n_pivots;     // pivots since the last reset
    int64_t max_pivots;   // 0 = no cap
    int64_t trace_n;      // pivots recorded in the trace buffers
    int64_t slot;         // physical column of `ec` (== ec unless the representation is compact)
};

// Blocked pivoting (single compact tableaux): up to kMaxBlock pivots are SELECTED ahead of the
// tableau update -- each look-ahead step evaluates just the objective row, one column, the RHS
// column and one row as they would be after the pending pivots -- and then applied to every
// stored element in ONE sweep (k rank-1 updates per element, in pivot order, operands and
// roundings unchanged).  This block lives next to the control block.
constexpr int kMaxBlock = 16;
constexpr int kLaBlockMax = 24;            // pending pivots one launch of the persistent look-ahead can hold (6 KB of LDS each)
// WIDE blocks (round 4): where the sweep dominates an iteration -- tableaux / column shards of a GB
// and more, which the persistent look-ahead does not fit anyway -- up to kWideBlock pivots are
// pending per pass (24 or 28 in practice: what three waves per SIMD can hold of prow operands,
// kernels_sweep.inc).  The list, the col_i / prow_i buffers and the row masks have room for
// kWideBlock pivots on every single-tableau handle; pivots 16 .. 31 record their slot hand-overs in
// a second mask array (bk_smask2, layout of bk_smask).  Everything that lives in LDS (persistent
// look-ahead, batches) stays at kMaxBlock.
constexpr int kWideBlock = 32;
struct BlockCtl {
    int64_t n_pending;            // pivots selected but not yet applied by a sweep
    int64_t stamp;                // persistent look-ahead: epoch base of the launch that wrote the list
    int64_t cr[kWideBlock];       // their pivot rows ...
    int64_t slot[kWideBlock];     // ... and the physical slots their entering columns gave up
    // persistent look-ahead: (stamp << 8 | steps) -- how many steps of the launch with that stamp
    // workgroup w completed (everything it owns of col_i / prow_i stored).  The leader raises
    // n_pending on its own; a workgroup that gave up on an exchange (kSyncLost) may be one step
    // behind it, so the sweep applies min(n_pending, min over w of steps) pivots and the host's
    // recovery takes the bookkeeping of the pivot beyond that back (k_la_rollback).
    int64_t done[256];            // kMaxShardLaWorkgroups entries (single tableaux use the first kMaxLaWorkgroups)
    int64_t ec[kWideBlock];       // persistent look-ahead: the logical columns that entered (k_la_rollback)
    int64_t prev[kWideBlock];     // column shards (k_shard_la_block): basis[cr] as it was before the pivot (k_shard_la_rollback)
};

// Record one workgroup of the persistent look-ahead kernel publishes per exchange: eight
// self-validating granules {tag = 32-bit epoch, 32 bits of payload}, each written by one 8-byte
// store (a reduction candidate (value, index, payload), a flag and two doubles; layout in
// simplex_kernels.hip, la_exchange).  Since round 5 the buffer of kMaxLaRecords records is laid out
// TRANSPOSED -- granule j of record R at 8-byte word j * kMaxLaRecords + R -- so that the collecting
// wave reads consecutive granules with consecutive lanes; ExchRec only sizes the buffer.
struct ExchRec {
    unsigned long long g[8];
};
// Up to kLaWaveRecordsMaxNw workgroups every WAVE publishes a record and every wave polls them all (the
// launch can sit on one XCD: 32 CUs); from there up to kMaxLaWorkgroups every WORKGROUP publishes one
// record (its four waves' winners reduced through LDS) and its first wave polls -- the poll traffic of
// the first form grows with the square of the workgroups, the LDS hop of the second does not
// (DESIGN_experiments.md R5.16 / R5.18).  Both forms use the same transposed buffers.
constexpr int kLaWaveRecordsMaxNw = 32;
constexpr int kMaxLaWorkgroups = 64;
// A column shard's persistent look-ahead (k_shard_la_block, round 6) runs one workgroup per 256 rows of the
// WHOLE column -- 129 for config 5 however many GPUs share it -- with a record (a 64-byte line) per workgroup
// and one polling wave each; the sweeps read BlockCtl::done with up to four entries per lane.
constexpr int kMaxShardLaWorkgroups = 256;
static_assert(sizeof(BlockCtl::done) / sizeof(int64_t) == kMaxShardLaWorkgroups, "BlockCtl::done");
constexpr int kMaxLaRecords = 4 * kLaWaveRecordsMaxNw;  // one record per wave of a 256-thread workgroup / one per workgroup
static_assert(kMaxLaWorkgroups <= 64 && kMaxLaWorkgroups <= kMaxLaRecords,
              "a sweep's wave reads BlockCtl::done with one lane per workgroup; per-workgroup records are collected one per lane");

// Column partition, exchange mode 2 (the shards write into each other's fine-grained buffers):
// layout of one shard's exchange buffer in 8-byte granules {tag = pivot number, 32 bits of payload}
//     pairs  [2 parities][world][4]      the local pricing winners (key, global column)
//     column [2 parities][2 x rows_p]    the entering column
// and what a kernel needs to take part: every shard's buffer as THIS process maps it, the own one,
// the own rank, the tag of this pivot and the poll bound.  peers == nullptr: not in this mode.
constexpr int32_t kExchangeLost = 104;      // device status: a peer's data never arrived (-> MI_RCCL_ERROR)
struct P2pLayout {
    int world; int64_t rows_p;
    __host__ __device__ int64_t pair_off(unsigned par, int r) const { return ((int64_t)par * world + r) * 4; }
    __host__ __device__ int64_t col_off(unsigned par) const { return (int64_t)2 * world * 4 + (int64_t)par * 2 * rows_p; }
    __host__ __device__ int64_t granules() const { return (int64_t)2 * world * 4 + (int64_t)4 * rows_p; }
};
struct P2pArgs {
    unsigned long long *const *peers = nullptr;
    unsigned long long *mine = nullptr;
    P2pLayout lay{};
    int rank = 0;
    unsigned epoch = 0, max_spins = 0;
};

// One tableau in HBM.  Row-major, leading dimension ld (a multiple of 16 doubles so
// that every row starts on a 128-byte boundary and 16-byte vector accesses never
// straddle rows); columns [cols, ld) are padding and hold zeros.
struct TabView {
    double  *M;
    int64_t  ld, rows, cols;
    int64_t *basis;       // rows-1 entries
    double  *col;         // snapshot of the entering column before the pivot, rows entries
    double  *prow;        // normalised pivot row, ld entries (padding zero)
    double  *rhs;         // contiguous snapshot of the RHS column (column shards only), rows entries
    Ctl     *ctl;
    int64_t *trace_ec;    // may be null
    int64_t *trace_cr;
    int64_t  trace_cap;
    double  *part_v;      // per-wave pricing partials left by k_update (key space); the
    int64_t *part_i;      // upper half holds the ratio-test partials of the split select
    int64_t *part_s;      // payload of each partial (physical slot / pivot-element bits)
    int      part_cap;
    // compact representation (non-basic columns + RHS only): physical slot <-> logical column
    // maps; both null for the dense logical layout
    int64_t *p2l;         // cols-1 entries: logical column stored in physical slot j
    int64_t *l2p;         // logical var_count entries: slot of a logical column, -1 if basic
    int64_t  col_bias;    // dense column shard: global index of its column 0 (0 everywhere else)
    // blocked pivoting: entering-column snapshots (kMaxBlock x bk_stride), normalised pivot rows
    // (kMaxBlock x ld of the view in use) and the pending list; null when not available
    double   *bk_col, *bk_prow;
    BlockCtl *blk;
    int64_t   bk_stride;
    // bit i of bk_rmask[r]: row r is the pivot row of pending pivot i; bits i / 16+i of
    // bk_smask[pair]: the even / odd column of that pair is the slot pending pivot i gave up
    uint32_t *bk_rmask, *bk_smask;
    uint32_t *bk_smask2;          // slot hand-overs of pending pivots 16 .. 31 (wide blocks; null for batches)
    ExchRec  *la_px, *la_rx;      // kMaxLaRecords pricing / ratio records (persistent look-ahead)
    // batch of n_lps same-shape LPs: per-LP element strides (all zero for a single tableau)
    int64_t  n_lps;
    int64_t  zs_M, zs_basis, zs_col, zs_prow, zs_part, zs_p2l, zs_l2p;
    int64_t  zs_bk, zs_bkp, zs_rm, zs_sm;       // per-LP block state: bk_col, bk_prow, bk_rmask, bk_smask (blk: one BlockCtl each)
};

// One shard of a k_shard_la_block launch (an array of these in device memory, indexed by blockIdx.y:
// one entry per device-local shard -- one where a shard has its GPU to itself, the logical shards of a
// one-GPU test box all in ONE launch, whose workgroups are then co-resident by construction).
struct ShardLaunch {
    TabView t;
    unsigned long long *const *peers;   // every shard's exchange buffer as this process maps it
    unsigned long long *mine;           // this shard's own
    int64_t col_offset;                 // dense shards: global index of local column 0
    int rank, pad;
};

struct UpdateShape {
    int strips, strip_pairs, tr, row_chunks, waves_per_block, n_partials;
};

// select: price -> gather column -> ratio test -> normalise pivot row (one workgroup)
// n_part > 0: price from the partials the preceding launch_update(..., price=1) left behind
void launch_select(const TabView &t, int is_max, double fp_factor, int n_part, hipStream_t s);
// the same select as two multi-workgroup launches (large tableaux)
void launch_select_split(const TabView &t, int is_max, double fp_factor, int n_part, hipStream_t s);
bool select_split_supported(const TabView &t);
// pieces of it, for the step-wise ABI entry points
void launch_price_only(const TabView &t, int is_max, double fp_factor, hipStream_t s);
void launch_ratio_only(const TabView &t, int64_t ec, double fp_factor, hipStream_t s);
void launch_prepare_pivot(const TabView &t, int64_t ec, int64_t cr, hipStream_t s);
// the bandwidth kernel: M[r][c] -= col[r] * prow[c] (r != cr), M[cr][c] = prow[c]
// returns the number of pricing partials written (0 if price == 0)
int  launch_update(const TabView &t, double sgn, int price, hipStream_t s, int64_t launch_index = 0);
void set_alternate_sweep(int on);
// blocked pivoting: look-ahead step j of a block (select pivot j as if pivots 0..j-1 of the block
// had been applied), and the sweep that applies the whole block.  n_part as for launch_select;
// launch_lookahead returns the number of pricing partials it leaves for step j+1.
bool block_supported(const TabView &t);
int  launch_lookahead(const TabView &t, int j, int is_max, double fp_factor, int n_part, hipStream_t s);
// stamp != 0: apply the pending list only if the look-ahead launch with that epoch base wrote it,
// and of it only the pivots all la_nw workgroups of that launch completed (BlockCtl::done)
int  launch_sweep(const TabView &t, int kmax, double sgn, hipStream_t s, unsigned stamp = 0, int la_nw = 0);
// wide blocks: the block sizes k_sweepw is compiled for, and the one a view of this size should run
// with (0: stay at kMaxBlock)
bool wide_block_size_ok(int k);
int  wide_block_default(const TabView &t);
void set_sweep_skew(int rows);             // k_sweepw_ring, one round of workgroups: rows by which the first / last third of the tiles are taller / shorter (-1: by the tile height)
void set_sweep_xmap(int on);               // k_sweepw_ring: workgroup -> (strip, tile) by XCD (see the kernel)
void set_sweepw_ring(int on);              // wide sweeps through the LDS ring (default) or the register form
int  sweep_kind(int kmax);                 // 2 wide pair, 1 k_sweep16, 0 k_sweep<..>: what launch_sweep picks
// after a lost exchange (kSyncLost): undo the bookkeeping (column maps, basis, pivot count, trace)
// of the pivots the leader committed but the sweep did not apply
void launch_la_rollback(const TabView &t, int la_nw, hipStream_t s);
int  la_block_workgroups(const TabView &t);
int  la_launch_workgroups(const TabView &t);
// the whole look-ahead of a block (steps 0 .. ksteps-1) as ONE launch of a few persistent
// workgroups that exchange their reduction candidates through la_px / la_rx; epoch_base (> 0)
// must grow by at least 2*kMaxBlock+2 from launch to launch on the same tableau (the records
// are zeroed whenever the host wraps it around)
bool la_block_supported(const TabView &t);
void launch_la_block(const TabView &t, int ksteps, int is_max, double fp_factor,
                     unsigned epoch_base, hipStream_t s);
// the same with the kernel picked by `form` (a block size: <= kMaxBlock the 16-step look-ahead, above
// it the 24-step one) instead of by ksteps -- prime_block_kernels launches each with 0 steps
void launch_la_block_form(const TabView &t, int form, int ksteps, int is_max, double fp_factor,
                          unsigned epoch_base, hipStream_t s);
// tuning / test hooks of the persistent look-ahead: all its workgroups on one XCD (default on),
// polls before a workgroup gives up waiting (kSyncLost), a workgroup that stops publishing
void set_la_one_xcd(int on);
void set_la_max_spins(unsigned n);
void set_la_fault(int step_plus_1);
void set_sweep_shape(int tr, int nt);      // tuning hook
void set_sweep_impl(int impl);             // tuning / test hook: 0 k_sweep16 for full blocks (default), 1 k_sweep always
UpdateShape update_shape(const TabView &t);
// column-partitioned shards (one shard = one handle)
// x.peers != nullptr (exchange mode 2, FUSED form): the kernel also is the producer / consumer of
// the exchange next to it -- the pricing kernel pushes the pair to every shard, the contribution
// kernel waits for all pairs and (the owner) pushes the column, the split look-ahead step waits for
// the column -- so that a pivot is four launches and no collective
void launch_shard_price(const TabView &t, int is_max, int64_t col_offset, double *out2, int n_part,
                        hipStream_t s, const P2pArgs &x = P2pArgs());
void launch_shard_contribute(const TabView &t, const double *gathered, int n_shards,
                             int64_t col_offset, double fp_factor, int64_t *bits_out,
                             int64_t *ec_out, hipStream_t s);
// forced_cr >= 0: no ratio test, the pivot row is the caller's
void launch_shard_prepare(const TabView &t, const double *col, const int64_t *ec_dev,
                          double fp_factor, hipStream_t s, int64_t forced_cr = -1);
// the owner of logical column ec contributes it (a pivot the caller chose)
void launch_shard_forced_contribute(const TabView &t, int64_t ec, int64_t col_offset, int64_t *bits_out,
                                    int64_t *ec_out, hipStream_t s);
// two-phase hand-over of one compact column shard: slots keep[] of `art` + its RHS copy -> `mt`,
// objective row obj0 re-eliminated with the given scales (src/simplex.lisp:437-451)
void launch_shard_handover(const TabView &art, const TabView &mt, const int64_t *keep, const double *obj0,
                           const double *scales, hipStream_t s);
// ... and their blocked forms: step j of a block (no update), the sweep is launch_sweep
void launch_shard_la_contribute(const TabView &t, int j, const double *gathered, int n_shards,
                                int64_t col_offset, double fp_factor, int64_t *bits_out,
                                int64_t *ec_out, hipStream_t s, const P2pArgs &x = P2pArgs());
int  launch_shard_la_prepare(const TabView &t, int j, const double *col, const int64_t *ec_dev,
                             double fp_factor, int is_max, hipStream_t s, const P2pArgs &x = P2pArgs());
int  launch_shard_p2p_step(const TabView &t, int j, int n_part, int n_shards, int64_t col_offset, double fp_factor,
                           int is_max, int64_t *ec_dev, hipStream_t s, const P2pArgs &x);
// the look-ahead of a whole block of every device-local shard as ONE persistent launch (exchange mode 2;
// kernels_shard_block.inc): workgroups a shard needs (0: not available for this view), the launch, and
// the recovery's bookkeeping roll-back
int  shard_la_block_workgroups(const TabView &t);
void launch_shard_la_block(const ShardLaunch *dev_shards, int n_local, int nw_max, const P2pLayout &lay, int ksteps,
                           int is_max, double fp_factor, unsigned epoch_base, unsigned xepoch_base,
                           unsigned p2p_spins, int hop, hipStream_t s);
void launch_shard_la_rollback(const TabView &t, int la_nw, hipStream_t s);
void set_shard_la_fault(int step_plus_1);  // test hook (test build): as set_la_fault, the last workgroup of the last local shard
bool shard_la_split(const TabView &t);     // the look-ahead step of this shard is the multi-workgroup pair
void set_shard_la_split(int mode);         // tuning / test hook: 0 by size, 1 one workgroup, 2 split over many
// two-phase hand-over (src/simplex.lisp:437-451)
// unit_basis: the basic columns of `art` are known to be exact unit vectors (column-parallel
// re-elimination); otherwise the sequential form
void launch_handover(const TabView &art, const TabView &main_tab, bool unit_basis, hipStream_t s);
void launch_handover_objective_columns(const TabView &mt, hipStream_t s);   // scales in mt.col[0 .. m)
// whole-batch solve, one workgroup per LP (false: an LP does not fit the LDS budget)
bool launch_batch_solve(const TabView &t, int is_max, double fp_factor, hipStream_t s);
// one block of every LP of a batch: look-ahead (one workgroup per LP, 16 pivots selected ahead)
// then ONE sweep launch over all LPs (grid.z = LP); false: not available for this shape
bool launch_batch_block_split(const TabView &t, int is_max, double fp_factor, hipStream_t s);
void set_batch_block(int k);       // tuning hook: pivots per pass of the blocked per-LP kernel (1 = off)
// dense logical tableau <-> compact representation
void launch_verify_basis(const TabView &t, int *flag, hipStream_t s);
void launch_compact(const TabView &dense, const TabView &compact, hipStream_t s);
void launch_expand(const TabView &dense, const TabView &compact, int64_t *brow, hipStream_t s);
void launch_ctl_reset(const TabView &t, int64_t max_pivots, int reset_trace, hipStream_t s);
void launch_ctl_finish(const TabView &t, hipStream_t s);
// the first n control blocks -> pinned coherent host memory, then `seq` -> *host_seq (system-scope release)
void launch_ctl_publish(const TabView &t, int64_t n, void *host_dst, unsigned long long *host_seq,
                        unsigned long long seq, hipStream_t s);
// `from` -> kRunning (kNeedDense: after the host has rebuilt the dense tableau; kSyncLost: after
// it has switched the handle to the two-launch look-ahead)
void launch_ctl_resume(const TabView &t, hipStream_t s, int32_t from);
// build-tableau's rules for a constraint row (src/simplex.lisp:243-265, 296-300): the one copy every assembly
// kernel (kernels_assemble.inc and the family files) and the host's checks use.
// The row's word: bit 0 = its right-hand side is negative, so the row is negated whole and its sense flipped
// (:243-252); bits 1-2 = its sense after that: 0 `<=` (slack +1, basic), 1 `>=` (slack -1, artificial), 2 `=`
// (no slack, artificial).
XW_HD inline int row_word(bool rhs_negative, int sense)
{
    const int op = sense == 2 ? 2 : (rhs_negative ? 1 - sense : sense);
    return (rhs_negative ? 1 : 0) | (op << 1);
}
XW_HD inline bool row_word_artificial(int word) { return (word >> 1) != 0; }
// ab[R], row R's artificial-basis entry: its slack column for a `<=` row; for an artificial row num_cols (the
// main tableau's columns) until the artificial columns are dealt, in DECREASING row order (push, :257, :261,
// :296-300), then that column, num_cols - 1 + rank.  One thread.
XW_HD inline void deal_artificial_columns(int32_t *ab, int m, int32_t num_cols)
{
    int32_t n = 0;
    for (int R = m - 1; R >= 0; --R)
        if (ab[R] == num_cols) ab[R] = num_cols - 1 + n++;
}
// from a dealt ab[R]: is the row artificial, and its main-basis entry (num_cols for an artificial row); the
// artificial basis is ab[R] itself
XW_HD inline bool    ab_artificial(int32_t ab, int32_t num_cols) { return ab >= num_cols - 1; }
XW_HD inline int32_t ab_main_basis(int32_t ab, int32_t num_cols) { return ab >= num_cols - 1 ? num_cols : ab; }
// branch-and-bound node tableaux (kernels_bb.inc): the base problem's GENERAL-form main tableau
// (tight rows x cols, last row = objective), per base row the build-tableau negation flag, its basis,
// and the var-mapping; the node rows of LPs [first, first + n_lps) of the descriptor arrays
struct BBBaseView {
    const double  *M;                 // rows x cols, tight
    int64_t        rows, cols, ncv, nb;
    const int32_t *flip;              // rows - 1
    const int64_t *basis;             // rows - 1 (== cols for an artificial row)
    const int32_t *kind;              // per variable: 0 positive, 1 negative, 2 signed
    const int64_t *vcol;
    const double  *voff;
};
struct BBNodeRows {
    const int64_t *var;               // (node, k) at node * d + k, newest row first
    const int32_t *sense;             // 0 `<=`, 1 `>=`
    const double  *bound;
    int64_t        d, first;
};
// every node of mt (and of at, a view whose M is NULL is left out): tableau and basis; scratch: m int32 per node
void launch_node_assemble(const TabView &mt, const TabView &at, const BBBaseView &b, const BBNodeRows &nr,
                          int32_t *scratch, hipStream_t s);
// synthetic LP straight into HBM
void launch_synth_fill(const TabView &t, int64_t n_vars, int64_t n_cons, uint64_t seed,
                       const uint64_t *dev_seeds, int64_t col_begin, int64_t col_end, hipStream_t s);

// The resident solve (tableaux whose stored part fits the register files: DESIGN.md): the strip
// layout of a compact view, the exchange buffer it needs (per handle; zero it once), and ONE launch
// that runs up to `cap` pivots of n-solve-tableau per LP with the tableau on chip.  epoch_base must
// grow by at least cap + 2 from launch to launch on the same buffer.
struct ResidentPlan { int TR, CW, G; int64_t slot_granules, lp_granules; };
struct ResidentArgs {
    double sgn, price_tol, ratio_thr;
    unsigned long long *xbuf;
    int64_t xs_lp, xs_slot;
    int G, cap;
    unsigned epoch_base, spins_first, spins;
    int fault;
};
bool   resident_plan(const TabView &compact, ResidentPlan *p);
size_t resident_xbuf_bytes(const TabView &compact);
bool   launch_resident(const TabView &compact, unsigned long long *xbuf, int is_max, double fp_factor,
                       int cap, unsigned epoch_base, hipStream_t s);
void   set_resident_fault(int on);      // test hook: the last workgroup of every LP never publishes
void   set_resident_lds(int mode);      // tuning hook: 1 = part of the strip in LDS (three workgroups per CU), 0 = never
void   set_resident_poll(int mode);     // tuning hook: who polls the exchange records (0 by size, 1 wave 0, 2 every wave)

// Exact (fraction-free, Bareiss) tableaux: kernels_exact.inc, capi_exact.inc.  The tableau is an
// integer matrix T and one positive integer D with t_ij = T_ij / D (objective row included),
// stored as int64_t (bits 64), __int128 (bits 128) or X256 (bits 256: four 64-bit limbs, xwide.h; the
// single tableau only, and only on a handle that allows it).  Every stored value stays inside the
// symmetric range (-2^(W-1), 2^(W-1)), so products and their differences never overflow the
// double-width intermediates.
constexpr int32_t kXOverflow = 110;    // a value left the width in use: restart wider or MI_EXACT_OVERFLOW
constexpr int32_t kXInexact  = 111;    // a Bareiss division left a remainder: a bug (MI_EXACT_INEXACT)
constexpr int     kXThreads  = 256;    // workgroup size of every exact kernel that prices, tests ratios or snapshots
// the pivot being applied (x_record): in XCtl for the single tableau, in LDS for a batch member
struct XPivot {
    int64_t  ec, cr;      // the pivot
    int32_t  sgn, shift;  // its sign; trailing zero bits of dold
    __int128 pa;          // |pivot|
    __int128 dold;        // D before the pivot
    __int128 inv;         // inverse of the odd part of dold modulo 2^W
};
// the 256-bit storage type, its products, and the unsigned twin the inverses live in
typedef XWide<4>  X256;
typedef XWide<8>  X512;
typedef XUWide<4> XU256;
// XPivot's twin at 256 bits.  XPivot itself is also the record a batch member keeps in LDS, and the batches
// stay at 64 / 128 bits: it keeps its layout, and the single tableau's control block carries this one beside it.
struct XPivotW {
    int64_t  ec, cr;
    int32_t  sgn, shift;
    X256     pa, dold, inv;
};
struct XCtl {
    int32_t  status;      // kRunning, or MI_OPTIMAL / MI_UNBOUNDED / MI_MAX_PIVOTS / kXOverflow / kXInexact
    int32_t  err;         // 0, or kXOverflow / kXInexact raised by an update (the larger one wins)
    int32_t  apply;       // the last select / force chose a pivot for the update that follows it
    int32_t  stall;       // the stall flag of rule 2: the last pivot k_x_select chose was degenerate (rhs 0)
    int64_t  n_pivots;    // pivots chosen by k_x_select since the tableau's start (cumulative)
    int64_t  cap_at;      // k_x_select stops with MI_MAX_PIVOTS once n_pivots reaches it (0: no cap)
    int64_t  trace_n;     // pivots recorded (trace buffers hold the first trace_cap)
    __int128 D;           // the common denominator, > 0
    XPivot   piv;         // that pivot (device only)
    X256     Dw;          // bits == 256: the common denominator (D is unused then) ...
    XPivotW  pivw;        // ... and the pivot
};
struct XView {
    void    *T;           // rows x cols, row-major, no padding
    void    *col;         // rows: sgn * T[i][ec] before the pivot
    void    *prow;        // cols: T[cr][j] before the pivot
    int64_t *basis;       // rows - 1
    XCtl    *ctl;
    int64_t *trace_ec, *trace_cr;
    int64_t  rows, cols, trace_cap;
    int      bits;        // 64, 128 or 256
    int      rule;        // MI_RULE_*: how k_x_select prices and breaks ratio ties
};
void launch_x_select(const XView &v, int is_max, hipStream_t s);
void launch_x_force(const XView &v, int64_t ec, int64_t cr, hipStream_t s);
void launch_x_update(const XView &v, hipStream_t s);
// main[r][j] = lc * art[r][src(j)] (r < m); main[m][j] = D_art * cl[j] - sum_r w[r] * art[r][src(j)];
// main D = lc * D_art.  w (m) and cl (main cols) hold values of the handles' width (device memory), lc points
// at one such value on the host.
void launch_x_handover(const XView &art, const XView &mt, const void *w, const void *cl, const void *lc, hipStream_t s);
// Batches of exact tableaux of one shape, one workgroup per member (kernels_exact_batch.inc,
// capi_exact_batch.inc).  One XbView per width of a handle: member q's tableau at T + q * rows * cols,
// its basis at basis + q * (rows - 1), its trace at trace_* + q * trace_cap, its hand-over multipliers
// (main batches) at aux + q * (cols + 1).  A workgroup whose member is not kRunning does nothing.
constexpr int32_t kXbIdle = 112;       // a slot no member runs in (another width, declined, not yet handed over)
constexpr size_t  kXbSnapshotLimit = 48 * 1024;   // LDS bytes of the two snapshots at 128 bits a shape may need
struct XbCtl {
    int32_t  status;      // kRunning, kXbIdle, or MI_OPTIMAL / MI_UNBOUNDED / MI_MAX_PIVOTS / kXOverflow / kXInexact
    int32_t  tp;          // artificial member: 0 phase 1, 1 handed over (phase 2 on the main member), 2 ended between
    int32_t  tp_status;   // tp == 2: MI_INFEASIBLE / MI_ART_NONZERO / MI_ART_STUCK
    int32_t  stall;       // the stall flag of rule 2: the last pivot k_xb_solve chose was degenerate (rhs 0)
    int64_t  n_pivots;    // pivots chosen by k_xb_solve since the member's start (cumulative)
    int64_t  cap_at;      // k_xb_solve stops with MI_MAX_PIVOTS once n_pivots reaches it (0: no cap); on an
                          // artificial member of a two-phase job: the target of both phases and the drive-outs
    int64_t  trace_n;     // pivots recorded (the member's trace buffers hold the first trace_cap)
    int64_t  driveouts;   // forced pivots of k_xb_between
    __int128 D;           // the common denominator, > 0
};
struct XbView {
    void       *T;
    int64_t    *basis;
    XbCtl      *ctl;
    int64_t    *trace_ec, *trace_cr;
    const void *aux;
    int64_t     n, rows, cols, trace_cap;
    int         bits;     // 64 or 128
    int         rule;     // MI_RULE_*: how k_xb_solve prices and breaks ratio ties
};
// at most launch_cap pivots per member (a bounded launch: mi355x_xbatch_cancel)
void launch_xb_solve(const XbView &v, int is_max, int64_t launch_cap, hipStream_t s);
void launch_xb_between(const XbView &art, const XbView &mt, hipStream_t s);
// Exact branch-and-bound (kernels_exact_bb.inc, capi_exact_bb.inc): the base problem's general-form tableau
// at integer scale Db, and the node rows of the members of a batch.
struct XbbBaseView {
    const void    *B;                 // rows x cols values of the width, tight: Db * (base entry)
    const void    *voff;              // per variable, of the width: Db * offset
    int64_t        rows, cols, ncv, nb;
    const int64_t *basis;             // rows - 1; an entry == cols: an artificial row
    const int32_t *kind;              // per variable: 0 positive, 1 negative, 2 signed
    const int64_t *vcol;
    __int128       Db;                // > 0, fits the width
};
struct XbbNodeRows {
    const int64_t *var;               // (member, k) at member * d + k, newest row first
    const int32_t *sense;             // 0 `<=`, 1 `>=`
    const int64_t *bound;
    int64_t        d;
};
// members q0 .. q0 + count - 1 into their slots of mt and / or at (a view whose T is NULL is left out)
void launch_xbb_assemble(const XbView &mt, const XbView &at, const XbbBaseView &b, const XbbNodeRows &nr, int64_t q0,
                         int64_t count, hipStream_t s);
// every member whose width[q] is the view's: D, right-hand sides, objective row (limb pairs) and basis
void launch_xbb_readback(const XbView &v, const int32_t *width, int64_t *values, int64_t *basis, hipStream_t s);
// Exact batches built from problem rows (kernels_exact_lps.inc, capi_exact_lps.inc): the members of a group in
// column space, reduced fractions, member q's (m + 1) x (ncv + 1) entries at q * (m + 1) * (ncv + 1).
struct XbLpsView {
    const int64_t *num, *den;         // rows 0 .. m-1: ncv coefficients and the right-hand side; row m: the objective row
    const int32_t *sense;             // (member, row) at member * m + row: 0 `<=`, 1 `>=`, 2 `=`
    int64_t        m, ncv, n_slack, n_art;   // n_slack rows are not `=`; n_art rows end up `>=` or `=` (every member)
};
// members q0 .. q0 + count - 1 into their slots of mt and / or at (a view whose T is NULL is left out): tableau,
// basis and D; status kXOverflow for a tableau that does not fit the view's width
void launch_xb_assemble_lps(const XbView &mt, const XbView &at, const XbLpsView &sp, int64_t q0, int64_t count, hipStream_t s);
size_t xb_assemble_lps_lds(int64_t m);                                      // its dynamic LDS in bytes
// Double-precision batches built from problem rows (kernels_batch_lps.inc, capi_batch_lps.inc): the members of a
// group in column space, member q's (m + 1) x (ncv + 1) doubles at q * (m + 1) * (ncv + 1).
struct BatchLpsView {
    const double  *L;                 // rows 0 .. m-1: ncv coefficients and the right-hand side; row m: the objective row
    const int32_t *sense;             // (member, row) at member * m + row: 0 `<=`, 1 `>=`, 2 `=`
    int64_t        m, ncv, n_slack, n_art;   // n_slack rows are not `=`; n_art rows end up `>=` or `=` (every member)
};
// every member of mt (and of at, a view whose M is NULL is left out): tableau and basis; scratch: 3 * m int32 per member
void launch_batch_lps_assemble(const TabView &mt, const TabView &at, const BatchLpsView &sp, int32_t *scratch, hipStream_t s);
// per member of a dense batch: last row (cols), last column (rows), basis (rows - 1), each plane member-major (device pointers)
void launch_batch_readback(const TabView &t, double *last_rows, double *last_cols, int64_t *bases, hipStream_t s);
#ifdef MI355X_TEST_HOOKS
// test build: one arithmetic primitive of kernels_exact.inc applied element-wise (k_x_arith_probe; the
// opcodes and the limb layout are mi355x_test_xarith's, include/mi355x_simplex_tune.h).  Device pointers.
enum XProbeOp { kXProbeMul64 = 0, kXProbeMul128, kXProbeAdd256, kXProbeSub256, kXProbeNeg256, kXProbeLt256,
                kXProbeSubOvf64, kXProbeSubOvf128, kXProbeFit64, kXProbeFit128, kXProbeDiv64, kXProbeDiv128,
                kXProbeRem, kXProbeInv64, kXProbeInv128, kXProbeCtz, kXProbeInv256, kXProbeCtz256, kXProbeOps };
void launch_x_arith_probe(int op, int64_t n, const int64_t *a, const int64_t *b, int64_t *out, int32_t *rc, hipStream_t s);
// the same for the 256-bit width's primitives with 512-bit operands or results: elements of eight limbs
// (k_x_arith_probe8, mi355x_test_xarith8)
enum XProbe8Op { kXProbe8Mul256 = 0, kXProbe8Add512, kXProbe8Sub512, kXProbe8Neg512, kXProbe8Lt512, kXProbe8Eq512,
                 kXProbe8SubOvf256, kXProbe8Fit256, kXProbe8Div256, kXProbe8Rem256, kXProbe8Ops };
void launch_x_arith_probe8(int op, int64_t n, const int64_t *a, const int64_t *b, int64_t *out, int32_t *rc, hipStream_t s);
#endif

// Single-float tableaux (kernels_single.inc, capi_single.inc): the reference's single-float path in IEEE binary32.
// Common Lisp SINGLE-FLOAT-EPSILON = 2^-24 (1 + 2^-23)  (src/utils.lisp:84-124)
constexpr float kClEpsilonSingle = 0x1.000002p-24f;
// One tableau of floats in HBM.  Row-major, leading dimension ld a multiple of 32 floats (128-byte row starts);
// columns [cols, ld) are padding (zero in the pivot row).  The control block is the double path's Ctl.
struct SView {
    float   *M;
    int64_t  ld, rows, cols;
    int64_t *basis;       // rows-1 entries
    float   *col;         // snapshot of the entering column before the pivot, rows entries
    float   *prow;        // normalised pivot row, ld entries (padding zero)
    Ctl     *ctl;
    int64_t *trace_ec, *trace_cr;
    int64_t  trace_cap;
};
struct SingleThresholds { float price, ratio, feasible; };    // (f/8) eps, 0 + (f/2) eps, f eps: float arithmetic
SingleThresholds single_thresholds(double fp_factor);
struct SingleUpdateShape { int strips, strip_quads, tr, row_chunks; };
SingleUpdateShape single_update_shape(const SView &t);
// the LDS-resident solve: the ONE budget (dynamic LDS bytes: stored tableau + pivot row + column snapshot; the
// reductions' scratch is static and comes on top, inside the CU's 160 KiB), and the pivots one launch may make
constexpr size_t kSingleLdsBudget = 156 * 1024;
constexpr int    kSingleLaunchCap = 4096;
size_t single_lds_bytes(const SView &t);
bool   single_lds_available(const SView &t);   // fits the budget AND the kernel's dynamic-LDS attribute could be raised
void launch_s_ctl_reset(const SView &t, int64_t max_pivots, int reset_trace, hipStream_t s);
void launch_s_select(const SView &t, int is_max, double fp_factor, hipStream_t s);
void launch_s_update(const SView &t, hipStream_t s);
void launch_s_price_only(const SView &t, int is_max, double fp_factor, hipStream_t s);
void launch_s_ratio_only(const SView &t, int64_t ec, double fp_factor, hipStream_t s);
void launch_s_prepare_pivot(const SView &t, int64_t ec, int64_t cr, hipStream_t s);
void launch_s_solve(const SView &t, int is_max, double fp_factor, int cap, hipStream_t s);
void launch_s_handover_copy(const SView &art, const SView &mt, hipStream_t s);

// Batches of single-float tableaux of one shape (kernels_single_batch.inc, capi_single_batch.inc): one workgroup owns
// one member for its whole solve (s_solve_in_lds, the loop of k_s_solve).  Member q: tableau at M + q * stride (stride
// = rows * ld floats, a multiple of 32), basis at basis + q * max(rows - 1, 1) (a member of one row has no basis entry: nothing reads one there),
// control block ctl + q, trace at trace_ec / trace_cr + q * trace_cap.
struct SbView {
    float   *M;
    int64_t  stride, ld, rows, cols, n_lps;
    int64_t *basis;
    Ctl     *ctl;
    int64_t *trace_ec, *trace_cr;
    int64_t  trace_cap;
};
// stored quads (rows x ceil(cols / 4)) up to which a member takes 256 threads.  Measured (profiles/sbatch_rate.txt, part 2):
// at 1024 members 256 threads beat 1024 at every shape the LDS budget holds, 3.7 x at 425 quads, 1.15 x at 9700 -- no
// crossover inside the budget, so the threshold is the budget itself and 1024 threads are the tuning hook's.
constexpr int64_t kSbatchQuads1024 = (int64_t)(kSingleLdsBudget / 16);
int    sbatch_threads_for(int64_t rows, int64_t cols);
size_t sbatch_lds_bytes(const SbView &b);
bool   sbatch_available(const SbView &b, int threads, int *members_per_cu);   // fits the budget AND the attributes could be raised
void launch_sb_ctl_reset(const SbView &b, hipStream_t s);                  // every member: kRunning, no pivots, an empty trace
void launch_sb_begin(const SbView &b, int64_t max_pivots, const int32_t *phase, int want_phase, hipStream_t s);
void launch_sb_solve(const SbView &b, int threads, int is_max, double fp_factor, int cap, const int32_t *gate, hipStream_t s);
void launch_sb_between(const SbView &art, const SbView &main_b, int threads, int32_t *phase, double fp_factor,
                       int64_t max_pivots, hipStream_t s);
// Every kernel of the family is ONE template over the batch's view (SbView, SrView below); the launchers are overloads
// on the view.
// RAGGED batches of single-float tableaux (kernels_single_batch.inc over an SrView, capi_single_ragged.inc): every member its own
// shape and sense, one workgroup per member, the loop and the step between the phases those of the batch of one shape
// (src/simplex.lisp:402-461).  Member q: tableau at M + m_off floats (rows x ld, ld = cols rounded up to 32 floats, so
// every m_off is a multiple of 32 and the 16-byte quad loads of s_solve_in_lds stay aligned), basis at basis +
// basis_off, control block ctl + q, trace at trace_ec / trace_cr + q * trace_cap; sgn: +1 max, -1 min.
struct SrMember { int64_t m_off, basis_off, ld, rows, cols; float sgn; };
struct SrView {
    float          *M;
    int64_t        *basis;
    Ctl            *ctl;
    int64_t        *trace_ec, *trace_cr;
    int64_t         trace_cap, n_lps;
    const SrMember *members;              // n_lps descriptors (device)
};
// A batch of one shape is a ragged batch whose descriptors can be computed: member q of b (sgn: the call says it).
// The kernels and the host (capi_single_batch.inc: sb_host_member) ask this ONE function.
XW_HD inline SrMember sb_descriptor(const SbView &b, int64_t q)
{
    return SrMember{q * b.stride, q * (b.rows > 1 ? b.rows - 1 : 1), b.ld, b.rows, b.cols, 0.0f};
}
bool   sragged_raise(int threads);                                           // the two kernels' dynamic-LDS attribute
bool   sragged_occupancy(int threads, size_t lds, int *members_per_cu);      // the ragged solve kernel's residency at this LDS size
// one occupancy class: `count` member indices at `members` (device; nullptr: members 0 .. count - 1), lds: the
// class's largest member's bytes
void launch_sb_solve(const SrView &b, const int32_t *members, int64_t count, size_t lds, int threads, double fp_factor,
                     int cap, const int32_t *gate, hipStream_t s);
void launch_sb_between(const SrView &art, const SrView &main_b, const int32_t *members, int64_t count, size_t lds,
                       int threads, int32_t *phase, double fp_factor, int64_t max_pivots, hipStream_t s);
// The global form of a single-float batch (kernels_single_global.inc): one workgroup per member, the tableau in HBM,
// pivot row and column snapshot in LDS -- for members beyond the LDS budget.
size_t sgbatch_lds_bytes(const SbView &b);                                  // k_sg_solve's dynamic LDS
size_t sgbatch_between_lds_bytes(const SbView &art);                        // k_sb_between's, for a global-form pair
constexpr int64_t kSgbatchBytes1024 = 256 * 1024;                           // stored bytes from which a member takes 1024 threads
int    sgbatch_threads_for(int64_t rows, int64_t ld);
int    sgbatch_launch_cap_for(int64_t rows, int64_t ld);
bool   sgbatch_available(const SbView &b, int threads, int *members_per_cu);  // fits the budget AND the attributes could be raised
void launch_sg_solve(const SbView &b, int threads, int is_max, double fp_factor, int cap, const int32_t *gate, hipStream_t s);
void launch_sg_between(const SbView &art, const SbView &main_b, int threads, int32_t *phase, double fp_factor,
                       int64_t max_pivots, hipStream_t s);
// Single-float branch-and-bound (kernels_single_bb.inc, capi_single_bb.inc): the base problem's general-form
// tableau in floats; the node rows of the members are an XbbNodeRows, as for the exact search.
struct SbbBaseView {
    const float   *B;                 // rows x cols floats, tight
    const float   *voff;              // per variable: its offset (not read for a free variable)
    int64_t        rows, cols, ncv, nb;
    const int64_t *basis;             // rows - 1; an entry == cols: an artificial row
    const int32_t *kind;              // per variable: 0 positive, 1 negative, 2 signed
    const int64_t *vcol;
};
size_t sbb_assemble_lds(int64_t m, int64_t d);                              // its dynamic LDS in bytes (m constraint rows)
// every member of mt and of at (at.M == nullptr: no artificial rows): tableau over the whole leading dimension, basis
void launch_sbb_assemble(const SbView &mt, const SbView &at, const SbbBaseView &b, const XbbNodeRows &nr, hipStream_t s);
// per member: last column (rows), last row (cols), basis (rows - 1), each plane member-major (device pointers)
void launch_sb_readback(const SbView &b, float *rhs, float *obj, int64_t *basis, hipStream_t s);
// Single-float batches from problem rows (kernels_single_lps.inc, capi_single_lps.inc): the members in column space,
// in floats (device pointers) -- per member (m + 1) x (ncv + 1) rows, then m senses (0 `<=`, 1 `>=`, 2 `=`)
struct SlpView {
    const float   *L;
    const int32_t *sense;
    int64_t        m, ncv, n_slack, n_art;
};
constexpr int kSlpMaxRows = 256;                                            // k_slp_assemble: one row per thread, one trip
// every member of mt and of at (at.M == nullptr: no artificial rows): tableau over the whole leading dimension, basis
void launch_slp_assemble(const SbView &mt, const SbView &at, const SlpView &sp, hipStream_t s);
// RAGGED batches built on the device (capi_single_ragged_build.inc): the two assemblies above with a shape per member
// (the same kernel templates over SrView and the sources below), and the light read-back of a ragged batch.
// From rows: L and sense tight and concatenated, member q's (m + 1) x (ncv + 1) floats at L + l_off, its m senses at
// sense + s_off; n_slack of its rows are not `=`, n_art end up `>=` or `=`.  m <= kSlpMaxRows.
struct SrlpMember { int64_t l_off, s_off; int32_t m, ncv, n_slack, n_art; };
struct SrlpView { const float *L; const int32_t *sense; const SrlpMember *members; };
// From nodes: node q's d rows (newest first) at off in the concatenated var / sense / bound arrays.
struct SrbbNode { int64_t off; int32_t d; };
struct SrbbNodeRows { const int64_t *var; const int32_t *sense; const int64_t *bound; const SrbbNode *nodes; };
// every member of mt and of at (at.M == nullptr: no member has artificial rows); all pointers are device pointers
void launch_slp_assemble(const SrView &mt, const SrView &at, const SrlpView &sp, hipStream_t s);
// lds: sbb_assemble_lds of the largest member of the launch
void launch_sbb_assemble(const SrView &mt, const SrView &at, const SbbBaseView &b, const SrbbNodeRows &nr, size_t lds, hipStream_t s);
// per member: last column, last row, basis, into three concatenated planes at the running sums of rows, cols (col_off,
// device, n_lps entries) and rows - 1
void launch_sb_readback(const SrView &b, const int64_t *col_off, float *rhs, float *obj, int64_t *basis, hipStream_t s);
// The same two assemblies spread over a grid, for GLOBAL-form batches (kernels_single_assemble_global.inc): a row pass
// into per-member scratch planes (device memory of sga_*_scratch_bytes, the caller's, alive until the stream has run
// the launches), one write pass and the artificial objective row, ordered by the stream alone.  Any m, any depth.
size_t sga_lps_scratch_bytes(int64_t n_lps, int64_t m);
size_t sga_nodes_scratch_bytes(int64_t n_nodes, int64_t m);                 // m: the node's constraint rows
// (ev, measurement aid, may be nullptr: four events recorded in front of the row pass and behind each of the passes)
void launch_sga_lps(const SbView &mt, const SbView &at, const SlpView &sp, int32_t *scratch, hipStream_t s,
                    hipEvent_t *ev = nullptr);
void launch_sga_nodes(const SbView &mt, const SbView &at, const SbbBaseView &b, const XbbNodeRows &nr, int32_t *scratch,
                      hipStream_t s);

int         update_variant_count();
const char *update_variant_name(int v);
void        set_update_variant(int v);      // tuning hook (bench / microbench only)
int         get_update_variant();
const char *update_kernel_symbol();

}  // namespace mi355x
