/* mi355x_simplex_tune.h -- tuning, measurement and test hooks of libmi355x_simplex.so.
 *
 * NOT part of the drop-in boundary (that is mi355x_simplex.h, every entry of which restates a
 * function of the reference): nothing here corresponds to anything in
 * neil-lindquist/linear-programming.  bench.py, tools/ and tests/ use these to pick between
 * implementations of the same bit-identical path and to read back measurement data.
 *
 * State model.  The knobs that choose WHICH implementation of the solve loop runs (select mode,
 * compact, block, look-ahead mode, tail policy, hand-over mode, batch mode, batch block, resident,
 * column-partition exchange) are SNAPSHOTTED INTO A HANDLE WHEN IT IS CREATED: set them, then create
 * the handle that should run that way; a handle never changes path because another thread turned
 * a knob, so the per-handle thread-safety promise of mi355x_simplex.h holds whatever other threads
 * do with these hooks.  The remaining hooks (update-kernel tiling, sweep shape / implementation,
 * shard look-ahead split, one-XCD placement, poll bounds, resident poll mode) are
 * process-wide and read at every launch: measurement and test use only, change them while no other
 * thread is inside the library.  Every hook returns the value now in effect.
 */
#ifndef MI355X_SIMPLEX_TUNE_H
#define MI355X_SIMPLEX_TUNE_H

#include "mi355x_simplex.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the per-pivot update kernel (k_update): compiled tilings ------------------------- */
int         mi355x_tune_variant_count(void);
const char *mi355x_tune_variant_name(int variant);
int         mi355x_tune_set_variant(int variant);            /* 0 = default (by size)           */
int         mi355x_tune_set_alternate_sweep(int on);         /* odd launches sweep bottom-up     */
int         mi355x_tune_set_ld_extra(int doubles);           /* extra row padding, multiple of 16 */

/* ---- which implementation of the solve loop runs -------------------------------------- */
int         mi355x_tune_set_select_mode(int mode);           /* 0 auto, 1 one workgroup, 2 split */
int         mi355x_tune_set_compact(int on);                 /* 1: [non-basic | RHS] (default)   */
int         mi355x_tune_set_block(int k);                    /* pivots per sweep: 0 by size (default: 16,
                                                                or a wide block of 28 where the sweep
                                                                dominates), 1 off, 2 .. 16, 24, 28    */
int         mi355x_tune_set_lookahead_mode(int mode);        /* 0 auto, 1 two launches per step,
                                                                2 one persistent launch per block
                                                                (tableaux of up to 64 look-ahead
                                                                workgroups = 16384 rows and 32768
                                                                stored columns; auto: of those with more
                                                                than 32, the ones below 2e9 bytes stored) */
int         mi355x_tune_set_sweep_shape(int rows_per_workgroup, int nontemporal /* -1 by size */);
int         mi355x_tune_set_sweep_impl(int impl);            /* 0 k_sweep16 for full blocks, 1 k_sweep
                                                                always, 3 the two-launch form of the wide
                                                                sweeps (k_sweepw<16> + k_sweepw_rest);
                                                                4 / 8: rows per step of k_sweep16      */
int         mi355x_tune_set_sweepw_ring(int on);             /* wide sweeps (k > 16 pivots per pass): 1
                                                                (default) the tile's rows travel through a
                                                                per-wave LDS ring (k_sweepw_ring), 0 the
                                                                register form of round 4 (k_sweepw); A/B of
                                                                the ring's cache policy: 2 no non-temporal
                                                                access, 3 non-temporal stores only        */
int         mi355x_tune_set_prime(int on);                   /* 1 (default): a handle's first block is
                                                                preceded by one EMPTY block of every kernel
                                                                form its requests can pick, so that no later
                                                                request pays a kernel's first launch; 0 off */
int         mi355x_tune_set_sweep_xcd_map(int on);           /* k_sweepw_ring: 1 the (strip, tile) pairs in
                                                                strip-major order cut into one run per XCD
                                                                (traffic 1.06 x instead of 1.14 x, 1.5 %
                                                                slower), 0 (default) the grid's own order */
int         mi355x_tune_set_sweep_skew(int rows);            /* k_sweepw_ring where ONE round of workgroups (three
                                                                per CU) covers the tableau: the thirds of the
                                                                tiles in dispatch order are tr + rows / tr /
                                                                tr - rows tall -- a SIMD serves its oldest wave
                                                                first.  -1 (default): 5/16 of the tile height
                                                                (config 3: 28 of 92, 108.5 -> 102.5 us per
                                                                pass); 0: equal tiles */
int         mi355x_tune_set_ctl_wait(int mode);              /* how a status read-back waits: 2 (default) a
                                                                kernel publishes the control block to pinned
                                                                memory and the host polls its sequence number,
                                                                1 copy + polled hipStreamQuery, 0 copy +
                                                                hipStreamSynchronize                      */
int         mi355x_tune_set_shard_la_split(int mode);        /* column shards, local look-ahead step:
                                                                0 by size, 1 one workgroup, 2 many */
int         mi355x_tune_set_colpart_exchange(int mode);      /* column partition over RCCL, how the
                                                                entering column travels (read when a
                                                                handle is created): 0 int64 SUM
                                                                all-reduce of owner's bits + zeros
                                                                (no host sync), 1 ncclBroadcast from
                                                                the owner (root read back from the
                                                                all-gather: one host sync per pivot),
                                                                2 no collective at all: the shards
                                                                write pricing pairs and the entering
                                                                column straight into each other's
                                                                fine-grained buffers (P2P / IPC over
                                                                xGMI), self-validating granules; a
                                                                shard that has its device to itself
                                                                steps in two launches, 3 the same
                                                                with the four launches per step of
                                                                shards that share a stream         */
/* one process per GPU in exchange mode 2: the ranks' exchange buffers are mapped into each other's
 * address space through IPC handles.  With a communicator (an id from mi355x_rccl_unique_id) the
 * library all-gathers the handles itself when the handle is created; with id128 == NULL no
 * communicator exists at all (RCCL is not touched) and the host connects the ranks: every rank
 * takes its 64-byte handle, the host gathers them in rank order (world x 64 bytes) and hands the
 * table to every rank before the first solve. */
int         mi355x_colpart_p2p_handle(mi355x_colpart *p, void *handle64);
int         mi355x_colpart_p2p_connect(mi355x_colpart *p, const void *handles);
int         mi355x_tune_set_tail_policy(int p);              /* n pivots, n not a multiple of the block:
                                                                0 spread evenly, 1 full blocks + remainder */
int         mi355x_tune_set_handover_mode(int mode);         /* 0 auto, 1 sequential re-elimination */
int         mi355x_tune_set_batch_mode(int mode);            /* 0 auto, 1 lockstep, 2 all in one workgroup
                                                                per LP, 3 look-ahead per LP + sweeps over all LPs */
int         mi355x_tune_set_batch_block(int k);              /* blocked per-LP kernel, 1 = off   */
int         mi355x_tune_set_resident(int mode);              /* resident solve (the stored tableau in
                                                                registers, one exchange per pivot):
                                                                0 auto = whenever the shape fits AND
                                                                every knob above is at its default,
                                                                1 never, 2 whenever the shape fits  */
int         mi355x_tune_set_resident_poll(int mode);         /* who polls the exchange records:
                                                                0 by size (every wave when an LP has
                                                                <= 8 workgroups), 1 wave 0, 2 every */
int         mi355x_tune_set_resident_lds(int mode);          /* 1: 24 of a strip's 64 columns in LDS (three
                                                                workgroups per CU; shapes of <= 256
                                                                constraints) -- measured NOT faster, see
                                                                kernels_launch.inc; 0 (default): never */
/* 1 when the solve entry points would run this handle (in its current representation) resident */
int         mi355x_tab_resident(mi355x_tab *t);

/* ---- persistent look-ahead (k_la_block) ------------------------------------------------ */
int         mi355x_tune_set_la_one_xcd(int on);              /* 1 (default): all its workgroups on
                                                                one XCD, verified inside the launch
                                                                (up to 32 workgroups; more are spread
                                                                over the chip whatever this says)   */
int         mi355x_tune_set_la_max_spins(unsigned polls);    /* polls before a workgroup gives up
                                                                on a record; 0 = default (2^21)  */
/* How often an exchange of the persistent look-ahead was lost on this handle (0 = never).  After a
 * loss the solve carries on on the two-launch look-ahead; the persistent form is re-armed after 1024
 * clean blocks (four times as many after each further loss).  mi355x_debug_set_la_rearm overrides the
 * number of clean blocks left (tests). */
int         mi355x_tab_la_lost(const mi355x_tab *t);
/* Workgroups of this handle's last persistent look-ahead launch (0: none so far): a thread per constraint
 * row and per pair of non-RHS columns. */
int         mi355x_tab_la_workgroups(const mi355x_tab *t);
int         mi355x_debug_set_la_rearm(mi355x_tab *t, int64_t blocks);
/* Which implementation the dispatcher actually enqueued on this handle so far, launches by class:
 * out8[0] per-pivot updates (k_update), [1] persistent look-ahead blocks (k_la_block), [2] two-launch
 * look-ahead blocks (k_la_gather / k_la_scale per step), [3] k_sweep16 sweeps, [4] wide sweeps
 * (k_sweepw + k_sweepw_rest), [5] short sweeps (k_sweep), [6] resident launches (k_resident),
 * [7] split selects (k_select_gather + k_select_scale). */
int         mi355x_tab_path_counts(const mi355x_tab *t, int64_t *out8);

/* ---- measurement ------------------------------------------------------------------------ */
/* HIP-event brackets on the handle's stream (what `mi355x_tab_timing_*` of the main header
 * brackets is the tableau update / sweep; `which` selects another kernel class):
 * 0 update / sweep, 1 look-ahead (select) */
int         mi355x_tab_timing_read_kind(mi355x_tab *t, int which, int64_t *n_launches,
                                        double *sum_ms, double *min_ms);
/* column partition over RCCL: HIP-event brackets around the two per-pivot collectives of every
 * `stride`-th pivot (at most max_samples per shard and per solve call; 0 = off); _read waits for
 * the shards' streams and returns the averages over this process's shards since the last read */
int         mi355x_colpart_block_size(const mi355x_colpart *p);   /* pivots per sweep of a shard's slice */
/* exchange mode 2, blocked shards: the look-ahead of a whole block as ONE persistent launch per device
 * (k_shard_la_block).  out4: [0] blocks enqueued that way, [1] exchanges it lost, [2] the handle is demoted
 * to the two-launch step right now, [3] the next block would take the persistent form */
int         mi355x_colpart_la_stats(mi355x_colpart *p, int64_t *out4);
int         mi355x_colpart_is_compact(const mi355x_colpart *p);   /* 1 compact shards, 0 dense shards */
int         mi355x_colpart_debug_set_la_rearm(mi355x_colpart *p, int64_t blocks);   /* as mi355x_debug_set_la_rearm */
int         mi355x_colpart_debug_rhs(mi355x_colpart *p, int shard, double *out, int64_t n, int clear);   /* mi355x_debug_rhs of a local shard */
int         mi355x_tune_set_shard_la_block(int mode);        /* read when a handle is created: 0 (default) the
                                                                persistent block launch wherever it fits, 1 never */
int         mi355x_tune_set_shard_self_hop(int on);          /* measurement: a LONE shard runs exchange A (its
                                                                pricing pair) against its own buffer -- what a
                                                                shard of several pays minus the wire        */
int         mi355x_tune_set_p2p_spins(unsigned n);           /* polls before a shard gives a peer's granules
                                                                up (read at creation; 0 = default 2^24)      */
int         mi355x_colpart_exchange_timing_enable(mi355x_colpart *p, int stride, int max_samples);
int         mi355x_colpart_exchange_timing_read(mi355x_colpart *p, int64_t *n_samples,
                                                double *allgather_us, double *allreduce_us);
/* measurement aid: launches the sweep of the handle's CURRENT pending list n more times (a sweep
 * does not consume the list) and returns the average launch duration (HIP events).  The tableau
 * is meaningless afterwards. */
int         mi355x_debug_repeat_sweep(mi355x_tab *t, int n, double *avg_us);
/* debugging aid: copies n doubles of the handle's scratch `rhs` buffer (the per-phase clocks of
 * a -DMI355X_LA_TIMING build); clear != 0 zeroes it afterwards */
int         mi355x_debug_rhs(mi355x_tab *t, double *out, int64_t n, int clear);
int         mi355x_debug_last_wait(double *out2);            /* host microseconds of the last status read-back:
                                                                [0] launching k_ctl_publish, [1] polling its
                                                                sequence number (bench.py's steady-state leg)   */
/* test aid: member lp_index of a dense batch as it is STORED, padding columns included -- one 2-D copy of
 * rows x ld doubles; *ld (may be NULL) = the leading dimension; out NULL: only *ld.  What a create entry left
 * in the columns [cols, ld) (mi355x_batch_create_lps writes them itself). */
int         mi355x_batch_debug_stored(mi355x_batch *b, int64_t lp_index, double *out, int64_t *ld);
/* Which driver mi355x_batch_solve ran on this batch so far, launches by class (the batch counterpart of
 * mi355x_tab_path_counts): out4[0] resident launches (k_resident, every LP on chip), [1] blocks of the split
 * form (a k_batch_block look-ahead per LP + ONE sweep over all LPs), [2] one-workgroup-per-LP launches
 * (k_batch_block, or k_batch_solve without blocking), [3] lockstep (select, update) launch pairs. */
int         mi355x_batch_path_counts(const mi355x_batch *b, int64_t *out4);
/* measurement aid: enable != 0 brackets the assembly kernels (k_blp_rows, k_assemble, k_art_objective) of
 * every sub-batch mi355x_*batch_create_lps builds from now on with HIP events; every call returns the device
 * milliseconds and the sub-batches counted since the previous call (either may be NULL) and starts over. */
int         mi355x_batch_lps_timing(int enable, double *sum_ms, int64_t *n_sub_batches);

/* ---- branch-and-bound: device assembly of node tableaux (k_bb_rows, k_assemble) ------------------------ */
/* n_nodes nodes of one depth of problem p's search -- node q's rows (var, sense 0 `<=` / 1 `>=`, bound)
 * at [q * depth, (q + 1) * depth), newest first, as mi355x_simplex_solver_bb_trace reports them --
 * assembled on `device` and downloaded: per node the main tableau (rows x cols, tight), its basis
 * (rows - 1) and, art_cols > 0, the artificial tableau (rows x art_cols) and its basis; each bit-identical
 * to mi355x_build_tableau of the node problem.  NULL arrays: only the shapes.  Every node must have the
 * same number of artificial rows (MI_BAD_ARG otherwise). */
int         mi355x_bb_debug_assemble(const mi355x_problem *p, int64_t n_nodes, int64_t depth, const int64_t *var,
                                     const int32_t *sense, const double *bound, int device, int64_t *rows,
                                     int64_t *cols, int64_t *art_cols, double *main_out, int64_t *main_basis,
                                     double *art_out, int64_t *art_basis);

/* ---- fault injection: TEST BUILD ONLY ---------------------------------------------------- */
/* single-float tableaux (mi355x_stab_*): the form handles created from now on take -- 0 auto (LDS when the stored
 * bytes plus scratch fit the budget), 1 always the select / update pair, 2 LDS (still only where it fits) */
int         mi355x_tune_set_single_form(int form);
/* measurement: k_s_update launched `reps` times on one prepared pivot, between two events: *avg_ms per launch,
 * *bytes read + written per launch (rows x ld floats each way); the tableau is not preserved */
int         mi355x_stab_debug_update_time(mi355x_stab *h, int64_t entering_col, int64_t changing_row, int reps,
                                          double *avg_ms, int64_t *bytes);
/* batches of single-float LPs (mi355x_sbatch_*), both snapshotted per handle at create: the workgroup a batch
 * takes -- 0 auto (the shape's rule), 256 or 1024 -- and the pivots per member one launch may make -- 0 the
 * default (4096; global form: 4096 scaled down by stored bytes over the LDS budget, at least 1), else a count.
 * _global_threads: the workgroup of batches made by mi355x_sbatch_create_global -- 0 auto, 256 or 1024 */
int         mi355x_tune_set_sbatch_threads(int threads);
int         mi355x_tune_set_sbatch_launch_cap(int cap);
int         mi355x_tune_set_sbatch_global_threads(int threads);
/* ragged batches (mi355x_sbatch_create_ragged), snapshotted per handle at create: 1 one class for all members -- one
 * launch per round at the largest member's LDS size; 4 up to four occupancy classes (the workgroups resident per
 * compute unit at the member's own LDS size, capped at 4), one launch per class and round, the class of the largest
 * members first; 0 the default, which is one class: a launch per class was measured at half the rate of one launch
 * on 256 members over all four classes, as the stream runs the classes one after the other
 * (profiles/sbatch_ragged_rate.txt, part 4).  (The workgroup and the launch cap are _sbatch_threads' and
 * _sbatch_launch_cap's.) */
int         mi355x_tune_set_sbatch_ragged_classes(int classes);
/* test aid: member lp_index of a single-float batch as it is STORED, padding columns included -- rows x ld floats;
 * *ld (may be NULL) = the leading dimension; out NULL: only *ld.  What a create entry left in the columns
 * [cols, ld) (mi355x_sbatch_create_lps writes them itself). */
int         mi355x_sbatch_debug_stored(mi355x_sbatch *b, int64_t lp_index, float *out, int64_t *ld);
/* measurement aid (tools/slps_global_rate.py): enable != 0 makes every mi355x_sbatch_create_lps_global from now on
 * record HIP events around its three passes; the call also reports the LAST timed create's milliseconds -- row pass,
 * write pass, artificial objective row (0 without artificial rows; -1: not measured).  Any pointer may be NULL. */
int         mi355x_sbatch_lps_global_timing(int enable, double *rows_ms, double *write_ms, double *objective_ms);

/* Compiled in with -DMI355X_TEST_HOOKS (libmi355x_simplex_test.so, built next to the product
 * library by linear-programming_amd/build.py and loaded by the tests that need it); the product
 * library neither exports these nor contains the code paths behind them. */
#ifdef MI355X_TEST_HOOKS
int         mi355x_tune_set_resident_fault(int on);          /* the last workgroup of every LP never
                                                                publishes (co-residency lost)    */
int         mi355x_tune_set_shard_la_fault(int step_plus_1); /* the same two faults (below) in the last
                                                                workgroup of the last local shard of a
                                                                k_shard_la_block launch                  */
int         mi355x_tune_set_la_fault(int step_plus_1);       /* > 0: the last workgroup stops
                                                                publishing from that step on; < 0: it
                                                                publishes its ratio record of step
                                                                -step_plus_1 - 1 and then gives up
                                                                alone (the leader commits a pivot
                                                                that workgroup never stored)     */
/* Arithmetic probe: one primitive of the exact kernels' wide integer arithmetic (kernels_exact.inc, the very
 * functions the solve kernels call) applied to n operand tuples in one launch.  Element i of a, b and out is
 * four little-endian 64-bit limbs at [4 i, 4 i + 4), two's complement; a 64-bit value takes limb 0, a 128-bit
 * value limbs 0 and 1 (unused operand limbs are ignored, unused result limbs are zero).  rc[i] is the
 * primitive's own status, or -1 where an operand breaks the precondition stated below.  op:
 *    0 xmul 64 x 64 -> 128          1 xmul 128 x 128 -> 256
 *    2 s256_add   3 s256_sub   4 s256_neg (a)   5 s256_lt -> out limb 0 (256-bit a, b; wrapping)
 *    6 xsub_ovf: 128-bit a - b      7 xsub_ovf: 256-bit a - b         rc 1: the difference left the width
 *    8 xfit 128 -> 64 (a)           9 xfit 256 -> 128 (a)             rc 1: outside the symmetric range
 *   10 xdiv: 128-bit a / 64-bit b  11 xdiv: 256-bit a / 128-bit b     b > 0; shift and inverse derived from b
 *                                                                     as a pivot record derives them; rc 0,
 *                                                                     110 (quotient too wide) or 111 (remainder)
 *   12 xrem: |256-bit a| mod 128-bit b (0 < b < 2^127)
 *   13 xinv_odd modulo 2^64 (a)    14 xinv_odd modulo 2^128 (a)       a odd
 *   15 xctz of the 128-bit a (non-zero) -> out limb 0
 *   16 xinv_odd modulo 2^256 (a odd, all four limbs)               17 xctz of the 256-bit a (non-zero) -> out limb 0 */
int         mi355x_test_xarith(int op, int64_t n, const int64_t *a, const int64_t *b, int64_t *out,
                               int32_t *rc, int device);
/* The same for the primitives of the 256-bit width (xwide.h) that take or return 512-bit values: element i of a,
 * b and out is EIGHT limbs at [8 i, 8 i + 8); a 256-bit value takes limbs 0 .. 3.  op:
 *    0 xmul 256 x 256 -> 512
 *    1 add   2 xsub   3 negate (a)   4 xlt -> out limb 0   5 xeq -> out limb 0   (512-bit a, b; wrapping)
 *    6 xsub_ovf: 512-bit a - b                                        rc 1: the difference left the width
 *    7 xfit 512 -> 256 (a)                                            rc 1: outside the symmetric range
 *    8 xdiv: 512-bit a / 256-bit b                                    b > 0; rc 0, 110 or 111 as above
 *    9 xrem: |512-bit a| mod 256-bit b (0 < b < 2^255) */
int         mi355x_test_xarith8(int op, int64_t n, const int64_t *a, const int64_t *b, int64_t *out,
                                int32_t *rc, int device);
#endif

#ifdef __cplusplus
}
#endif
#endif
