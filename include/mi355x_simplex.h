/*
 * mi355x_simplex.h -- C ABI of libmi355x_simplex.so
 *
 * MI355X (gfx950) dense-simplex backend for the Common Lisp library
 * neil-lindquist/linear-programming (v2.3.0).  This is the drop-in boundary:
 * the entry points below are what a CFFI binding behind the library's
 * `linear-programming:*solver*` hook (src/solver.lisp:39-56) calls in place of
 * the Lisp loops of src/simplex.lisp.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C, no callbacks, no ownership transfer: the caller owns every host
 *     buffer, the library owns the device memory behind a handle;
 *   - a tableau is the reference's `tableau-matrix` (src/simplex.lisp:48-58):
 *     rows = constraint_count + 1 (last row = objective row),
 *     cols = var_count + 1       (last column = right-hand side),
 *     row-major, tightly packed doubles on the host side;
 *   - every function returns a status (>= 0: outcome, < 0: error);
 *     mi355x_last_error() gives the thread-local message of the last error;
 *   - there is NO CPU fallback: without a gfx950 device every compute entry
 *     point fails with MI_NO_DEVICE;
 *   - a handle may be used from one thread at a time.
 *
 * Arithmetic contract (what makes results bit-identical to the reference's
 * double-float path): IEEE binary64, product and difference rounded separately
 * (no FMA) in the rank-1 update, true division for the pivot-row scaling and
 * the ratio test, tolerances factor/8, factor/2 (and factor for the phase-1
 * feasibility test) times Common Lisp's DOUBLE-FLOAT-EPSILON
 * 1.1102230246251568e-16, strict comparison with lowest index winning ties.
 */
#ifndef MI355X_SIMPLEX_H
#define MI355X_SIMPLEX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355X_SIMPLEX_ABI_VERSION 1

/* outcomes (returned by the solve entry points) */
#define MI_OK            0
#define MI_OPTIMAL       0   /* find-entering-column returned NIL            simplex.lisp:455-456 */
#define MI_UNBOUNDED     1   /* -> unbounded-problem-error                   simplex.lisp:458-459 */
#define MI_INFEASIBLE    2   /* -> infeasible-problem-error                  simplex.lisp:405-407 */
#define MI_MAX_PIVOTS    3   /* pivot cap reached (backend-specific; the reference has no cap) */
#define MI_ART_NONZERO   4   /* "Artificial variable ~S still non-zero"       simplex.lisp:423-424 */
#define MI_ART_STUCK     5   /* "Artificial variable still in basis and ..."  simplex.lisp:432-433 */
#define MI_NONFINITE     6   /* compact column shards only: the entering column holds an inf / NaN;
                                the reference would spread NaNs over basic columns, which are not
                                stored there (single tableaux and batches switch to the dense
                                tableau by themselves and continue) */
#define MI_CANCELLED     7   /* mi355x_*_cancel was called from another thread: the solve stopped between
                                two chunks of launches; whole pivots only, the tableau is consistent and a
                                later solve call carries on from it */
#define MI_RUNNING     100   /* asynchronous use only: the iterations enqueued so far have not
                                terminated the solve (mi355x_tab_sync) */
/* errors */
#define MI_BAD_ARG      -1
#define MI_HIP_ERROR    -2
#define MI_RCCL_ERROR   -3
#define MI_NO_DEVICE    -4
#define MI_NO_MEMORY    -5
#define MI_UNSUPPORTED  -6   /* -> unsupported-constraint-error (integer / binary variables) */
#define MI_EXACT_OVERFLOW -7 /* exact tableaux: a value needs more than 128 bits -> unsupported-constraint-error */
#define MI_EXACT_INEXACT  -8 /* exact tableaux: a fraction-free division left a remainder (an internal error) */
/* batches of exact tableaux (mi355x_xbatch_*, below) */
#define MI355X_XBATCH_WORKGROUP 256    /* threads of the workgroup that owns a member */
#define MI355X_XBATCH_TRACE_CAP 1024   /* pivots a member's trace buffers hold (mi355x_xbatch_trace) */
/* batches of single-float tableaux (mi355x_sbatch_*, below) */
#define MI355X_SBATCH_TRACE_CAP 1024   /* pivots a member's trace buffers hold (mi355x_sbatch_trace) */

typedef struct mi355x_tab   mi355x_tab;     /* one tableau resident in HBM              */
typedef struct mi355x_batch mi355x_batch;   /* a batch of same-shape tableaux in HBM    */
typedef struct mi355x_problem  mi355x_problem;   /* a parsed LP, src/problem.lisp:45-53 (host)  */
typedef struct mi355x_solution mi355x_solution;  /* what the read-back needs of a solved tableau */
typedef struct mi355x_solve    mi355x_solve;     /* a problem on its way to a solution (resumable)  */
typedef struct mi355x_solve_many mi355x_solve_many; /* a LIST of problems on their way to solutions   */
typedef struct mi355x_xtab     mi355x_xtab;      /* one exact (fraction-free integer) tableau in HBM */
typedef struct mi355x_xbatch   mi355x_xbatch;    /* many exact tableaux of one shape, one workgroup per member */
typedef struct mi355x_xbb_base mi355x_xbb_base;  /* a base problem's general form, for exact branch-and-bound nodes */

/* ---- library / device ------------------------------------------------------------- */
int         mi355x_abi_version(void);
int         mi355x_device_count(void);             /* number of gfx950 devices visible, 0 if none */
const char *mi355x_last_error(void);               /* thread-local, never NULL */
double      mi355x_epsilon(void);                  /* CL double-float-epsilon used by the tolerances */
/* Optional: pay the one-off costs now instead of inside the first solve (the HIP context of
 * `device`, the library's code object, the pinned staging buffers of the streamed uploads) -- a host
 * calls it once when it loads the backend.  Idempotent; solves a 1-pivot LP on the device. */
int         mi355x_init(int device);

/* ---- tableau lifecycle  (tableau struct, src/simplex.lisp:48-58) ------------------- */
/* Upload a tableau.  host_basis has rows-1 entries (tableau-basis-columns) or is NULL. */
int  mi355x_tab_create(mi355x_tab **out, int64_t rows, int64_t cols,
                       const double *host_matrix, const int64_t *host_basis, int device);
/* Upload a tableau in COMPACT form: only the n_stored = var_count - (rows-1) non-basic columns
 * plus the RHS column (host_stored: rows x (n_stored+1), row-major; stored_cols[j] = logical column
 * of stored column j); the basic columns are BY DEFINITION the unit vectors host_basis describes
 * (what build-tableau produces for the slack columns of a single-phase problem).  The handle
 * behaves exactly like one made by mi355x_tab_create from the equivalent dense tableau -- the
 * dense logical form is materialised only if an entry point needs it -- but a third less data
 * crosses PCIe and no dense buffer is allocated for a plain solve + light read-back. */
int  mi355x_tab_create_compact(mi355x_tab **out, int64_t rows, int64_t var_count, int64_t n_stored,
                               const double *host_stored, const int64_t *stored_cols,
                               const int64_t *host_basis, int device);
/* Replace the contents of an existing handle (same shape). */
int  mi355x_tab_upload(mi355x_tab *t, const double *host_matrix, const int64_t *host_basis);
/* copy-tableau (src/simplex.lisp:61-71): device-to-device deep copy of matrix + basis. */
int  mi355x_tab_copy(mi355x_tab **out, const mi355x_tab *src);
/* Build the bench/test LP  max c'x, Ax <= b, x >= 0  directly in HBM
 * (splitmix64 stream; identical doubles to linear-programming_amd/synth.py):
 * tableau [A | I | b ; -c | 0 | 0], basis n_vars .. n_vars+n_cons-1.
 * col_begin/col_end select a column slice [col_begin, col_end) of the
 * var_count = n_vars+n_cons non-RHS columns (column-partitioned shards keep
 * the RHS column as their last column); pass 0, -1 for the whole tableau. */
int  mi355x_tab_create_synthetic(mi355x_tab **out, int64_t n_vars, int64_t n_cons,
                                 uint64_t seed, int64_t col_begin, int64_t col_end, int device);
void mi355x_tab_destroy(mi355x_tab *t);
int  mi355x_tab_shape(const mi355x_tab *t, int64_t *rows, int64_t *cols, int64_t *ld);

/* Which representation currently holds the tableau in HBM.  The solve entry points run on the
 * COMPACT representation [non-basic columns | RHS] (rows x (var_count - constraint_count + 1))
 * whenever the basis columns are exact unit vectors -- they are for every tableau
 * build-tableau produces, and pivoting keeps them so -- because basic columns never change
 * under a pivot; every other entry point sees the dense logical tableau (rebuilt on demand),
 * so the representation is invisible except through this query.  *stored_cols includes the
 * RHS column. */
int  mi355x_tab_layout(const mi355x_tab *t, int *compact, int64_t *stored_cols, int64_t *stored_ld);

/* ---- the hot path ------------------------------------------------------------------ */
/* n-pivot-row (src/simplex.lisp:337-359): normalise row `pivot_row` by its entry in
 * `entering_col`, eliminate that column from every other row (objective row included),
 * basis[pivot_row] = entering_col. */
int  mi355x_tab_pivot(mi355x_tab *t, int64_t entering_col, int64_t pivot_row);
/* find-entering-column (src/simplex.lisp:362-379): *col = column or -1 for NIL. */
int  mi355x_tab_price(mi355x_tab *t, int is_max, double fp_factor, int64_t *col);
/* find-pivoting-row (src/simplex.lisp:382-389): *row = row or -1 for NIL. */
int  mi355x_tab_ratio(mi355x_tab *t, int64_t entering_col, double fp_factor, int64_t *row);
/* n-solve-tableau, single-phase branch (src/simplex.lisp:453-461), entirely on the
 * device.  max_pivots = 0: no cap (as the reference).  Returns MI_OPTIMAL,
 * MI_UNBOUNDED or MI_MAX_PIVOTS; *n_pivots = pivots performed by this call. */
int  mi355x_tab_solve(mi355x_tab *t, int is_max, double fp_factor, int64_t max_pivots,
                      int64_t *n_pivots);
/* A way out of a blocking solve.  The reference's loop (src/simplex.lisp:453-461) has no iteration
 * cap and no anti-cycling rule; in Lisp a cycling LP can be interrupted, a blocking foreign call
 * cannot.  mi355x_tab_cancel may be called from ANY thread while another thread is inside
 * mi355x_tab_solve / mi355x_solve_two_phase on the same handle (the one exception to "one thread
 * at a time"): the solve returns MI_CANCELLED after the chunk of launches in flight -- at most 64
 * blocks of 16 pivots, 512 per-pivot iterations or one resident launch of 65536 pivots, i.e. well
 * under a second at every BASELINE size -- with *n_pivots = the pivots done and the tableau whole
 * (download / trace / a further solve call all work).  The request is sticky: cancelling a handle
 * nobody is solving cancels its next solve.  For mi355x_solve_two_phase cancel either (or both)
 * of the two handles.  The other way to keep a host responsive is max_pivots: solve in bounded
 * chunks and look around in between (what the Lisp glue does). */
int  mi355x_tab_cancel(mi355x_tab *t);
/* n-solve-tableau, two-phase branch (src/simplex.lisp:402-452): `art` is the
 * artificial tableau (a min problem), `main_tab` the main tableau with the same
 * row count; both are modified.  n_pivots[0] = phase 1 (incl. drive-out pivots),
 * n_pivots[1] = phase 2.  Returns MI_OPTIMAL / MI_UNBOUNDED / MI_INFEASIBLE /
 * MI_ART_NONZERO / MI_ART_STUCK. */
int  mi355x_solve_two_phase(mi355x_tab *art, mi355x_tab *main_tab, int main_is_max,
                            double fp_factor, int64_t *n_pivots);
/* The step BETWEEN the phases on its own (src/simplex.lisp:405-451), for a caller that drives the
 * phases itself in bounded chunks (mi355x_tab_solve(art, 0, f, cap, ..) until it is no longer
 * MI_MAX_PIVOTS, this, then mi355x_tab_solve(main_tab, ..) likewise -- what the Lisp glue and
 * mi355x_simplex_solver_step do): `art` holds the optimal artificial tableau; the feasibility test
 * (fp= 0 objective), the drive-out pivots of artificial variables still basic, rows and basis into
 * `main_tab`, its objective row re-eliminated.  *n_driveout = drive-out pivots made.  Returns MI_OK
 * (main_tab is ready for phase 2), MI_INFEASIBLE, MI_ART_NONZERO or MI_ART_STUCK. */
int  mi355x_two_phase_handover(mi355x_tab *art, mi355x_tab *main_tab, double fp_factor,
                               int64_t *n_driveout);

/* ---- read-back (src/simplex.lisp:74-120 needs last row, last column, basis) -------- */
/* Any pointer may be NULL.  host_matrix: rows*cols, host_basis: rows-1,
 * last_row: cols (objective row), last_col: rows (RHS column). */
int  mi355x_tab_download(mi355x_tab *t, double *host_matrix, int64_t *host_basis,
                         double *last_row, double *last_col);
/* A sub-block of the logical tableau -- (aref matrix r c) for r in [row0, row0+n_rows),
 * c in [col0, col0+n_cols) -- into a tightly packed row-major host array of n_rows*n_cols
 * doubles: single columns / rows / entries of tableaux too large to download whole. */
int  mi355x_tab_download_block(mi355x_tab *t, int64_t row0, int64_t n_rows, int64_t col0,
                               int64_t n_cols, double *host_block);
/* (entering column, pivot row) of the pivots made by solve calls since the last
 * upload / trace reset, oldest first; at most cap pairs are written, *n = number
 * of pivots recorded on the device (tracing holds up to 2^20 pairs). */
int  mi355x_tab_trace(mi355x_tab *t, int64_t *entering_cols, int64_t *pivot_rows,
                      int64_t cap, int64_t *n);

/* ---- asynchronous / measurement plumbing ------------------------------------------- */
/* Run the handle's kernels on an existing HIP stream (hipStream_t as void*), e.g.
 * torch.cuda.current_stream().cuda_stream -- NULL is HIP's default (null) stream, which is what
 * torch uses unless told otherwise.  use_own != 0: back to the handle's private stream. */
int  mi355x_tab_set_stream(mi355x_tab *t, void *hip_stream, int use_own);
/* Enqueue up to n_pivots iterations of price -> ratio -> pivot without any host
 * synchronisation (kernels turn into no-ops once the tableau is optimal/unbounded).
 * reset != 0 restarts the device-side pivot counter/status first. */
int  mi355x_tab_solve_async(mi355x_tab *t, int is_max, double fp_factor, int64_t n_pivots,
                            int reset);
/* Restart the device-side status / pivot counter of a handle and set its pivot cap
 * (0 = none) without touching the tableau. */
int  mi355x_tab_reset(mi355x_tab *t, int64_t max_pivots);
/* Wait for the stream; returns the device-side status (MI_OPTIMAL, MI_UNBOUNDED,
 * MI_MAX_PIVOTS, or MI_RUNNING when the enqueued iterations ran out first) and the number
 * of pivots done since the last reset.  That number can be smaller than what was enqueued even
 * with MI_RUNNING: after a non-finite entering column (the handle moved to the dense tableau) or
 * on a GPU shared with other work (the handle moved to the look-ahead form that needs no
 * co-resident workgroups) the rest of the request was dropped -- enqueue the difference again. */
int  mi355x_tab_sync(mi355x_tab *t, int64_t *n_pivots);
/* Per-launch HIP-event timing of the rank-1 update kernel (the bandwidth kernel):
 * enable = k > 0 brackets every k-th update launch with an event pair on the launch stream
 * (up to 4096 timed launches kept); 0 switches it off.  mi355x_tab_timing_read waits for the stream and returns
 * the number of timed launches, their summed and minimum duration in milliseconds,
 * then clears the record. */
int  mi355x_tab_timing_enable(mi355x_tab *t, int enable);
int  mi355x_tab_timing_read(mi355x_tab *t, int64_t *n_launches, double *sum_ms, double *min_ms);
/* Name of the rank-1 update kernel as it appears in rocprofv3 kernel traces. */
const char *mi355x_update_kernel_name(void);
/* Pivots one tableau-update launch of this handle applies in its current representation: > 1
 * when the solve loops run blocked (up to 16 pivots selected ahead, then applied by one k_sweep
 * launch; the timing above then brackets the sweeps), 1 for the plain k_update path.
 * Results do not depend on it. */
int  mi355x_tab_block_size(mi355x_tab *t);

/* ---- native host side of the hook: problem -> tableau -> solution ------------------- */
/* The reference's parsed `problem` struct (src/problem.lisp:45-53), variables identified by
 * their index in problem-vars.  A variable without a bounds entry is >= 0 (`positive`
 * mapping with offset 0); set_bounds(var, 0,_, 0,_) makes it free (`signed`, two columns).
 * op: 0 `<=`, 1 `>=`, 2 `=`; as after parsing, `<=` / `>=` rows carry rhs >= 0. */
int  mi355x_problem_create(mi355x_problem **out, int is_max, int64_t n_vars);
int  mi355x_problem_set_objective(mi355x_problem *p, const int64_t *var, const double *coef,
                                  int64_t nnz);
int  mi355x_problem_set_bounds(mi355x_problem *p, int64_t var, int has_lb, double lb, int has_ub,
                               double ub);
int  mi355x_problem_set_integer(mi355x_problem *p, int64_t var);
int  mi355x_problem_add_constraint(mi355x_problem *p, int op, const int64_t *var,
                                   const double *coef, int64_t nnz, double rhs);
void mi355x_problem_destroy(mi355x_problem *p);
/* The parsed problem as JSON text (inspection / tests).  Returns the length needed, writes at
 * most cap-1 characters plus a NUL. */
int64_t mi355x_problem_to_json(const mi355x_problem *p, char *buf, int64_t cap);
/* read-mps (src/external-formats.lisp:78-348): fixed-width MPS text -> problem.
 * default_is_max: 1 max, 0 min, -1 = the file's OBJSENSE section must say; rhs_id: name of the
 * RHS vector to use, NULL = the first one in the file; read_case: 0 upcase, 1 downcase,
 * 2 preserve, 3 invert (the reference's :read-case).  Variable names of the problem most
 * recently read by the calling thread, in problem-vars order: mi355x_mps_var_name. */
int  mi355x_problem_read_mps(const char *text, int64_t len, int default_is_max, const char *rhs_id,
                             int read_case, mi355x_problem **out);
/* The same with options.  flags = 0 is mi355x_problem_read_mps: single-variable rows are folded into
 * bounds exactly as the reference's loop does it (src/external-formats.lisp:312-323, quirks included:
 * a `<=` row writes (lb-max ub bound) into the upper bound, a `>=` row turns the variable integer, the
 * coefficient's sign is ignored, the constraint after a folded row is skipped).
 * MI_MPS_SINGLE_VARIABLE_ROWS_AS_MEANT: fold them the way the rows read instead (`<=` tightens the
 * upper bound, `>=` the lower bound, the sense flips for a negative coefficient, `=` fixes). */
#define MI_MPS_SINGLE_VARIABLE_ROWS_AS_MEANT 1
/* The default spelled out (flags = 0): the reference's loop, quirks included.  Since round 5 this is what
 * mi355x_problem_read_mps does (rounds 1-4 folded such rows "as meant": callers that want that behaviour back
 * pass MI_MPS_SINGLE_VARIABLE_ROWS_AS_MEANT to mi355x_problem_read_mps_ex).  Whenever the reference's loop
 * changes what a row means -- a `>=` / `=` row turns its variable INTEGER, a `<=` row takes the LARGER bound, the
 * constraint behind a folded row is skipped (its negative right-hand side not flipped) -- the call still
 * returns MI_OK and mi355x_last_error() holds a note naming the rows ("mps note: ..."; empty otherwise). */
#define MI_MPS_REFERENCE_COMPATIBLE 0
int  mi355x_problem_read_mps_ex(const char *text, int64_t len, int default_is_max, const char *rhs_id,
                                int read_case, int flags, mi355x_problem **out);
int64_t     mi355x_mps_var_count(void);
const char *mi355x_mps_var_name(int64_t i);
const char *mi355x_mps_objective_name(void);
/* build-tableau (src/simplex.lisp:142-328) in double-float, on the host.  which = 0: the main
 * tableau, 1: the artificial tableau (two-phase problems only).  Call once with NULL arrays for
 * the shape, again to fill matrix (rows*cols) and basis (rows-1).  Returns MI_UNBOUNDED for the
 * unbounded no-constraint special case (:170,:174). */
int  mi355x_build_tableau(const mi355x_problem *p, int which, int64_t *rows, int64_t *cols,
                          double *matrix, int64_t *basis, int *two_phase);
/* var-mapping entry of a variable (src/simplex.lisp:44-46): kind 0 positive, 1 negative,
 * 2 signed; first column; offset. */
int  mi355x_var_mapping(const mi355x_problem *p, int64_t var, int *kind, int64_t *col,
                        double *offset);
/* simplex-solver for LPs (src/simplex.lisp:506-542 without branch-and-bound): build-tableau,
 * upload, n-solve-tableau on the device (single- or two-phase), read back the objective row,
 * the RHS column and the basis only.  Returns MI_OPTIMAL and a solution, or MI_UNBOUNDED /
 * MI_INFEASIBLE / MI_UNSUPPORTED (integer variables) / an error. */
int  mi355x_simplex_solver(const mi355x_problem *p, double fp_tolerance, int device,
                           mi355x_solution **out);
/* The same solve as a resumable job, for a host that must never sit in an unbounded foreign call
 * (the reference's loop has no pivot cap and no anti-cycling rule, src/simplex.lisp:453-461; a Lisp
 * thread inside a foreign call cannot serve an interrupt).  begin: build-tableau + upload (declines
 * integer problems with MI_UNSUPPORTED, reports the unbounded no-constraint case as MI_UNBOUNDED).
 * step: at most max_pivots pivots (0 = no cap) of n-solve-tableau, across the phases of a two-phase
 * problem; *n_pivots = pivots of this call.  Returns MI_MAX_PIVOTS while the solve is still running
 * (call again: the continuation takes exactly the pivots one long call would), otherwise the final
 * status -- MI_OPTIMAL / MI_UNBOUNDED / MI_INFEASIBLE / MI_ART_NONZERO / MI_ART_STUCK, MI_CANCELLED
 * after mi355x_simplex_solver_cancel from another thread (a further step carries on).  finish: the
 * light read-back into a solution object (only after MI_OPTIMAL; MI_BAD_ARG otherwise) -- it always
 * consumes the job, as does abandon.  mi355x_simplex_solver = begin, step(0), finish. */
int  mi355x_simplex_solver_begin(const mi355x_problem *p, double fp_tolerance, int device,
                                 mi355x_solve **out);
int  mi355x_simplex_solver_step(mi355x_solve *job, int64_t max_pivots, int64_t *n_pivots);
int  mi355x_simplex_solver_cancel(mi355x_solve *job);
int  mi355x_simplex_solver_finish(mi355x_solve *job, mi355x_solution **out);
void mi355x_simplex_solver_abandon(mi355x_solve *job);
/* A LIST of problems (the hook takes one per call, src/solver.lisp:53-56; N small LPs one after the
 * other leave the GPU almost empty -- BASELINE config 4): what mi355x_simplex_solver returns for every
 * member, with the members solved side by side.  begin: build-tableau per member in C++, members of one
 * tableau shape and sense packed into ONE batch over n_devices GPUs (device_ids NULL = 0 .. n_devices-1;
 * two-phase members: a pair of batches), a member alone in its group as an ordinary job on the first
 * device; integer members are declined (MI_UNSUPPORTED) and unbounded no-constraint members decided here.
 * step: at most max_pivots pivots per member and phase (0 = no cap); returns MI_MAX_PIVOTS while some
 * member is still running (call again), MI_OK when every member has its final status.  status (n
 * entries, may be NULL): MI_RUNNING while undecided, then MI_OPTIMAL / MI_UNBOUNDED / MI_INFEASIBLE /
 * MI_ART_NONZERO / MI_ART_STUCK / MI_UNSUPPORTED.  finish: out[k] = the solution of member k (light
 * read-back) or NULL for a member without one; consumes the job, as does abandon. */
int  mi355x_simplex_solver_many_begin(const mi355x_problem *const *problems, int64_t n, double fp_tolerance,
                                      int n_devices, const int *device_ids, mi355x_solve_many **out);
int  mi355x_simplex_solver_many_step(mi355x_solve_many *job, int64_t max_pivots, int32_t *status);
int  mi355x_simplex_solver_many_finish(mi355x_solve_many *job, int32_t *status, mi355x_solution **out);
void mi355x_simplex_solver_many_abandon(mi355x_solve_many *job);
/* ---- exact rational tableaux  (the reference's `rational` dispatch, src/utils.lisp:84-124) -------
 * A tableau whose entries are all rational is solved with exact arithmetic: the device holds one
 * integer matrix T and one integer D > 0 with t_ij = T_ij / D (fraction-free, Bareiss), so pricing,
 * the ratio test and the phase-1 tests are the reference's exact comparisons and every value read back
 * is the exact rational the reference's tableau holds.  Pivot sequence, basis and entries are those of
 * src/simplex.lisp:337-461 under the rational dispatch.  Values are stored as 64-bit integers (128-bit
 * products) or 128-bit integers (256-bit products); a solve that overflows 64 bits restarts from the
 * initial tableau(s) at 128 bits (results do not depend on the width), one that overflows 128 bits ends
 * with MI_EXACT_OVERFLOW and the handle can only be destroyed -- unless the handle was created with
 * mi355x_xtab_create_wide and max_bits 256: then the solve restarts once more at 256 bits (four 64-bit limbs
 * per value, 512-bit products), and only what outgrows those ends with MI_EXACT_OVERFLOW.
 * Start state: with L_i the LCM of row i's denominators and the objective row's LCM multiplied into the
 * first constraint row's, D0 = prod L_i and T0 = D0 * t0 -- the state after the slack identity has been
 * pivoted, which needs the basis columns to be exact unit columns and the objective row zero on them
 * (what build-tableau produces, src/simplex.lisp:142-328); a solve of a tableau without that start returns
 * MI_UNSUPPORTED. */
/* Upload a build-tableau result: num / den are rows*cols (den > 0), basis has rows-1 entries (entries
 * outside [0, cols-1) are build-tableau's placeholders for artificial rows).  min_bits 0 or 64: start at
 * 64 bits when T0 fits, 128: start at 128.  MI_EXACT_OVERFLOW when T0 needs more than 128 bits. */
int  mi355x_xtab_create(mi355x_xtab **out, int64_t rows, int64_t cols, const int64_t *num,
                        const int64_t *den, const int64_t *basis, int device, int min_bits);
/* mi355x_xtab_create with the widest width the handle's solves may escalate to: max_bits 128 (exactly
 * mi355x_xtab_create) or 256.  min_bits 0, 64, 128 or 256, at most max_bits: the width to start at when T0
 * fits it (a T0 that does not starts at the next one that holds it).  Any other value of either is MI_BAD_ARG,
 * before a device is looked at.  MI_EXACT_OVERFLOW when T0 needs more than max_bits. */
int  mi355x_xtab_create_wide(mi355x_xtab **out, int64_t rows, int64_t cols, const int64_t *num,
                             const int64_t *den, const int64_t *basis, int device, int min_bits, int max_bits);
/* n-solve-tableau, single phase (src/simplex.lisp:453-461): at most max_pivots pivots (0 = no cap),
 * *n_pivots = pivots made by this call.  MI_OPTIMAL / MI_UNBOUNDED / MI_MAX_PIVOTS (a further call
 * carries on exactly) / MI_CANCELLED (mi355x_xtab_cancel from another thread; whole pivots only).
 * MI_EXACT_OVERFLOW once the widest width the handle allows is exceeded (the message names it); the handle
 * is dead from then on and every further call on it says the same. */
int  mi355x_xtab_solve(mi355x_xtab *t, int is_max, int64_t max_pivots, int64_t *n_pivots);
/* n-solve-tableau, two-phase branch (src/simplex.lisp:402-452): phase 1 on `art` (a min problem), the
 * exact feasibility test, the drive-out pivots (first non-basic column with a non-zero entry, negative
 * pivots included), the hand-over into `main_tab` (its objective row re-eliminated from the original
 * one: D * c - sum_i c[b_i] * T_i, after the constraint rows and D are multiplied by the LCM of c's
 * denominators) and phase 2.  max_pivots caps both phases together (0 = no cap); a call after
 * MI_MAX_PIVOTS or MI_CANCELLED carries on where the job stopped.  n_pivots[0] = phase-1 pivots made by
 * this call (drive-out pivots included; they are not in the trace, as in the reference's loop),
 * n_pivots[1] = phase-2 pivots.  Outcomes as mi355x_solve_two_phase.  The job runs at one width, both
 * tableaux restarting together; handles created with different max_bits are MI_BAD_ARG. */
int  mi355x_xtab_solve_two_phase(mi355x_xtab *art, mi355x_xtab *main_tab, int main_is_max,
                                 int64_t max_pivots, int64_t *n_pivots);
/* tableau-matrix / tableau-basis-columns (src/simplex.lisp:48-58): the raw T as (low, high) 64-bit
 * limbs of a two's complement 128-bit integer per entry (rows*cols*2), D likewise (2), the basis
 * (rows-1).  t_ij = T_ij / D.  Any pointer may be NULL. */
int  mi355x_xtab_download(mi355x_xtab *t, int64_t *num_lo_hi, int64_t *den_lo_hi, int64_t *basis);
/* The same with `limbs` little-endian 64-bit limbs per value (two's complement, sign-extended): entries
 * rows*cols*limbs, D limbs values.  limbs 2 or 4, and the handle's width at most 64 * limbs; anything else
 * is MI_BAD_ARG.  On a handle at 256 bits mi355x_xtab_download itself fails with MI_BAD_ARG (its message
 * names this form) and writes nothing: a value is never truncated. */
int  mi355x_xtab_download_limbs(mi355x_xtab *t, int limbs, int64_t *num_limbs, int64_t *den_limbs, int64_t *basis);
/* the (entering column, row) of every pivot chosen by the solve loops since the start, in order (the
 * drive-out pivots are not in it); at most cap, *n = all. */
int  mi355x_xtab_trace(mi355x_xtab *t, int64_t *entering_cols, int64_t *pivot_rows, int64_t cap, int64_t *n);
/* the width in use: 64, 128 or 256 */
int  mi355x_xtab_bits(const mi355x_xtab *t, int *bits);
/* mi355x_tab_cancel for the exact solves (any thread) */
int  mi355x_xtab_cancel(mi355x_xtab *t);
/* The pivot rule of the handle's solves: which column find-entering-column (src/simplex.lisp:362-379) and which
 * row find-pivoting-row (src/simplex.lisp:382-389) would choose is the default, MI_RULE_DANTZIG; the reference
 * has no anti-cycling rule, and on rationals a cycle never ends.  MI_RULE_BLAND replaces both choices: the
 * lowest column j < var_count whose objective entry is < 0 (max) / > 0 (min), and among the rows of the strict
 * minimum ratio the one whose basis column is lowest; it ends on every input (Bland's theorem).
 * MI_RULE_DANTZIG_BLAND is the default rule until a chosen pivot is degenerate (its row's right-hand side 0),
 * then Bland's until one is not; it ends on every input as well and makes far fewer pivots.  The drive-out
 * pivots are not affected.  The rule belongs to the handle: it survives the restart at a wider width.  Set it
 * on both handles of a two-phase pair.  MI_BAD_ARG for an unknown rule and for a handle that has made a pivot. */
enum { MI_RULE_DANTZIG = 0, MI_RULE_BLAND = 1, MI_RULE_DANTZIG_BLAND = 2 };
int  mi355x_xtab_set_pivot_rule(mi355x_xtab *t, int rule);
void mi355x_xtab_destroy(mi355x_xtab *t);
/* ---- batches of exact rational tableaux  (n-solve-tableau, src/simplex.lisp:399-461, under the rational
 * dispatch of src/utils.lisp:84-124, for many problems of one shape at once) ------------------------------
 * n_lps tableaux of one shape, each solved exactly as mi355x_xtab_* solves one -- the same pivot sequence,
 * basis and entries -- but side by side: one workgroup owns one member for its whole solve
 * (src/simplex.lisp:453-461 inside one launch), and everything between the phases (src/simplex.lisp:405-451:
 * feasibility test, drive-out pivots, hand-over) runs on the device per member as well.
 * Status per member (status[], n_lps entries, may be NULL): MI_OPTIMAL / MI_UNBOUNDED / MI_INFEASIBLE /
 * MI_ART_NONZERO / MI_ART_STUCK / MI_MAX_PIVOTS, MI_EXACT_OVERFLOW for a member that needs more than 128 bits,
 * MI_UNSUPPORTED for one whose start is not unit basis columns over a zero objective entry, MI_RUNNING for
 * one a cancel left unfinished.  One member's outcome never changes another's; the calls themselves return
 * MI_OK, MI_CANCELLED or an error.
 * Width: every member starts at 64 bits when its start state fits (min_bits as for mi355x_xtab_create); a
 * member that overflows 64 bits starts again from its own start state at 128 bits, both phases of a
 * two-phase job, and replays up to the same cumulative pivot count beside the other restarted members.
 * Results never depend on the width.
 * A shape whose pivot-row and entering-column snapshots ((rows + cols) values of 128 bits) do not fit the
 * LDS a workgroup may have is declined by create with MI_UNSUPPORTED.  (MI355X_XBATCH_WORKGROUP and
 * MI355X_XBATCH_TRACE_CAP, above: the workgroup's threads and the pivots a member's trace buffers hold.) */
/* num / den / basis: the members back to back, each as for mi355x_xtab_create. */
int  mi355x_xbatch_create(mi355x_xbatch **out, int64_t n_lps, int64_t rows, int64_t cols,
                          const int64_t *num, const int64_t *den, const int64_t *basis,
                          int device, int min_bits);
/* Single phase (src/simplex.lisp:453-461): at most max_pivots pivots per member by this call (0 = no cap);
 * a further call carries every unfinished member on exactly where it stopped.  n_pivots (n_lps entries, may
 * be NULL): pivots made by this call. */
int  mi355x_xbatch_solve(mi355x_xbatch *b, int is_max, int64_t max_pivots,
                         int32_t *status, int64_t *n_pivots);
/* Two-phase (src/simplex.lisp:402-452), member q of `art` with member q of `main_b`: max_pivots caps both
 * phases of a member together, the drive-out pivots counted in phase 1 (they are not in the trace).  The
 * drive-out pivots of a member are made in one step, as by mi355x_xtab_solve_two_phase: the call that ends
 * a member's phase 1 may exceed max_pivots by its drive-outs (phase 2 then waits for the next call);
 * n_pivots holds 2 values per member (phase 1, phase 2), the pivots made by this call. */
int  mi355x_xbatch_solve_two_phase(mi355x_xbatch *art, mi355x_xbatch *main_b, int main_is_max,
                                   int64_t max_pivots, int32_t *status, int64_t *n_pivots);
/* member lp_index as mi355x_xtab_download returns one tableau */
int  mi355x_xbatch_download(mi355x_xbatch *b, int64_t lp_index, int64_t *num_lo_hi,
                            int64_t *den_lo_hi, int64_t *basis);
/* member lp_index's pivots as mi355x_xtab_trace: the buffers hold the first MI355X_XBATCH_TRACE_CAP, *n = all */
int  mi355x_xbatch_trace(mi355x_xbatch *b, int64_t lp_index, int64_t *entering_cols,
                         int64_t *pivot_rows, int64_t cap, int64_t *n);
/* the width member lp_index uses: 64 or 128 */
int  mi355x_xbatch_bits(const mi355x_xbatch *b, int64_t lp_index, int *bits);
/* any thread: the call running on the batch returns MI_CANCELLED after its current launches (whole pivots) */
int  mi355x_xbatch_cancel(mi355x_xbatch *b);
/* mi355x_xtab_set_pivot_rule for every member of the batch, at either width: what replaces find-entering-column
 * (src/simplex.lisp:362-379) and find-pivoting-row (src/simplex.lisp:382-389) in its solves.  Set it on both
 * batches of a two-phase pair, those of mi355x_xbatch_create_nodes included.  MI_BAD_ARG for an unknown rule
 * and for a batch one of whose members has made a pivot. */
int  mi355x_xbatch_set_pivot_rule(mi355x_xbatch *b, int rule);
void mi355x_xbatch_destroy(mi355x_xbatch *b);
/* ---- exact branch-and-bound  (simplex-solver with integer variables on rationals, src/simplex.lisp:462-542,
 * where violated-integer-constraint's integerp, :475-480, is meaningful) ------------------------------------
 * The search, build-tableau of the base problem and the reading of solutions stay in the host language,
 * which has bignums.  The library turns a base problem and lists of node rows into batches of exact start
 * states on the device, and gathers what tableau-objective-value / -variable / -reduced-cost read. */
/* The base problem's general-form tableau -- build-tableau's main tableau (src/simplex.lisp:189-283) with
 * basis[i] == cols for a row that needs an artificial variable -- as rationals num / den, plus what places
 * a node row: ncv structural columns, nb rows pushed for doubly-bounded variables (:198-202; node rows go
 * after them, :146), and per variable its var-mapping (:189-212): kind 0 positive / 1 negative / 2 signed,
 * its column, its offset off_num / off_den.  MI_EXACT_OVERFLOW when the problem at one integer scale needs
 * more than 128 bits.  A base may be destroyed while batches made from it live. */
int  mi355x_xbb_base_create(mi355x_xbb_base **out, int64_t rows, int64_t cols, const int64_t *num,
                            const int64_t *den, const int64_t *basis, int64_t ncv, int64_t nb,
                            int64_t n_vars, const int32_t *kind, const int64_t *col,
                            const int64_t *off_num, const int64_t *off_den, int device);
void mi355x_xbb_base_destroy(mi355x_xbb_base *base);
/* build-and-solve's tableaux (src/simplex.lisp:489-500 through build-tableau, :142-328) of n_nodes nodes of
 * one depth and one number of artificial rows, written on the device: node q is the base problem with the
 * rows var <= bound (sense 0) / var >= bound (sense 1) at [q * depth, (q + 1) * depth), newest first, in
 * front of its constraints.  *out_main is a batch of (rows + depth) x (cols + depth) members; *out_art is
 * NULL when no row is artificial (solve *out_main with mi355x_xbatch_solve), else the batch of artificial
 * tableaux (solve the pair with mi355x_xbatch_solve_two_phase).  Both are ordinary mi355x_xbatch handles;
 * a member whose start state needs more than 128 bits reports MI_EXACT_OVERFLOW when solved.  MI_BAD_ARG
 * when the nodes differ in their number of artificial rows; MI_UNSUPPORTED for a shape
 * mi355x_xbatch_create declines.  min_bits as for mi355x_xbatch_create. */
int  mi355x_xbatch_create_nodes(mi355x_xbatch **out_main, mi355x_xbatch **out_art,
                                const mi355x_xbb_base *base, int64_t n_nodes, int64_t depth,
                                const int64_t *var, const int32_t *sense, const int64_t *bound,
                                int min_bits);
/* build-tableau (src/simplex.lisp:214-328) of n_lps problems of one shape, written on the device: a batch of
 * exact LPs straight from the problems' rows, with no tableau built on the host.  Member q is given in column
 * space, as build-tableau holds it after :189-241 and before :243, at q * (m + 1) * (ncv + 1): rows 0 .. m-1 are
 * the ncv structural coefficients and, last, the right-hand side with the offsets already subtracted; row m is
 * the objective row as :270-283 stores it, the signs applied, the constant last.  Every entry is a reduced
 * fraction num / den (den > 0, gcd(|num|, den) == 1, zero is 0 / 1); sense (n_lps x m): 0 `<=`, 1 `>=`, 2 `=`.
 * What the members start from is what build-tableau followed by mi355x_xbatch_create gives, entry for entry: a
 * row whose right-hand side is < 0 negated and its sense flipped (:243-252), slack columns in row order for
 * the rows that are not `=` (:254-265), artificial columns in decreasing row order (:257, :261, :296-300), the
 * artificial objective row (:302-316), and the integer scale of mi355x_xtab_create.  *out_main is a batch of
 * (m + 1) x (ncv + n_slack + 1) members; *out_art is NULL when no row is artificial (solve *out_main with
 * mi355x_xbatch_solve), else the batch of artificial tableaux with n_art more columns (solve the pair with
 * mi355x_xbatch_solve_two_phase).  Both are ordinary mi355x_xbatch handles; the rows stay on the device while
 * either lives, and a member that overflows 64 bits is assembled again from them at 128 bits.  A tableau
 * leaves a width exactly when its common denominator or one of its entries does -- no intermediate of the
 * assembly is larger -- and a member whose start state needs more than 128 bits reports MI_EXACT_OVERFLOW
 * when solved.  MI_BAD_ARG (the message names the member) for m < 1, ncv < 1, a fraction that is not reduced, a
 * sense outside 0 .. 2, and members that differ in their number of `=` rows or of artificial rows;
 * MI_UNSUPPORTED for exactly the shapes mi355x_xbatch_create declines.  min_bits as for mi355x_xbatch_create. */
int  mi355x_xbatch_create_lps(mi355x_xbatch **out_main, mi355x_xbatch **out_art,
                              int64_t n_lps, int64_t m, int64_t ncv,
                              const int64_t *num, const int64_t *den, const int32_t *sense,
                              int device, int min_bits);
/* All that tableau-objective-value, tableau-variable and tableau-reduced-cost read (src/simplex.lisp:74-120)
 * of every member, in one copy: values_lo_hi holds per member 1 + rows + cols limb pairs -- D, the last
 * column (rows values), the last row (cols values) --, basis (may be NULL) rows - 1 entries per member.
 * status (n_lps entries, may be NULL): MI_OK, or MI_EXACT_OVERFLOW for a member past 128 bits (zeros). */
int  mi355x_xbatch_readback(mi355x_xbatch *b, int64_t *values_lo_hi, int64_t *basis, int32_t *status);
/* Branch-and-bound (simplex-solver with integer variables, src/simplex.lisp:462-542) as a resumable job.
 * Opt-in: every other entry point still declines integer problems with MI_UNSUPPORTED.  The search is the
 * reference's node for node -- a depth-first walk over an explicit stack of entries, each node the problem
 * with the entry's rows (newest first) in front of its own constraints, the first integer variable of
 * int_order (problem-integer-vars, in order) whose value is not integral branched on, the `<=` child on
 * top, an integral node kept only when strictly better, a non-integral one dropped when not better than
 * the incumbent.  Node LPs are solved ahead of time, up to `width` of them side by side (same-shape
 * nodes in one multi-device batch over n_devices GPUs, device_ids NULL = 0 .. n_devices-1); the result,
 * the trace and every value are the same for every width.
 * Integrality of the double-float path: a value is integral iff it is an integer-valued double
 * (v == floor(v), the f64 reading of integerp); int_tolerance > 0 (in units of CL's double-float-epsilon,
 * like fp_tolerance) counts |v - round(v)| <= int_tolerance * epsilon as integral instead.  The value
 * tested is mi355x_solution_variable's; the branching bounds are floor(v) and ceiling(v).
 * begin: arguments checked (MI_BAD_ARG), then MI_NO_DEVICE without a device; nothing is solved yet.
 * step: processes at most max_nodes nodes (0 = no cap); *n_nodes = nodes processed by this call.  Returns
 * MI_MAX_PIVOTS while the search is running (call again: the continuation is exactly what one call would
 * do), otherwise the final status: MI_OPTIMAL (an incumbent), MI_INFEASIBLE (none), MI_UNBOUNDED /
 * MI_ART_NONZERO / MI_ART_STUCK (a node LP ended so, raised when that node is reached in DFS order), or
 * MI_CANCELLED after mi355x_simplex_solver_bb_cancel from another thread (a further step carries on).
 * finish: the incumbent's solution (only after MI_OPTIMAL, MI_BAD_ARG otherwise); consumes the job, as
 * does abandon.  stats: nodes processed, node LPs solved (speculative ones included), deepest node
 * processed.  trace: the processed nodes in order -- parent (its index in the trace, -1 for the root),
 * the branching row that made the node (var, sense 0 `<=` / 1 `>=`, bound; var -1 for the root), the
 * outcome (MI_BB_*) and the node's objective value (NaN without one); at most cap rows, *n = all. */
#define MI_BB_INFEASIBLE  0   /* the node LP is infeasible: dropped                              */
#define MI_BB_PRUNED      1   /* not integral and not better than the incumbent: dropped         */
#define MI_BB_BRANCHED    2   /* not integral: its two children pushed                           */
#define MI_BB_INCUMBENT   3   /* integral and better: the new incumbent                          */
#define MI_BB_NOT_BETTER  4   /* integral, not better than the incumbent                         */
#define MI_BB_FAILED      5   /* the node LP ended the search (unbounded, artificial variables)  */
typedef struct mi355x_bb mi355x_bb;
int  mi355x_simplex_solver_bb_begin(const mi355x_problem *p, const int64_t *int_order, int64_t n_int,
                                    double fp_tolerance, double int_tolerance, int64_t width, int n_devices,
                                    const int *device_ids, mi355x_bb **out);
int  mi355x_simplex_solver_bb_step(mi355x_bb *job, int64_t max_nodes, int64_t *n_nodes);
int  mi355x_simplex_solver_bb_cancel(mi355x_bb *job);
int  mi355x_simplex_solver_bb_finish(mi355x_bb *job, mi355x_solution **out);
void mi355x_simplex_solver_bb_abandon(mi355x_bb *job);
int  mi355x_simplex_solver_bb_stats(const mi355x_bb *job, int64_t *n_processed, int64_t *n_solved,
                                    int64_t *max_depth);
int  mi355x_simplex_solver_bb_trace(const mi355x_bb *job, int64_t *parent, int64_t *var, int32_t *sense,
                                    double *bound, int32_t *outcome, double *objective, int64_t cap,
                                    int64_t *n);
/* tableau-objective-value / tableau-variable / tableau-reduced-cost (src/simplex.lisp:74-120).
 * reduced_cost fails with MI_BAD_ARG for a variable without a lower bound, as the reference. */
int  mi355x_solution_objective_value(const mi355x_solution *s, double *out);
int  mi355x_solution_variable(const mi355x_solution *s, int64_t var, double *out);
int  mi355x_solution_reduced_cost(const mi355x_solution *s, int64_t var, double *out);
int  mi355x_solution_pivots(const mi355x_solution *s, int64_t *phase1, int64_t *phase2);
void mi355x_solution_destroy(mi355x_solution *s);

/* ---- batches of independent LPs (BASELINE config 4) -------------------------------- */
/* n_lps same-shape LPs stacked in one allocation; one (select, update) launch pair advances
 * every unfinished LP by one pivot.  host_matrices: n_lps * rows * cols doubles,
 * host_bases: n_lps * (rows-1) (may be NULL). */
int  mi355x_batch_create(mi355x_batch **out, int64_t n_lps, int64_t rows, int64_t cols,
                         const double *host_matrices, const int64_t *host_bases, int device);
/* The synthetic LP of mi355x_tab_create_synthetic, one per seed (seeds: n_lps host values). */
int  mi355x_batch_create_synthetic(mi355x_batch **out, int64_t n_lps, int64_t n_vars,
                                   int64_t n_cons, const uint64_t *seeds, int device);
/* n-solve-tableau (single phase) on every LP of the batch; status[i] (MI_OPTIMAL /
 * MI_UNBOUNDED / MI_MAX_PIVOTS) and n_pivots[i] per LP (host arrays, may be NULL).
 * max_pivots = 0: no cap.  Returns MI_OK or an error. */
int  mi355x_batch_solve(mi355x_batch *b, int is_max, double fp_factor, int64_t max_pivots,
                        int32_t *status, int64_t *n_pivots);
int  mi355x_batch_download(mi355x_batch *b, int64_t lp_index, double *host_matrix,
                           int64_t *host_basis, double *last_row, double *last_col);
/* HIP-event timing of the batched update launches (see mi355x_tab_timing_*). */
/* Optional: do now what the first mi355x_batch_solve would do first -- allocate and fill the
 * representation the solve loop runs on -- so that a timed solve contains no allocation. */
int  mi355x_batch_prepare(mi355x_batch *b);
int  mi355x_batch_timing_enable(mi355x_batch *b, int enable);
int  mi355x_batch_timing_read(mi355x_batch *b, int64_t *n_launches, double *sum_ms, double *min_ms);
void mi355x_batch_destroy(mi355x_batch *b);

/* The same without blocking the caller: the batch loop is driven by the host (blind chunks of
 * launches, one status read-back per chunk), so the asynchronous form runs it on a worker thread
 * of the library; mi355x_batch_sync waits for it and delivers what mi355x_batch_solve delivers.
 * One solve at a time per batch; the batch must not be touched in between.  (How a
 * single-threaded host -- the Lisp image -- keeps the sub-batches of several GPUs going.) */
int  mi355x_batch_solve_async(mi355x_batch *b, int is_max, double fp_factor, int64_t max_pivots);
int  mi355x_batch_sync(mi355x_batch *b, int32_t *status, int64_t *n_pivots);
/* mi355x_tab_cancel for batches (any thread): the solve in flight -- blocking, or on the library's
 * worker thread -- returns MI_CANCELLED (mi355x_batch_solve / _sync / mi355x_multibatch_solve)
 * after its current chunk of launches; status[i] = MI_RUNNING for the LPs it left unfinished,
 * every tableau whole.  (The per-LP kernels end a launch after 4096 pivots per LP at the latest.) */
int  mi355x_batch_cancel(mi355x_batch *b);

/* One batch over several devices (config 4 as specified: 1024 LPs over 8 GPUs): LP k lives in
 * sub-batch k / ceil(n_lps / n_devices) (contiguous blocks, one sub-batch per device), independent
 * units, no communication.  mi355x_multibatch_solve starts every sub-batch's loop on its own worker
 * thread and waits; status / n_pivots are indexed by the GLOBAL LP index.  device_ids: one per
 * sub-batch, or NULL = devices 0 .. n_devices-1 -- with fewer visible devices than that the
 * sub-batches become logical sub-batches on device 0 (own stream each; how the path is tested on
 * one GPU).  n_devices is capped at n_lps; mi355x_multibatch_info reports what is in use. */
typedef struct mi355x_multibatch mi355x_multibatch;
int  mi355x_multibatch_create(mi355x_multibatch **out, int64_t n_lps, int64_t rows, int64_t cols,
                              const double *host_matrices, const int64_t *host_bases, int n_devices,
                              const int *device_ids);
int  mi355x_multibatch_create_synthetic(mi355x_multibatch **out, int64_t n_lps, int64_t n_vars,
                                        int64_t n_cons, const uint64_t *seeds, int n_devices,
                                        const int *device_ids);
int  mi355x_multibatch_info(const mi355x_multibatch *mb, int *n_sub_batches, int *n_devices_used);
int  mi355x_multibatch_solve(mi355x_multibatch *mb, int is_max, double fp_factor, int64_t max_pivots,
                             int32_t *status, int64_t *n_pivots);
int  mi355x_multibatch_download(mi355x_multibatch *mb, int64_t lp_index, double *host_matrix,
                                int64_t *host_basis, double *last_row, double *last_col);
/* n-solve-tableau, two-phase branch (src/simplex.lisp:402-452), member by member of two matching
 * batches: member k of `art` is the artificial tableau (a min problem) of the problem whose main
 * tableau is member k of `main_mb` (same member count, row count and sub-batch layout).  Phase 1 runs
 * as the batch loop on `art`; the feasibility test (fp= 0 objective), the drive-out pivots of
 * artificial variables still basic (419-434: row fetches and single pivots on that member inside the
 * batch) and the hand-over (437-451) run per member on the devices; phase 2 is the batch loop on
 * `main_mb`.  status[k]: MI_OPTIMAL / MI_UNBOUNDED / MI_INFEASIBLE / MI_ART_NONZERO / MI_ART_STUCK as
 * mi355x_solve_two_phase.  n_pivots: two entries per member (phase 1 incl. drive-out pivots, phase
 * 2), may be NULL.  Read results with mi355x_multibatch_download(main_mb, k, ...).
 * mi355x_multibatch_two_phase_handover is the step between the phases on its own, for a caller that
 * drives both phases in bounded chunks (mi355x_multibatch_solve with a cap, what the Lisp glue does):
 * phase1_status = the per-member statuses phase 1 ended with (NULL: all MI_OPTIMAL); status[k] = MI_OK
 * when member k of main_mb is ready for phase 2, otherwise that member's final outcome (its main
 * tableau is then neutralised so that the batch loop of phase 2 passes over it); n_driveout per
 * member, may be NULL. */
int  mi355x_multibatch_two_phase_handover(mi355x_multibatch *art, mi355x_multibatch *main_mb,
                                          double fp_factor, const int32_t *phase1_status,
                                          int32_t *status, int64_t *n_driveout);
int  mi355x_multibatch_solve_two_phase(mi355x_multibatch *art, mi355x_multibatch *main_mb, int main_is_max,
                                       double fp_factor, int32_t *status, int64_t *n_pivots);
int  mi355x_multibatch_cancel(mi355x_multibatch *mb);
void mi355x_multibatch_destroy(mi355x_multibatch *mb);
/* build-tableau (src/simplex.lisp:243-328) of n_lps problems of one shape, written on the device(s): batches
 * straight from the problems' rows, with no dense tableau built or uploaded by the host (opt-in; what
 * mi355x_xbatch_create_lps is for the exact batches, in doubles).  Member q is given in column space, as
 * build-tableau holds it after :189-241 and before :243, at lps + q * (m + 1) * (ncv + 1): rows 0 .. m-1 are the
 * ncv structural coefficients and, last, the right-hand side with the offsets already subtracted; row m is the
 * objective row as :270-283 stores it, the signs applied, the constant last.  sense (n_lps x m): 0 `<=`, 1 `>=`,
 * 2 `=`.  Every entry and every basis entry the members start from is what mi355x_build_tableau produces, bit for
 * bit, the sign of zero included: a row whose right-hand side is < 0.0 negated and its sense flipped (:243-252;
 * not -0.0, not NaN), slack columns in row order for the rows that are not `=` (:254-265; the other slack
 * columns of a negated row hold -0.0), artificial columns in decreasing row order (:257, :261, :296-300), the
 * artificial objective row summed in increasing row order from 0.0 (:302-316).  *out_main is a batch of
 * (m + 1) x (ncv + n_slack + 1) members whose basis entry is the number of columns on an artificial row;
 * *out_art is NULL when no row is artificial (solve *out_main), else the batch of artificial tableaux with n_art
 * more columns (phase 1 on *out_art, mi355x_multibatch_two_phase_handover, phase 2 on *out_main, or
 * mi355x_multibatch_solve_two_phase).  Both are ordinary handles in the state mi355x_*batch_create leaves: every
 * solve, hand-over, download, cancel and destroy entry serves them.  The multibatch form splits the members as
 * mi355x_multibatch_create does and sends each sub-batch's rows to its device.  MI_BAD_ARG (before any device is
 * looked for; the message names the member) for a NULL array, m < 1, ncv < 1, a sense outside 0 .. 2, and
 * members that differ in their number of `=` rows or of artificial rows -- a row is artificial when it is `=`
 * or, after the flip, `>=`. */
int  mi355x_batch_create_lps(mi355x_batch **out_main, mi355x_batch **out_art,
                             int64_t n_lps, int64_t m, int64_t ncv,
                             const double *lps, const int32_t *sense, int device);
int  mi355x_multibatch_create_lps(mi355x_multibatch **out_main, mi355x_multibatch **out_art,
                                  int64_t n_lps, int64_t m, int64_t ncv,
                                  const double *lps, const int32_t *sense,
                                  int n_devices, const int *device_ids);
/* All that tableau-objective-value, tableau-variable and tableau-reduced-cost read (src/simplex.lisp:74-120) of
 * every member, gathered on the device and fetched with one copy per sub-batch: last_rows n_lps x cols, last_cols
 * n_lps x rows, bases n_lps x (rows - 1), by the global member index; each may be NULL. */
int  mi355x_batch_readback(mi355x_batch *b, double *last_rows, double *last_cols, int64_t *bases);
int  mi355x_multibatch_readback(mi355x_multibatch *mb, double *last_rows, double *last_cols, int64_t *bases);

/* ---- column-partitioned tableau: per-shard steps (BASELINE config 5) --------------- */
/* One tableau whose non-RHS columns are split across shards (one shard = one handle = one
 * GPU / rank; every shard keeps its own copy of the RHS column as its last column and updates
 * it redundantly).  One pivot = three local steps and two exchanges, all asynchronous on the
 * handle's stream (see mi355x_tab_set_stream), none needing the host to know who owns the
 * entering column:
 *   1. mi355x_shard_price       local pricing winner -> dev_out2 = {key, global column}
 *      -- exchange A: all-gather of the 2 doubles of every shard
 *   2. mi355x_shard_contribute  every shard derives the same global winner (lexicographic
 *      (key, column) minimum == lowest-index strict minimum) and applies the threshold;
 *      the owner writes the entering column's bit patterns (rows int64) to dev_col_bits,
 *      everyone else zeros; dev_ec = global entering column or -1
 *      -- exchange B: integer SUM all-reduce of dev_col_bits (= broadcast from the owner)
 *   3. mi355x_shard_pivot       ratio test on the exchanged column against the own RHS copy
 *      (same result on every shard), normalise own slice of the pivot row, rank-1 update
 *      of own slice, basis[cr] = global column.
 * col_offset = global index of the shard's first column.  dev_* are raw device addresses
 * (e.g. torch tensors' data_ptr()).  Status/pivot count: mi355x_tab_sync. */
/* A COMPACT shard stores only non-basic columns (plus the RHS copy): global_cols[j] is the
 * global logical column held in local slot j (cols-1 entries, host array).  The shard that
 * owns the entering column hands its slot over to the leaving basic column at every pivot
 * (DESIGN.md 4.5), so ownership of logical columns moves between slots but a shard's size never
 * changes and basic columns are stored nowhere.  basis[] holds global column indices.
 * mi355x_shard_columns reads the current slot -> global column map back. */
/* global_cols[j] == -1: slot j is DEAD -- stored and updated like any other column, never priced
 * and owned by no logical column (what the two-phase hand-over leaves in a shard that held
 * artificial columns only). */
int  mi355x_shard_set_compact(mi355x_tab *t, int64_t global_var_count, const int64_t *global_cols);
int  mi355x_shard_columns(mi355x_tab *t, int64_t *global_cols);
int  mi355x_shard_price(mi355x_tab *t, int is_max, int64_t col_offset, double *dev_out2);
int  mi355x_shard_contribute(mi355x_tab *t, const double *dev_gathered, int n_shards,
                             int64_t col_offset, double fp_factor, int64_t *dev_col_bits,
                             int64_t *dev_ec);
int  mi355x_shard_pivot(mi355x_tab *t, const int64_t *dev_col_bits, const int64_t *dev_ec,
                        double fp_factor);
/* Blocked form of the three steps: `step` = 0 .. 15 within a block.  The
 * exchanges are the same two per pivot; the shard's slice of the tableau is NOT updated by
 * mi355x_shard_la_pivot -- the pending pivots are chained through on whatever a step reads --
 * and mi355x_shard_sweep applies all pending pivots in one pass (call it after the last step of
 * a block, at the latest after 16 steps, and before anything else touches the shard). */
int  mi355x_shard_la_contribute(mi355x_tab *t, int step, const double *dev_gathered, int n_shards,
                                int64_t col_offset, double fp_factor, int64_t *dev_col_bits,
                                int64_t *dev_ec);
int  mi355x_shard_la_pivot(mi355x_tab *t, int step, const int64_t *dev_col_bits, const int64_t *dev_ec,
                           double fp_factor);
int  mi355x_shard_sweep(mi355x_tab *t);

/* ---- column-partitioned tableau: the whole solve behind one handle (BASELINE config 5) ---- */
/* n-solve-tableau (src/simplex.lisp:453-461, single phase) on ONE tableau whose non-RHS columns
 * are distributed over n_devices GPUs: the driver of the per-shard steps above lives in the
 * library, with the two exchanges per pivot issued from C++ on the shards' streams --
 *   * one process, several GPUs (what the Lisp host uses: `:devices n`): one shard and one host
 *     thread per device, RCCL communicators from ncclCommInitAll, exchange A = ncclAllGather of
 *     16 bytes per shard, exchange B = ncclAllReduce(int64 SUM) of the entering column's bit
 *     patterns (owner's bits + zeros == a broadcast whose root no host needs to know);
 *   * fewer visible devices than shards: the shards become LOGICAL shards on device 0 and the
 *     exchanges device-local kernels with the collectives' semantics (same pivots, same bits:
 *     how the partitioned path is tested on one GPU);
 *   * one process per GPU (torch.distributed.run / mpirun): every rank creates the handle with
 *     world/rank and the 128-byte id rank 0 obtained from mi355x_rccl_unique_id, the
 *     communicator comes from ncclCommInitRank, the per-pivot loop is still entirely in here.
 * Shards are compact (only non-basic columns are distributed) whenever the basis columns of the
 * uploaded tableau are exact unit vectors, dense otherwise; pivoting is blocked (16 pivots per
 * sweep of a shard's slice).  A failing RCCL call returns MI_RCCL_ERROR; the communicators are then
 * aborted (the other ranks' pending collectives could never complete) and the handle can only be
 * destroyed.
 * n_devices >= 1; a tableau with fewer distributable columns than that gets one shard per column
 * (mi355x_colpart_info reports the number in use).  Results are bit-identical to mi355x_tab_solve
 * on one device. */
typedef struct mi355x_colpart mi355x_colpart;
int  mi355x_colpart_create(mi355x_colpart **out, int64_t rows, int64_t cols,
                           const double *host_matrix, const int64_t *host_basis, int n_devices);
/* the same on chosen devices: device_ids[0 .. n_devices) (distinct), NULL = devices 0 .. n_devices-1.
 * Logical shards (fewer visible devices than shards) all live on device_ids[0]. */
int  mi355x_colpart_create_on(mi355x_colpart **out, int64_t rows, int64_t cols,
                              const double *host_matrix, const int64_t *host_basis, int n_devices,
                              const int *device_ids);
/* the synthetic LP of mi355x_tab_create_synthetic generated shard by shard in HBM (benchmarks) */
int  mi355x_colpart_create_synthetic(mi355x_colpart **out, int64_t n_vars, int64_t n_cons,
                                     uint64_t seed, int n_devices);
/* one process per GPU: this rank's shard of a world of `world` shards, on `device` */
int  mi355x_rccl_unique_id(void *id128);
int  mi355x_colpart_create_synthetic_rank(mi355x_colpart **out, int64_t n_vars, int64_t n_cons,
                                          uint64_t seed, int world, int rank, int device,
                                          const void *id128);
/* number of shards, of distinct physical devices they live on, and whether the exchanges are
 * RCCL collectives (1) or device-local kernels (0) */
int  mi355x_colpart_info(const mi355x_colpart *p, int *n_shards, int *n_devices_used, int *uses_rccl);
/* n-solve-tableau; max_pivots = 0: no cap.  MI_OPTIMAL / MI_UNBOUNDED / MI_MAX_PIVOTS /
 * MI_NONFINITE (compact shards, see above) or an error */
int  mi355x_colpart_solve(mi355x_colpart *p, int is_max, double fp_factor, int64_t max_pivots,
                          int64_t *n_pivots);
/* n-solve-tableau, two-phase branch (src/simplex.lisp:402-452) with the artificial tableau
 * column-partitioned (`art`: made by mi355x_colpart_create[_on] from the artificial tableau of
 * build-tableau; its basis columns are unit columns, so its shards are compact).  Phase 1 = the
 * partitioned loop on `art` (a min problem); the feasibility test (fp= 0 objective), the drive-out
 * pivots of artificials still basic (the owner contributes the chosen column, one exchange, every
 * shard pivots on the given row) and the hand-over run as in mi355x_solve_two_phase.  The main
 * tableau is never uploaded: its constraint rows ARE the artificial tableau's (:437-441), so every
 * shard keeps the main problem's columns among its slots (gathered on its own device, nothing moves
 * between devices; a shard left with artificial columns only keeps one as a dead slot that is
 * never priced), and its objective row -- main_objective_row: the last row of the main tableau,
 * main_cols doubles -- is re-eliminated over the basic rows on the devices (:444-451).
 * *main_out (also set on MI_UNBOUNDED) is the main tableau, solved by phase 2: read it with
 * mi355x_colpart_download (rows x main_cols), destroy it like any other handle.  `art` keeps the
 * artificial tableau as phase 1 and the drive-out pivots left it (download / destroy only: its
 * communicators now belong to *main_out).  One-process forms only (logical shards, or one shard
 * per visible device).  n_pivots[0] = phase 1 incl. drive-out pivots, n_pivots[1] = phase 2.
 * Returns what mi355x_solve_two_phase returns, or MI_UNSUPPORTED when the partition cannot follow
 * the reference bit for bit: an artificial tableau whose basis is not a set of unit columns, or a
 * drive-out pivot on a NEGATIVE element (it leaves -0.0 in basic columns, which compact shards do
 * not store) -- solve the caller's (untouched) tableaux with mi355x_solve_two_phase then. */
int  mi355x_colpart_solve_two_phase(mi355x_colpart *art, int64_t main_cols,
                                    const double *main_objective_row, int main_is_max,
                                    double fp_factor, int64_t *n_pivots, mi355x_colpart **main_out);
/* benchmarks: enqueue exactly n_pivots iterations (reset != 0: restart the pivot count), then
 * mi355x_colpart_sync waits, applies pending pivots and reports like mi355x_tab_sync */
int  mi355x_colpart_solve_async(mi355x_colpart *p, int is_max, double fp_factor, int64_t n_pivots,
                                int reset);
int  mi355x_colpart_sync(mi355x_colpart *p, int64_t *n_pivots);
/* mi355x_tab_cancel for mi355x_colpart_solve (any thread; the one-process forms -- logical shards or
 * one shard per visible device): MI_CANCELLED after the chunk of 64 .. 256 pivots in flight, every
 * shard swept.  One process per GPU: MI_UNSUPPORTED (the ranks would have to agree on the chunk, or
 * the others' collectives never complete) -- bound such solves with max_pivots. */
int  mi355x_colpart_cancel(mi355x_colpart *p);
/* read-back as mi355x_tab_download (any pointer may be NULL).  host_matrix (the whole logical
 * tableau) needs every shard in this process; basis, last row and last column are complete in
 * the one-process modes, and basis / last column also on every rank of the multi-process mode. */
int  mi355x_colpart_download(mi355x_colpart *p, double *host_matrix, int64_t *host_basis,
                             double *last_row, double *last_col);
int  mi355x_colpart_trace(mi355x_colpart *p, int64_t *entering_cols, int64_t *pivot_rows,
                          int64_t cap, int64_t *n);
void mi355x_colpart_destroy(mi355x_colpart *p);

/* ---- single-float tableaux (opt-in): the reference's single-float path ----------------------
 * Common Lisp reads 0.5 as a SINGLE-FLOAT, and the reference then solves in single-float arithmetic with
 * single-float thresholds (src/utils.lisp:84-124: fp<, fp>, fp= dispatch on float-contagion).  A mi355x_stab is
 * one tableau of IEEE binary32 entries in HBM and these entries are that path: every product is rounded, then
 * the difference is rounded (no FMA), division is true division, no double-precision intermediate anywhere;
 * thresholds are computed in float from fp_factor f (rounded to float first): pricing v < 0 - (f/8) eps_s,
 * ratio eligibility 0 + (f/2) eps_s < a, phase-1 feasibility |0 - obj| <= f eps_s, with
 * eps_s = single-float-epsilon = 2^-24 (1 + 2^-23).  Tie and NaN rules are those of mi355x_tab_*: the lowest
 * index of the strict extremum; a NaN key is no candidate except in column 0; a NaN quotient wins only as the
 * first eligible row.  Statuses, argument validation and MI_NO_DEVICE as for mi355x_tab_*.
 * A handle takes one of two forms when it is created (mi355x_stab_info): 2 = the whole solve loop in one
 * workgroup with the tableau in LDS (tableaux whose stored bytes plus scratch fit the budget), 1 = a select and
 * an update launch per pivot (any size).  Results never depend on the form. */
typedef struct mi355x_stab mi355x_stab;     /* one single-float tableau resident in HBM */
/* single-float-epsilon (src/utils.lisp:91), the float's value exactly, as a double */
double mi355x_epsilon_single(void);
/* Upload a build-tableau result (src/simplex.lisp:142-328) coerced to single-float: rows x cols, tightly packed. */
int  mi355x_stab_create(mi355x_stab **out, int64_t rows, int64_t cols, const float *matrix_rowmajor,
                        const int64_t *basis, int device);
/* find-entering-column (src/simplex.lisp:362-379): *col = column or -1 */
int  mi355x_stab_price(mi355x_stab *h, int is_max, double fp_factor, int64_t *col);
/* find-pivoting-row (src/simplex.lisp:382-389): *row = row or -1 */
int  mi355x_stab_ratio(mi355x_stab *h, int64_t entering_col, double fp_factor, int64_t *row);
/* n-pivot-row (src/simplex.lisp:337-359) */
int  mi355x_stab_pivot(mi355x_stab *h, int64_t entering_col, int64_t changing_row);
/* n-solve-tableau, single tableau (src/simplex.lisp:453-461).  max_pivots > 0 caps the pivots of this call
 * exactly (MI_MAX_PIVOTS); a solve continued call by call makes the pivots of one long call. */
int  mi355x_stab_solve(mi355x_stab *h, int is_max, double fp_factor, int64_t max_pivots, int64_t *n_pivots);
/* n-solve-tableau, two-phase branch (src/simplex.lisp:402-452): phase 1 on `art` (a min problem), (fp= 0
 * objective) with eps_s, the exact /= 0 tests and the drive-out pivots, the copy, the sequential objective-row
 * elimination in float, phase 2 on `main_tab`.  max_pivots > 0 caps the pivots of this call, both phases and the
 * drive-outs together; a call that ends with MI_MAX_PIVOTS is continued by the next call on the same pair.
 * pivots_out[0] = phase 1 + drive-outs, pivots_out[1] = phase 2, of this call. */
int  mi355x_stab_solve_two_phase(mi355x_stab *art, mi355x_stab *main_tab, int main_is_max, double fp_factor,
                                 int64_t max_pivots, int64_t *pivots_out);
/* tableau-matrix / basis-columns and what the read-back needs (src/simplex.lisp:74-120); any pointer may be NULL */
int  mi355x_stab_download(mi355x_stab *h, float *matrix, int64_t *basis, float *last_row, float *last_col);
/* (entering column, row) of the pivots made since the upload; *n = their number (the buffers hold the first cap) */
int  mi355x_stab_trace(mi355x_stab *h, int64_t *entering_cols, int64_t *rows, int64_t cap, int64_t *n);
/* shape, leading dimension in floats, the form taken (1 pair, 2 LDS), the LDS budget in bytes; any pointer may be NULL */
int  mi355x_stab_info(const mi355x_stab *h, int64_t *rows, int64_t *cols, int64_t *ld, int *form,
                      int64_t *lds_budget_bytes);
/* frees the handle (NULL: no-op); replaces the garbage collector's part in the reference */
void mi355x_stab_destroy(mi355x_stab *h);

/* ---- batches of single-float LPs (opt-in): one workgroup per member, the tableau in LDS ------
 * n_lps single-float tableaux of ONE shape.  One workgroup owns one member for its whole solve, with the member's
 * tableau, pivot row and column snapshot in LDS; both phases and everything between them run on the device.  The
 * contract is member by member: what a member ends with -- status, pivot counts, trace, basis and every tableau
 * entry, bit for bit (any NaN equal to any NaN) -- is what mi355x_stab_solve / mi355x_stab_solve_two_phase gives
 * that member alone under the same sequence of calls; one member's outcome never changes another's.
 * Per-member statuses: MI_OPTIMAL, MI_UNBOUNDED, MI_INFEASIBLE, MI_MAX_PIVOTS, MI_ART_NONZERO, MI_ART_STUCK, and
 * MI_RUNNING for a member a cancel left unfinished.  The calls return MI_OK, MI_CANCELLED or an error.
 * max_pivots (0: none) caps each member's pivots of THIS call; a further call carries every unfinished member on
 * from where it stopped (calls in chunks make the pivots of one long call) and does not touch a finished one. */
typedef struct mi355x_sbatch mi355x_sbatch;    /* (MI355X_SBATCH_TRACE_CAP, above: the pivots a member's trace holds) */
/* matrices: the members back to back, each as for mi355x_stab_create (rows x cols, tightly packed); basis: rows - 1
 * entries per member.  MI_UNSUPPORTED: the shape does not fit the LDS budget (its members go through mi355x_stab_*). */
int  mi355x_sbatch_create(mi355x_sbatch **out, int64_t n_lps, int64_t rows, int64_t cols, const float *matrices,
                          const int64_t *basis, int device);
/* n-solve-tableau (single phase) on every member; status[i], n_pivots[i] (pivots of this call) per member, either
 * may be NULL. */
int  mi355x_sbatch_solve(mi355x_sbatch *b, int is_max, double fp_factor, int64_t max_pivots, int32_t *status,
                         int64_t *n_pivots);
/* n-solve-tableau's two-phase branch per member: caps, drive-out counting and n_pivots (2 per member: phase 1 +
 * drive-outs, phase 2, of this call) follow mi355x_stab_solve_two_phase. */
int  mi355x_sbatch_solve_two_phase(mi355x_sbatch *art, mi355x_sbatch *main_b, int main_is_max, double fp_factor,
                                   int64_t max_pivots, int32_t *status, int64_t *n_pivots);
/* member lp_index as mi355x_stab_download gives it; any pointer may be NULL */
int  mi355x_sbatch_download(mi355x_sbatch *b, int64_t lp_index, float *matrix, int64_t *basis, float *last_row,
                            float *last_col);
/* member lp_index's pivots since the batch was created: *n their number, the first min(*n, cap, TRACE_CAP) copied */
int  mi355x_sbatch_trace(mi355x_sbatch *b, int64_t lp_index, int64_t *entering_cols, int64_t *rows, int64_t cap,
                         int64_t *n);
/* workgroup_threads: 256 or 1024, chosen from the shape at create; members_per_cu: workgroups of that size and LDS
 * footprint the runtime reports resident per compute unit.  Any pointer may be NULL. */
int  mi355x_sbatch_info(const mi355x_sbatch *b, int64_t *n_lps, int64_t *rows, int64_t *cols, int64_t *ld,
                        int *workgroup_threads, int64_t *lds_bytes_per_member, int *members_per_cu);
/* Any thread: the solve running on the batch -- or the next one -- stops between two rounds of launches with
 * MI_CANCELLED; the members hold whole pivots only and the next call carries them on. */
int  mi355x_sbatch_cancel(mi355x_sbatch *b);
void mi355x_sbatch_destroy(mi355x_sbatch *b);
/* The GLOBAL form (opt-in), for members beyond the LDS budget: one workgroup still owns one member for its whole
 * solve, but the member's tableau stays in device memory; LDS holds the pivot row and the column snapshot only.
 * Arguments, checks and their order are mi355x_sbatch_create's; the handle is an ordinary mi355x_sbatch, and
 * _solve, _solve_two_phase (both handles of ONE form, else MI_BAD_ARG), _download, _trace, _readback, _info,
 * _cancel and _destroy work on it under the same member-by-member contract.  Every shape the argument checks accept
 * is taken, small ones included; MI_UNSUPPORTED only where pivot row + column snapshot exceed the LDS budget (rows +
 * cols beyond about 39 000), and from _solve_two_phase where the step between the phases (two rows + a column of the
 * artificial shape) does.  Large members in small numbers are faster one by one through mi355x_stab_*: DESIGN 4.6k. */
int  mi355x_sbatch_create_global(mi355x_sbatch **out, int64_t n_lps, int64_t rows, int64_t cols, const float *matrices,
                                 const int64_t *basis, int device);
/* *form: 2 the members' tableaux in LDS, 3 the global form (continuing mi355x_stab_info: 1 pair, 2 LDS).  For form 3
 * mi355x_sbatch_info reports that form's workgroup, its dynamic LDS per member and its kernel's occupancy. */
int  mi355x_sbatch_form(const mi355x_sbatch *b, int *form);
/* The RAGGED form (opt-in): n_lps single-float tableaux of their OWN shapes and senses as one batch, for lists whose
 * members would otherwise each be alone in a batch of one shape.  One workgroup still owns one member for its whole
 * solve with the member's tableau in LDS, and the loop (n-solve-tableau, src/simplex.lisp:402-461) is the one of the
 * batch of one shape; a round is ONE launch at the largest member's LDS size (measured faster than a launch per
 * occupancy class; the classes stay behind mi355x_tune_set_sbatch_ragged_classes).
 * rows[q], cols[q]: member q's shape; is_max[q] != 0: a `max` problem (NULL: every member is `min`, as the artificial
 * batch of a pair is); matrices: the members' tight row-major tableaux one after the other; basis: their rows - 1
 * entries one after the other.  MI_BAD_ARG: a NULL array, a member with rows < 1, cols < 2 or beyond
 * mi355x_sbatch_create's limits; MI_UNSUPPORTED, naming the member: a member beyond the LDS budget
 * (mi355x_sbatch_create's rule and budget).  Nothing is left behind on a failure.
 * The handle is a mi355x_sbatch of form 4 (mi355x_sbatch_form): _solve, _solve_two_phase, _download, _trace, _cancel
 * and _destroy work on it under the same member-by-member contract.  The sense is each member's own: is_max /
 * main_is_max of a solve call must be -1 (anything else: MI_BAD_ARG).  A pair for _solve_two_phase is two form-4
 * handles of equal n_lps on one device with, per member, equal rows and art cols >= main cols (else MI_BAD_ARG).
 * mi355x_sbatch_info reports n_lps, rows = cols = ld = 0, the workgroup, the LARGEST member's lds_bytes_per_member
 * and the SMALLEST class (the largest members') as members_per_cu.  mi355x_sbatch_readback, which gathers planes of one shape, answers
 * MI_UNSUPPORTED on this form. */
int  mi355x_sbatch_create_ragged(mi355x_sbatch **out, int64_t n_lps, const int64_t *rows, const int64_t *cols,
                                 const int32_t *is_max, const float *matrices, const int64_t *basis, int device);
/* member lp_index of a ragged batch: its shape, leading dimension in floats, sense (1 max, 0 min) and the workgroups
 * resident per compute unit in the launch it goes in (its occupancy class, 1..4: by default the largest member's;
 * under the classes hook the member's own).  On forms 2 and 3: the batch's one
 * shape, *is_max = -1 (the sense is the solve call's) and members_per_cu.  Any pointer may be NULL. */
int  mi355x_sbatch_member_shape(const mi355x_sbatch *b, int64_t lp_index, int64_t *rows, int64_t *cols, int64_t *ld,
                                int32_t *is_max, int *occupancy_class);

/* ---- single-float branch-and-bound (opt-in): node LPs assembled on the device ------------------
 * simplex-solver (src/simplex.lisp:462-542) on a problem whose numbers Lisp reads as integers and single-floats.
 * The search, build-tableau of the base problem and the reading of a solution stay in the host language; the
 * library builds the node tableaux -- what build-tableau (src/simplex.lisp:142-328) makes of `node rows ++ problem
 * constraints` under Lisp's contagion, bit for bit -- as members of mi355x_sbatch handles, and gathers what
 * tableau-objective-value and tableau-variable read (src/simplex.lisp:74-107).
 * Base: the base problem's general-form main tableau in floats (rows x cols, tightly packed; a basis entry == cols
 * marks a row that needs an artificial variable, :254-265), ncv structural columns, nb rows of doubly-bounded
 * variables in front (:198-202), and per variable kind (0 positive, 1 negative, 2 signed), first column and offset
 * (:189-212).  col_int_sum[c]: the sum of the absolute values of the entries of column c that are INTEGERS in Lisp
 * (not floats with integer values), over the constraint rows -- the guard below rests on it.
 * Node rows: (var, sense 0 `<=` / 1 `>=`, bound), depth rows per node, newest first; they go between the nb bound
 * rows and the constraints (:214-221).  A row's right-hand side is float(bound) - offset (one rounding, the same
 * value as Lisp's bound - 1 * offset, :230-237); a negative one negates the row and flips its sense (:243-252),
 * leaving +0.0 in its other columns, as the d slack columns inserted into base rows hold +0.0.  Artificial columns
 * are dealt in decreasing row order (:257, :261, :296-300); the artificial objective row is per column the float
 * sum of the artificial rows in increasing row order from 0 (:302-316).
 * The guard: Lisp keeps integers exact among themselves in that sum, so a group is taken only when for every
 * column col_int_sum plus the node rows' own integer entries is at most 2^24 -- every integer partial sum is then
 * exact in a float.  Otherwise MI_UNSUPPORTED: the caller builds those nodes on the host (mi355x_sbatch_create).
 * MI_UNSUPPORTED as well for a shape beyond the batch's LDS budget (mi355x_sbatch_create's rule).
 * create_nodes: n_nodes nodes of ONE depth and ONE number of artificial rows (MI_BAD_ARG otherwise).  *out_main:
 * the main tableaux (rows + depth) x (cols + depth); *out_art: the artificial tableaux, (cols + depth + artificial
 * rows) columns, or NULL without artificial rows.  Every member is MI_RUNNING with an empty trace; the pair goes to
 * mi355x_sbatch_solve_two_phase, a main batch alone to mi355x_sbatch_solve.  The caller owns both handles. */
typedef struct mi355x_sbb_base mi355x_sbb_base;
int  mi355x_sbb_base_create(mi355x_sbb_base **out, int64_t rows, int64_t cols, const float *matrix, const int64_t *basis,
                            int64_t ncv, int64_t nb, int64_t n_vars, const int32_t *kind, const int64_t *col,
                            const float *offset, const double *col_int_sum, int device);
void mi355x_sbb_base_destroy(mi355x_sbb_base *base);
int  mi355x_sbatch_create_nodes(mi355x_sbatch **out_main, mi355x_sbatch **out_art, const mi355x_sbb_base *base,
                                int64_t n_nodes, int64_t depth, const int64_t *var, const int32_t *sense,
                                const int64_t *bound);
/* The same node batches in the GLOBAL form (opt-in; mi355x_sbatch_create_global's handles: form 3 of
 * mi355x_sbatch_form, its thread-count and launch-cap rules), for nodes beyond the LDS budget.  Arguments, checks and
 * their order, the guard and the tableaux -- node rows (src/simplex.lisp:214-221, :230-237), the flip (:243-252),
 * artificial columns (:257, :261, :296-300), the artificial objective row (:302-316) -- are mi355x_sbatch_create_nodes';
 * no handle is left behind on any failure.  The assembly is spread over a grid (a row pass per node, one write pass,
 * the artificial objective row behind it on one stream) and has NO row or depth limit of its own: every shape
 * mi355x_sbatch_create_global accepts is taken, small ones included; MI_UNSUPPORTED for the guard and where the pivot
 * row and column snapshot exceed the LDS budget (before anything is allocated). */
int  mi355x_sbatch_create_nodes_global(mi355x_sbatch **out_main, mi355x_sbatch **out_art, const mi355x_sbb_base *base,
                                       int64_t n_nodes, int64_t depth, const int64_t *var, const int32_t *sense,
                                       const int64_t *bound);
/* Per member the last column (rhs: rows values), the last row (obj_row: cols values) and the basis (rows - 1
 * entries), member-major: one gather kernel and one copy for the whole batch. */
int  mi355x_sbatch_readback(mi355x_sbatch *b, float *rhs, float *obj_row, int64_t *basis);

/* ---- single-float batches from problem rows (opt-in): build-tableau on the device ---------------
 * What mi355x_batch_create_lps is for doubles, in floats and under Lisp's int / single-float contagion: the members
 * arrive in column space, and the device writes what build-tableau (src/simplex.lisp:243-328) makes of each, bit
 * for bit, sign of zero included.  Member q: lps + q (m+1)(ncv+1) holds m rows of ncv coefficients and the
 * right-hand side, offsets already subtracted (:189-241), then the objective row (:270-283, signs applied, constant
 * last); sense is n_lps x m (0 `<=`, 1 `>=`, 2 `=`).
 * A row with right-hand side < 0.0f (false for -0.0 and NaN) is negated and its sense flipped (:243-252).  Lisp's
 * matrix starts as INTEGER zeros and (- 0) is 0: the slack columns of a negated row and its zero coefficients come
 * out +0.0 (mi355x_batch_create_lps leaves -0.0 there).  A ZERO IN A NEGATED ROW IS READ AS LISP'S INTEGER ZERO: a
 * single-float zero the user wrote there would be -0.0, and the caller keeps such members out.
 * Artificial columns are dealt in decreasing row order (:257, :261, :296-300); the artificial objective row is per
 * column the float sum of the artificial rows in increasing row order from 0 (:302-316).
 * The guard: Lisp keeps integers exact among themselves in that sum.  col_int_sum is n_lps x (ncv + 1) (NULL: all
 * zero): per member and column the sum of the absolute values of the entries Lisp holds as INTEGERS, over the
 * constraint rows.  An entry beyond 2^24 answers MI_UNSUPPORTED (the message names the member) and nothing is
 * allocated.  MI_UNSUPPORTED as well for a main or artificial shape beyond the batch's LDS budget
 * (mi355x_sbatch_create's rule).  MI_BAD_ARG, before any device is looked for: NULL out / lps / sense, n_lps, m or
 * ncv < 1, a sense outside 0..2, members that differ in their number of `=` rows or of artificial rows (the
 * message names the member).
 * *out_main: the main tableaux, (m + 1) x (ncv + slack columns + 1); *out_art: the artificial tableaux, with one
 * more column per artificial row, or NULL when no row is artificial.  Both are ordinary mi355x_sbatch handles in
 * the state mi355x_sbatch_create leaves: every member MI_RUNNING with an empty trace; the pair goes to
 * mi355x_sbatch_solve_two_phase, a main batch alone to mi355x_sbatch_solve.  The caller owns both handles. */
int  mi355x_sbatch_create_lps(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n_lps, int64_t m, int64_t ncv,
                              const float *lps, const int32_t *sense, const double *col_int_sum, int device);
/* The same batches in the GLOBAL form (opt-in; mi355x_sbatch_create_global's handles: form 3 of mi355x_sbatch_form,
 * its thread-count and launch-cap rules), for members beyond the LDS budget.  Arguments, checks and their order
 * (MI_BAD_ARG before any device is looked for), the guard and what is written -- the flip (src/simplex.lisp:243-252),
 * slack columns (:254-265), artificial columns (:257, :261, :296-300), the artificial objective row (:302-316), on
 * rows lowered by :189-241 and :270-283 -- are mi355x_sbatch_create_lps'; no handle is left behind on any failure.
 * The assembly is spread over a grid (a row pass per member, one write pass, the artificial objective row behind it
 * on one stream) and has NO row limit of its own: every shape mi355x_sbatch_create_global accepts is taken, small
 * ones included; MI_UNSUPPORTED for the guard and where the pivot row and column snapshot of the main or artificial
 * shape exceed the LDS budget (before anything is allocated). */
int  mi355x_sbatch_create_lps_global(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n_lps, int64_t m,
                                     int64_t ncv, const float *lps, const int32_t *sense, const double *col_int_sum,
                                     int device);

/* ---- ragged single-float batches built on the device (opt-in): rows and nodes of mixed shapes ----
 * mi355x_sbatch_create_ragged's form-4 handles, with the tableaux written by the device as for mi355x_sbatch_create_lps
 * and mi355x_sbatch_create_nodes -- the same rules, the same zero of a negated row, the same 2^24 guard, bit for bit --
 * but every member with a shape (and, from rows, a sense) of its own: one create for a list that those entries
 * would take one group at a time.  _solve, _solve_two_phase (sense -1), _download, _trace, _cancel, _destroy and
 * _member_shape work on the handles unchanged.
 * ALL OR NONE: either no member has artificial rows, and *out_art = NULL, or every member has at least one -- the counts
 * may differ from member to member -- and the result is a ragged pair.  A mixture is MI_BAD_ARG naming the first member
 * that differs; the caller splits its list.
 * create_lps_ragged: m[q], ncv[q], is_max[q] per member; lps: the members' (m + 1) x (ncv + 1) rows, tight, one after
 * the other; sense: their m senses one after the other; col_int_sum: their ncv + 1 sums one after the other, or NULL.
 * MI_BAD_ARG, before any device is looked for: a NULL array, m or ncv < 1, a sense outside 0..2, the mixture.
 * MI_UNSUPPORTED, naming the member, before anything is allocated: the guard, and a member whose tableau -- for a
 * member with artificial rows its ARTIFICIAL tableau -- is beyond the LDS budget (mi355x_sbatch_create's rule).  Any
 * later failure frees both handles. */
int  mi355x_sbatch_create_lps_ragged(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n_lps, const int64_t *m,
                                     const int64_t *ncv, const int32_t *is_max, const float *lps, const int32_t *sense,
                                     const double *col_int_sum, int device);
/* A form-4 handle carries its members' senses, and every node has the base problem's: say it once per base (0 min,
 * 1 max) before the first mi355x_sbatch_create_nodes_ragged (which answers MI_BAD_ARG without it).  The entries that
 * take the sense with the solve call do not read it.  The call writes into the base without a lock: make it before
 * the base is shared between threads, not beside a create on another thread. */
int  mi355x_sbb_base_set_sense(mi355x_sbb_base *base, int is_max);
/* create_nodes_ragged: depth[q] rows per node, the nodes' rows one after the other in var / sense / bound, newest row
 * first per node.  With a base that has artificial rows every node is two-phase.  The argument checks, the guard, the
 * assembly's LDS limit and the batch's budget are mi355x_sbatch_create_nodes', per node, the node named. */
int  mi355x_sbatch_create_nodes_ragged(mi355x_sbatch **out_main, mi355x_sbatch **out_art, const mi355x_sbb_base *base,
                                       int64_t n_nodes, const int64_t *depth, const int64_t *var, const int32_t *sense,
                                       const int64_t *bound);
/* mi355x_sbatch_readback for a ragged batch (form 4; MI_UNSUPPORTED on forms 2 and 3: call mi355x_sbatch_readback):
 * per member the last column, the last row and the basis into three concatenated planes -- member q's values at the
 * sums of rows, of cols and of rows - 1 over the members before it.  One gather launch and one copy. */
int  mi355x_sbatch_readback_ragged(mi355x_sbatch *b, float *rhs, float *obj_row, int64_t *basis);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_SIMPLEX_H */
