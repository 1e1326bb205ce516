// kernels_single_global.inc -- the GLOBAL form of a batch of single-float tableaux: one workgroup owns one member for
// its whole solve, as in kernels_single_batch.inc, but the member's tableau stays in HBM; LDS holds only the scaled
// pivot row, the entering-column snapshot and the reductions' scratch.  For members beyond the LDS budget.
// The loop is s_solve_in_lds with the LDS tableau replaced by t.M (row length t.ld): the third loop around the ONE copy
// of the selection code (s_block_price, s_block_gather_ratio, s_block_scale_row of kernels_single.inc), so a member
// ends with exactly what the select / update pair gives it alone.  The arithmetic is k_s_update's.
// No double appears in this file; -ffp-contract=off (a product is rounded, then the difference is rounded).
//
// Ordering.  A pivot's update writes rows that other waves of the workgroup read in the next pricing and the next
// column gather, so every pivot ends with a __syncthreads() after the update's stores; the snapshot and prow are
// complete, behind a barrier, before the update's first store (nothing reads the old pivot row or the old column
// from HBM after that barrier).  Plain loads and stores: the waves of a workgroup share one CU and its L1, so
// workgroup scope -- what __syncthreads() gives -- suffices.  No other workgroup ever touches a member: no agent-scope
// fence, no flag and no spin, so nothing here can wait for a workgroup that is not resident.
// Part of simplex_kernels.hip (ONE translation unit: included there, after kernels_single_batch.inc, inside namespace mi355x).

// rows of quads in flight per thread before the first use (as k_s_update keeps U rows in flight)
constexpr int kSgUnroll = 4;

// One workgroup of THREADS threads runs n-solve-tableau (src/simplex.lisp:453-461) on the tableau t.M in HBM.  Dynamic
// LDS: the pivot row (cols rounded up to a quad), then the column snapshot (rows rounded up to a quad).  At most `cap`
// pivots per launch; max_pivots is honoured exactly (k_s_select's order of tests).  The columns [cols rounded up to
// a quad, ld) of a row are never read and never written.
template <int THREADS>
__device__ __forceinline__ void s_solve_in_hbm(const SView &t, float sgn, float price_tol, float ratio_thr, int cap)
{
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    __shared__ SScratch sc;
    Ctl *ctl = t.ctl;
    const Ctl c0 = *ctl;
    if (c0.status != kRunning) return;
    const int rows = (int)t.rows, cols = (int)t.cols, vc = cols - 1;
    const int ldlq = (cols + 3) >> 2, ldl = 4 * ldlq;         // the quads / floats of a row that hold columns
    const int64_t ld = t.ld;
    float *M    = t.M;
    float *prow = s_lds;
    float *col  = prow + ldl;
    char *Mb = reinterpret_cast<char *>(M);
    const vec4f *P4 = reinterpret_cast<const vec4f *>(prow);
    // A member of this form is smaller than 2^32 bytes (sgbatch_available: rows + cols fit the LDS budget), so the
    // update addresses it with 32-bit byte offsets from the member's base.
    const int nq = rows * ldlq;                               // quads the update walks
    const unsigned row_bytes = (unsigned)ld * 4u;
    // thread's walk over the quads: (row, quad of the row) advances by THREADS quads per step
    const int step_r = THREADS / ldlq, step_q = THREADS % ldlq;
    const unsigned step_bytes = (unsigned)step_r * row_bytes + (unsigned)step_q * 16u;
    const unsigned wrap_bytes = row_bytes - (unsigned)ldlq * 16u;
    int32_t status = kRunning;
    int64_t n = c0.n_pivots, trace_n = c0.trace_n, last_ec = c0.ec, last_cr = c0.cr;
    for (int k = 0; ; ++k) {
        // The base the selection code sees is opaque to the compiler in every pivot: hoisted out of the loop, the
        // 64-bit addresses of its kBatch loads in flight would stay live across the update (and spill at 1024 threads).
        float *Mk = M;
        asm volatile("" : "+s"(Mk));
        const SCand e = s_block_price<THREADS>(Mk + (int64_t)(rows - 1) * ld, vc, sgn, &sc);
        if (s_price_says_optimal(e, price_tol)) { status = 0; break; }                 // MI_OPTIMAL
        if (c0.max_pivots > 0 && n >= c0.max_pivots) { status = 3; break; }            // MI_MAX_PIVOTS
        if (k >= cap) break;                                   // the launch's bound: still running
        const SCand q = s_block_gather_ratio<THREADS>(Mk, ld, rows, vc, e.i, col, ratio_thr, &sc);
        if (q.i < 0) { status = 1; break; }                    // MI_UNBOUNDED
        const int cr = q.i;
        s_block_scale_row<THREADS>(Mk + (int64_t)cr * ld, prow, ldlq, cols, __uint_as_float(q.s));
        __syncthreads();                                       // col and prow are complete: the first store comes below
        {
            int r = (int)threadIdx.x / ldlq, qd = (int)threadIdx.x % ldlq;
            unsigned off = (unsigned)r * row_bytes + (unsigned)qd * 16u;       // byte offset of quad (r, qd) in the member
            for (int base = threadIdx.x; base < nq; base += kSgUnroll * THREADS) {
                vec4f v[kSgUnroll];
                int rr[kSgUnroll], qq[kSgUnroll];
                unsigned oo[kSgUnroll];
#pragma unroll
                for (int u = 0; u < kSgUnroll; ++u) {          // kSgUnroll 16-byte loads in flight
                    rr[u] = r; qq[u] = qd; oo[u] = off;
                    if (base + u * THREADS < nq) v[u] = *reinterpret_cast<const vec4f *>(Mb + off);
                    else { v[u].x = 0.0f; v[u].y = 0.0f; v[u].z = 0.0f; v[u].w = 0.0f; }
                    r += step_r; qd += step_q; off += step_bytes;
                    if (qd >= ldlq) { qd -= ldlq; ++r; off += wrap_bytes; }
                }
#pragma unroll
                for (int u = 0; u < kSgUnroll; ++u) {
                    if (base + u * THREADS < nq) {
                        const vec4f p = P4[qq[u]];
                        const float s = col[rr[u]];
                        const float m0 = s * p.x, m1 = s * p.y, m2 = s * p.z, m3 = s * p.w;     // rounded products
                        vec4f o;
                        o.x = v[u].x - m0;                     // rounded differences
                        o.y = v[u].y - m1;
                        o.z = v[u].z - m2;
                        o.w = v[u].w - m3;
                        if (rr[u] == cr) o = p;                // the pivot row itself
                        *reinterpret_cast<vec4f *>(Mb + oo[u]) = o;
                    }
                }
            }
        }
        if (threadIdx.x == 0) {
            if (rows > 1) t.basis[cr] = e.i;                   // src/simplex.lisp:358
            if (t.trace_ec && trace_n < t.trace_cap) { t.trace_ec[trace_n] = e.i; t.trace_cr[trace_n] = cr; }
        }
        ++n; ++trace_n; last_ec = e.i; last_cr = cr;
        __syncthreads();                                       // the update's stores, before the next pricing and gather
    }
    if (threadIdx.x == 0) {
        ctl->status = status; ctl->n_pivots = n; ctl->trace_n = trace_n; ctl->ec = last_ec; ctl->cr = last_cr;
    }
}

// the global form's Loop of k_sb_solve (kernels_single_batch.inc): k_sb_solve<THREADS, SbView, SolveInHbm> is what the
// docs call k_sg_solve
struct SolveInHbm {
    template <int THREADS>
    static __device__ __forceinline__ void run(const SView &t, float sgn, float price_tol, float ratio_thr, int cap)
    {
        s_solve_in_hbm<THREADS>(t, sgn, price_tol, ratio_thr, cap);
    }
};

// ------------------------------------------------------------------ host-side launchers
// dynamic LDS of k_sg_solve: pivot row + column snapshot
size_t sgbatch_lds_bytes(const SbView &b)
{
    const size_t ldl = (size_t)((b.cols + 3) / 4 * 4), rp = (size_t)((b.rows + 3) / 4 * 4);
    return (ldl + rp) * sizeof(float);
}
// dynamic LDS of k_sb_between for a pair whose artificial batch is `art`: flags + row + column snapshot
size_t sgbatch_between_lds_bytes(const SbView &art)
{
    const size_t ldl = (size_t)((art.cols + 3) / 4 * 4), rp = (size_t)((art.rows + 3) / 4 * 4);
    return (2 * ldl + rp) * sizeof(float);
}
// The ONE rule: which workgroup a global-form batch takes.  Measured (profiles/sbatch_global_rate.txt, DESIGN 4.6k):
// 256 threads win by 4-9 % at every member count at 161 KiB stored (98 x 300); at 274 KiB (128 x 384) 1024 threads
// draw at 256 members and win by 10 % at 1024, and from 458 KiB up they win at every count, by up to 93 %.
int sgbatch_threads_for(int64_t rows, int64_t ld)
{
    return rows * ld * (int64_t)sizeof(float) < kSgbatchBytes1024 ? 256 : 1024;
}
// The launch cap of a global-form handle: a launch walks at most the bytes the LDS form's longest launch walks
// (kSingleLaunchCap pivots on a member that fills the budget), never fewer than one pivot.
int sgbatch_launch_cap_for(int64_t rows, int64_t ld)
{
    const double stored = (double)rows * (double)ld * sizeof(float);
    const double cap = (double)kSingleLaunchCap * (double)kSingleLdsBudget / stored;
    return cap >= (double)kSingleLaunchCap ? kSingleLaunchCap : cap < 1.0 ? 1 : (int)cap;
}
// false: pivot row + column snapshot do not fit the budget, or the attributes could not be raised
bool sgbatch_available(const SbView &b, int threads, int *members_per_cu)
{
    const size_t lds = sgbatch_lds_bytes(b);
    if (lds > kSingleLdsBudget) return false;
    if ((uint64_t)b.rows * (uint64_t)b.ld * sizeof(float) >= (1ull << 32)) return false;   // (implied by the budget: k_sg_solve's offsets)
    return sb_kernel_attributes<SbView, SolveInHbm>(threads, true, lds, members_per_cu);
}
void launch_sg_solve(const SbView &b, int threads, int is_max, double f, int cap, const int32_t *gate, hipStream_t s)
{
    sb_solve_launch<SbView, SolveInHbm>(b, nullptr, b.n_lps, sgbatch_lds_bytes(b), threads, is_max, f, cap, gate, s);
}
// k_sb_between for a pair of global-form batches: the body is the LDS form's, the LDS what it uses
void launch_sg_between(const SbView &art, const SbView &mb, int threads, int32_t *phase, double f, int64_t max_pivots, hipStream_t s)
{
    sb_between_launch(art, mb, nullptr, art.n_lps, sgbatch_between_lds_bytes(art), threads, phase, f, max_pivots, s);
}
