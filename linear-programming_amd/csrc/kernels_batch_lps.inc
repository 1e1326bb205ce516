// kernels_batch_lps.inc -- double-precision batches assembled in HBM from the members' problem rows
// (capi_batch_lps.inc drives them), and the light read-back of a batch.
//
// A member arrives in column space, as build-tableau holds it after src/simplex.lisp:189-241 and before
// :243: m rows of ncv structural coefficients and the right-hand side (offsets already subtracted), then the
// objective row of :270-283 (signs applied, constant last), with one sense per row.  These kernels write the
// member's main tableau, main basis, artificial tableau and artificial basis straight into batch allocations
// (padded `ld` layout of TabView, one LP per blockIdx.z / blockIdx.x), bit for bit what mi355x_build_tableau
// of the problem produces.  What is this file's:
//   * a row whose right-hand side is < 0.0 (false for -0.0 and NaN) is negated whole and its sense flipped
//     (:243-252) BEFORE its slack entry is written: its other slack columns carry -0.0;
//   * slack columns in row order for the rows that are not `=`, +1.0 (`<=`) or -1.0 (`>=`) (:254-265);
//   * the objective row is never negated, its slack columns hold 0.0;
//   * which rows are artificial and their ranks (k_blp_rows).
// Where the entries, the artificial columns, the bases and the artificial objective row go is
// kernels_assemble.inc's (k_assemble<BlpSrc>, k_art_objective).  The only arithmetic is negation and that sum.
#include "simplex_kernels.h"

constexpr int kBlpThreads = kAssembleThreads;

__device__ __forceinline__ int blp_row_word(const BatchLpsView &sp, int64_t z, int64_t i)
{
    return row_word(sp.L[(z * (sp.m + 1) + i) * (sp.ncv + 1) + sp.ncv] < 0.0, sp.sense[z * sp.m + i]);     // :243
}

// the rows source of k_assemble (kernels_assemble.inc); per row in scratch: ab[], the row's word, its slack column
// (-1: none)
struct BlpSrc {
    BatchLpsView sp;
    static constexpr int kWords = 3;
    struct Row { const double *Lr; int word; int64_t scol; };
    __host__ __device__ int64_t m() const { return sp.m; }
    __host__ __device__ int64_t num_cols() const { return sp.ncv + sp.n_slack + 1; }
    __device__ Row row(int64_t z, int64_t R, const int32_t *priv) const
    {
        const double *Lr = sp.L + (z * (sp.m + 1) + R) * (sp.ncv + 1);
        return R < sp.m ? Row{Lr, priv[R], priv[sp.m + R]} : Row{Lr, 0, -1};
    }
    __device__ double elem(const Row &r, int64_t C) const
    {
        const bool flip = r.word & 1;
        if (C < sp.ncv || C == num_cols() - 1) {
            const double x = r.Lr[C < sp.ncv ? C : sp.ncv];
            return flip ? -x : x;
        }
        if (C == r.scol) return (r.word >> 1) == 0 ? 1.0 : -1.0;
        return flip ? -0.0 : 0.0;
    }
};

// per member: flips, senses, slack columns, ab[] and both bases.  One workgroup per member; thread t owns the rows
// [t * chunk, (t + 1) * chunk) and the counts before them come from the other threads through LDS (the ranks
// deal_artificial_columns would find, without its serial walk over the rows).
__global__ __launch_bounds__(kBlpThreads) void k_blp_rows(TabView mt, TabView at, BatchLpsView sp, int32_t *scratch)
{
    __shared__ int32_t n_slack_of[kBlpThreads], n_art_of[kBlpThreads];
    const int64_t z = blockIdx.x, m = sp.m, cols = sp.ncv + sp.n_slack + 1;
    int32_t *ab = scratch + z * BlpSrc::kWords * m, *word = ab + m, *scol = word + m;
    const int64_t chunk = (m + kBlpThreads - 1) / kBlpThreads;
    const int64_t i0 = (int64_t)threadIdx.x * chunk < m ? (int64_t)threadIdx.x * chunk : m;
    const int64_t i1 = i0 + chunk < m ? i0 + chunk : m;
    int32_t ns = 0, na = 0;
    for (int64_t i = i0; i < i1; ++i) {
        const int op = blp_row_word(sp, z, i) >> 1;
        ns += op != 2;
        na += op != 0;
    }
    n_slack_of[threadIdx.x] = ns;
    n_art_of[threadIdx.x] = na;
    __syncthreads();
    int32_t slack_before = 0, art_through = 0, art_all = 0;
    for (int t = 0; t < kBlpThreads; ++t) {
        if (t < (int)threadIdx.x) { slack_before += n_slack_of[t]; art_through += n_art_of[t]; }
        art_all += n_art_of[t];
    }
    int64_t *mb = mt.basis + z * mt.zs_basis;
    int64_t *abasis = at.M ? at.basis + z * at.zs_basis : nullptr;
    for (int64_t i = i0; i < i1; ++i) {
        const int w = blp_row_word(sp, z, i), op = w >> 1;
        const int32_t sc = op != 2 ? (int32_t)(sp.ncv + slack_before) : -1;
        slack_before += op != 2;
        art_through += op != 0;
        // an artificial row's column: cols - 1 + the artificial rows with a greater index
        const int32_t a = op == 0 ? sc : (int32_t)(cols - 1) + (art_all - art_through);
        ab[i] = a; word[i] = w; scol[i] = sc;
        mb[i] = ab_main_basis(a, (int32_t)cols);
        if (abasis) abasis[i] = a;
    }
}

void launch_batch_lps_assemble(const TabView &mt, const TabView &at, const BatchLpsView &sp, int32_t *scratch, hipStream_t s)
{
    hipLaunchKernelGGL(k_blp_rows, dim3((unsigned)mt.n_lps), dim3(kBlpThreads), 0, s, mt, at, sp, scratch);
    launch_assemble(mt, at, BlpSrc{sp}, scratch, s);
}

// ---- the light read-back of a (dense) batch: per member the last row, the last column and the basis, gathered into
// one buffer of three planes -- n x cols doubles, n x rows doubles, n x (rows - 1) int64 -- for ONE copy to the host
__global__ __launch_bounds__(kBlpThreads) void k_batch_readback(TabView t, double *last_rows, double *last_cols, int64_t *bases)
{
    const int64_t z = blockIdx.x, rows = t.rows, cols = t.cols;
    const double *M = t.M + z * rows * t.ld;
    const int64_t *b = t.basis + z * t.zs_basis;
    for (int64_t C = threadIdx.x; C < cols; C += blockDim.x) last_rows[z * cols + C] = M[(rows - 1) * t.ld + C];
    for (int64_t R = threadIdx.x; R < rows; R += blockDim.x) last_cols[z * rows + R] = M[R * t.ld + cols - 1];
    for (int64_t R = threadIdx.x; R < rows - 1; R += blockDim.x) bases[z * (rows - 1) + R] = b[R];
}

void launch_batch_readback(const TabView &t, double *last_rows, double *last_cols, int64_t *bases, hipStream_t s)
{
    hipLaunchKernelGGL(k_batch_readback, dim3((unsigned)t.n_lps), dim3(kBlpThreads), 0, s, t, last_rows, last_cols, bases);
}
