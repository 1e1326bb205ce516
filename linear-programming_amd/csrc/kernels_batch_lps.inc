// kernels_batch_lps.inc -- double-precision batches assembled in HBM from the members' problem rows
// (capi_batch_lps.inc drives them), and the light read-back of a batch.
//
// A member arrives in column space, as build-tableau holds it after src/simplex.lisp:189-241 and before
// :243: m rows of ncv structural coefficients and the right-hand side (offsets already subtracted), then the
// objective row of :270-283 (signs applied, constant last), with one sense per row.  These kernels write the
// member's main tableau, main basis, artificial tableau and artificial basis straight into batch allocations
// (padded `ld` layout of TabView, one LP per blockIdx.z / blockIdx.x), bit for bit what mi355x_build_tableau
// of the problem produces:
//   * a row whose right-hand side is < 0.0 (false for -0.0 and NaN) is negated whole and its sense flipped
//     (:243-252) BEFORE its slack entry is written: its other slack columns carry -0.0;
//   * slack columns in row order for the rows that are not `=`, +1.0 (`<=`) or -1.0 (`>=`) (:254-265);
//   * the objective row is never negated, its slack columns hold 0.0;
//   * main-basis entries of artificial rows (`>=`, `=` after the flip) = the member's num-cols;
//   * artificial columns dealt in DECREASING row order (push, :257, :261, :296-300), +0.0 elsewhere;
//   * the artificial objective row summed over artificial rows in INCREASING row order from +0.0, one rounded
//     addition per row (:302-316).
// The only arithmetic is negation and that sum.
#include "simplex_kernels.h"

// per row of a member, in scratch: meta = flip | op << 1, the slack column (-1: none), the artificial rank
constexpr int kBlpThreads = 256;

__device__ __forceinline__ int blp_row_meta(const BatchLpsView &sp, int64_t z, int64_t i)
{
    const bool flip = sp.L[(z * (sp.m + 1) + i) * (sp.ncv + 1) + sp.ncv] < 0.0;     // :243
    const int s = sp.sense[z * sp.m + i];
    const int op = s == 2 ? 2 : (flip ? 1 - s : s);
    return (flip ? 1 : 0) | (op << 1);
}

// entry (R, C) of member z's main tableau, C < cols; meta / scol are row R's (R == m: 0 / -1)
__device__ __forceinline__ double blp_main_elem(const BatchLpsView &sp, const double *Lr, int meta, int64_t scol,
                                                int64_t C, int64_t cols)
{
    const bool flip = meta & 1;
    if (C < sp.ncv || C == cols - 1) {
        const double x = Lr[C < sp.ncv ? C : sp.ncv];
        return flip ? -x : x;
    }
    if (C == scol) return (meta >> 1) == 0 ? 1.0 : -1.0;
    return flip ? -0.0 : 0.0;
}

// per member: flips, senses, slack columns, artificial ranks and both bases.  One workgroup per member; thread t
// owns the rows [t * chunk, (t + 1) * chunk) and the counts before them come from the other threads through LDS.
__global__ __launch_bounds__(kBlpThreads) void k_blp_rows(TabView mt, TabView at, BatchLpsView sp, int32_t *scratch)
{
    __shared__ int32_t n_slack_of[kBlpThreads], n_art_of[kBlpThreads];
    const int64_t z = blockIdx.x, m = sp.m, cols = sp.ncv + sp.n_slack + 1;
    int32_t *meta = scratch + z * 3 * m, *scol = meta + m, *rank = scol + m;
    const int64_t chunk = (m + kBlpThreads - 1) / kBlpThreads;
    const int64_t i0 = (int64_t)threadIdx.x * chunk < m ? (int64_t)threadIdx.x * chunk : m;
    const int64_t i1 = i0 + chunk < m ? i0 + chunk : m;
    int32_t ns = 0, na = 0;
    for (int64_t i = i0; i < i1; ++i) {
        const int op = blp_row_meta(sp, z, i) >> 1;
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
    int64_t *ab = at.M ? at.basis + z * at.zs_basis : nullptr;
    for (int64_t i = i0; i < i1; ++i) {
        const int mt_i = blp_row_meta(sp, z, i), op = mt_i >> 1;
        const int32_t sc = op != 2 ? (int32_t)(sp.ncv + slack_before) : -1;
        slack_before += op != 2;
        art_through += op != 0;
        const int32_t rk = art_all - art_through;                          // artificial rows with a greater index
        meta[i] = mt_i; scol[i] = sc; rank[i] = rk;
        mb[i] = op == 0 ? sc : cols;
        if (ab) ab[i] = op == 0 ? sc : cols - 1 + rk;
    }
}

// every entry of both tableaux but the artificial objective row; grid (column blocks, row blocks, member)
__global__ __launch_bounds__(kBlpThreads) void k_blp_assemble(TabView mt, TabView at, BatchLpsView sp, const int32_t *scratch)
{
    const int64_t z = blockIdx.z, m = sp.m, cols = sp.ncv + sp.n_slack + 1;
    const int32_t *meta = scratch + z * 3 * m, *scol = meta + m, *rank = scol + m;
    double *M = mt.M + z * mt.zs_M;
    double *A = at.M ? at.M + z * at.zs_M : nullptr;
    const int64_t nac = at.M ? at.cols : 0;
    const int64_t c0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, cstep = (int64_t)gridDim.x * blockDim.x;
    for (int64_t R = blockIdx.y; R <= m; R += gridDim.y) {
        const double *Lr = sp.L + (z * (m + 1) + R) * (sp.ncv + 1);
        const int mt_r = R < m ? meta[R] : 0;
        const int64_t sc = R < m ? scol[R] : -1;
        for (int64_t C = c0; C < mt.ld; C += cstep)
            M[R * mt.ld + C] = C < cols ? blp_main_elem(sp, Lr, mt_r, sc, C, cols) : 0.0;
        if (!A || R == m) continue;
        const int64_t acol = (mt_r >> 1) != 0 ? cols - 1 + rank[R] : -1;
        for (int64_t C = c0; C < at.ld; C += cstep) {
            double x = 0.0;
            if (C < cols - 1) x = blp_main_elem(sp, Lr, mt_r, sc, C, cols);
            else if (C == nac - 1) x = blp_main_elem(sp, Lr, mt_r, sc, cols - 1, cols);
            else if (C == acol) x = 1.0;
            A[R * at.ld + C] = x;
        }
    }
}

// the artificial objective row: column sums over artificial rows, increasing row order, from +0.0
__global__ __launch_bounds__(kBlpThreads) void k_blp_art_objective(TabView at, BatchLpsView sp, const int32_t *scratch)
{
    const int64_t z = blockIdx.z, m = sp.m, cols = sp.ncv + sp.n_slack + 1, nac = at.cols;
    const int32_t *meta = scratch + z * 3 * m, *scol = meta + m;
    const double *L = sp.L + z * (m + 1) * (sp.ncv + 1);
    double *A = at.M + z * at.zs_M;
    for (int64_t C = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; C < at.ld; C += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        if (C < cols - 1 || C == nac - 1) {
            const int64_t Cm = C < cols - 1 ? C : cols - 1;
            for (int64_t R = 0; R < m; ++R) {
                const int mt_r = meta[R];
                if ((mt_r >> 1) != 0) s = __dadd_rn(s, blp_main_elem(sp, L + R * (sp.ncv + 1), mt_r, scol[R], Cm, cols));
            }
        }
        A[m * at.ld + C] = s;
    }
}

void launch_batch_lps_assemble(const TabView &mt, const TabView &at, const BatchLpsView &sp, int32_t *scratch, hipStream_t s)
{
    const unsigned n = (unsigned)mt.n_lps;
    const int64_t rows = mt.rows;
    hipLaunchKernelGGL(k_blp_rows, dim3(n), dim3(kBlpThreads), 0, s, mt, at, sp, scratch);
    const int64_t ld = at.M && at.ld > mt.ld ? at.ld : mt.ld;
    unsigned bx = (unsigned)((ld + kBlpThreads - 1) / kBlpThreads); if (bx > 16) bx = 16;
    unsigned by = (unsigned)(rows < 1024 ? rows : 1024);
    // large batches: a workgroup takes several rows instead of the grid growing past a quarter of a million workgroups
    while (by > 1 && (uint64_t)bx * by * n > (1u << 18)) by = (by + 1) / 2;
    hipLaunchKernelGGL(k_blp_assemble, dim3(bx, by, n), dim3(kBlpThreads), 0, s, mt, at, sp, (const int32_t *)scratch);
    if (at.M) {
        unsigned cx = (unsigned)((at.ld + kBlpThreads - 1) / kBlpThreads);
        hipLaunchKernelGGL(k_blp_art_objective, dim3(cx, 1, n), dim3(kBlpThreads), 0, s, at, sp, (const int32_t *)scratch);
    }
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
