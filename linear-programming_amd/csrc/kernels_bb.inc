// kernels_bb.inc -- branch-and-bound node tableaux assembled in HBM (host_bb.inc drives them).
//
// A node of the search is the problem with d extra rows `var <= bound` / `var >= bound` (newest
// first) placed between the rows build-tableau pushes for doubly-bounded variables and the
// problem's own rows (src/simplex.lisp:146, 198-202).  Its tableaux differ from the base problem's
// GENERAL-form tableau (built once on the host, uploaded once) only by those d rows, d slack
// columns inserted after the bound rows' slacks, and the artificial bookkeeping.  These kernels
// write every node's main tableau, main basis, artificial tableau and artificial basis straight
// into a batch allocation (padded `ld` layout of TabView, one LP per blockIdx.z / blockIdx.x),
// entry for entry what mi355x_build_tableau of the node problem produces:
//   * base rows copied, slack columns of the problem rows shifted by d; a base row that
//     build-tableau negated (rhs < 0, :243-252) carries -0.0 in the inserted columns too;
//   * a node row: rhs - coef * offset rounded as product then difference (no FMA), negated
//     whole when its rhs is negative (sense flipped), slack +1 (`<=`) or -1 (`>=`, artificial);
//   * main-basis entries of artificial rows = the node's num-cols;
//   * artificial columns dealt in DECREASING row order (push, :257, :261, :296-300);
//   * the artificial objective row summed over artificial rows in INCREASING row order from 0.0
//     (:302-316) -- recomputed, never updated.
#include "simplex_kernels.h"

// the d node rows of LP z: (rhs after `- coef * offset`, negated?) of node row k
__device__ __forceinline__ void bb_entry_row(const BBBaseView &b, const BBNodeRows &nr, int64_t z, int64_t k,
                                             int &kind, int64_t &col, double &rhs, bool &flip, int &op)
{
    const int64_t i = (nr.first + z) * nr.d + k;
    const int64_t v = nr.var[i];
    kind = b.kind[v]; col = b.vcol[v];
    rhs = nr.bound[i];
    if (kind != 2) rhs = __dsub_rn(rhs, __dmul_rn(1.0, b.voff[v]));     // coef 1, :230-237
    flip = rhs < 0.0;
    op = flip ? 1 - nr.sense[i] : nr.sense[i];
}

// entry (R, C) of LP z's main tableau
__device__ __forceinline__ double bb_main_elem(const BBBaseView &b, const BBNodeRows &nr, int64_t z, int64_t R,
                                               int64_t C)
{
    const int64_t d = nr.d, nb = b.nb, ncv = b.ncv, last = b.cols + d - 1;
    if (R >= nb && R < nb + d) {
        const int64_t k = R - nb;
        int kind, op; int64_t col; double rhs; bool flip;
        bb_entry_row(b, nr, z, k, kind, col, rhs, flip, op);
        double x = 0.0;
        if (C == last) x = rhs;
        else if (C == col) x = kind == 1 ? -1.0 : 1.0;
        else if (kind == 2 && C == col + 1) x = -1.0;
        if (flip) x = -x;
        if (C == ncv + nb + k) x = op == 0 ? 1.0 : -1.0;
        return x;
    }
    const int64_t r = R < nb ? R : R - d;                                  // base row (rows_b - 1: objective)
    const double *row = b.M + r * b.cols;
    if (C == last) return row[b.cols - 1];
    if (C < ncv + nb) return row[C];
    if (C < ncv + nb + d) return (r < b.rows - 1 && b.flip[r]) ? -0.0 : 0.0;
    return row[C - d];
}

// per LP: which rows are artificial, their rank (artificial column = num_cols - 1 + rank), both bases
__global__ __launch_bounds__(256) void k_bb_rows(TabView mt, TabView at, BBBaseView b, BBNodeRows nr, int32_t *scratch)
{
    const int64_t z = blockIdx.x;
    const int64_t d = nr.d, m = b.rows - 1 + d, num_cols = b.cols + d;
    int32_t *is_art = scratch + z * 2 * m, *rank = is_art + m;
    int64_t *mb = mt.basis + z * mt.zs_basis;
    for (int64_t R = threadIdx.x; R < m; R += blockDim.x) {
        int64_t bas;
        if (R >= b.nb && R < b.nb + d) {
            int kind, op; int64_t col; double rhs; bool flip;
            bb_entry_row(b, nr, z, R - b.nb, kind, col, rhs, flip, op);
            bas = op == 0 ? b.ncv + b.nb + (R - b.nb) : num_cols;
        } else {
            const int64_t bb = b.basis[R < b.nb ? R : R - d];
            bas = bb == b.cols ? num_cols : (bb >= b.ncv + b.nb ? bb + d : bb);
        }
        mb[R] = bas;
        is_art[R] = bas == num_cols;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t n = 0;
        for (int64_t R = m - 1; R >= 0; --R) { rank[R] = n; n += is_art[R]; }
    }
    __syncthreads();
    if (at.M) {
        int64_t *ab = at.basis + z * at.zs_basis;
        for (int64_t R = threadIdx.x; R < m; R += blockDim.x)
            ab[R] = is_art[R] ? num_cols - 1 + rank[R] : mb[R];
    }
}

// every entry of both tableaux but the artificial objective row; grid (column blocks, row blocks, LP)
__global__ __launch_bounds__(256) void k_bb_assemble(TabView mt, TabView at, BBBaseView b, BBNodeRows nr,
                                                     const int32_t *scratch)
{
    const int64_t z = blockIdx.z;
    const int64_t d = nr.d, m = b.rows - 1 + d, num_cols = b.cols + d;
    const int32_t *is_art = scratch + z * 2 * m, *rank = is_art + m;
    double *M = mt.M + z * mt.zs_M;
    double *A = at.M ? at.M + z * at.zs_M : nullptr;
    const int64_t nac = at.M ? at.cols : 0;
    for (int64_t R = blockIdx.y; R <= m; R += gridDim.y) {
        for (int64_t C = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; C < mt.ld; C += (int64_t)gridDim.x * blockDim.x)
            M[R * mt.ld + C] = C < num_cols ? bb_main_elem(b, nr, z, R, C) : 0.0;
        if (!A || R == m) continue;
        for (int64_t C = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; C < at.ld; C += (int64_t)gridDim.x * blockDim.x) {
            double x = 0.0;
            if (C < num_cols - 1) x = bb_main_elem(b, nr, z, R, C);
            else if (C == nac - 1) x = bb_main_elem(b, nr, z, R, num_cols - 1);
            else if (C < nac - 1) x = (is_art[R] && C - (num_cols - 1) == rank[R]) ? 1.0 : 0.0;
            A[R * at.ld + C] = x;
        }
    }
}

// the artificial objective row: column sums over artificial rows, increasing row order, from 0.0
__global__ __launch_bounds__(256) void k_bb_art_objective(TabView at, BBBaseView b, BBNodeRows nr, const int32_t *scratch)
{
    const int64_t z = blockIdx.z;
    const int64_t d = nr.d, m = b.rows - 1 + d, num_cols = b.cols + d, nac = at.cols;
    const int32_t *is_art = scratch + z * 2 * m;
    double *A = at.M + z * at.zs_M;
    for (int64_t C = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; C < at.ld; C += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        if (C < num_cols - 1 || C == nac - 1)
            for (int64_t R = 0; R < m; ++R)
                if (is_art[R]) s = __dadd_rn(s, A[R * at.ld + C]);
        A[m * at.ld + C] = s;
    }
}

void launch_bb_assemble(const TabView &mt, const TabView &at, const BBBaseView &b, const BBNodeRows &nr,
                        int32_t *scratch, hipStream_t s)
{
    const unsigned n = (unsigned)mt.n_lps;
    const int64_t rows = mt.rows;
    hipLaunchKernelGGL(k_bb_rows, dim3(n), dim3(256), 0, s, mt, at, b, nr, scratch);
    const int64_t ld = at.M && at.ld > mt.ld ? at.ld : mt.ld;
    unsigned bx = (unsigned)((ld + 255) / 256); if (bx > 16) bx = 16;
    unsigned by = (unsigned)(rows < 1024 ? rows : 1024);
    hipLaunchKernelGGL(k_bb_assemble, dim3(bx, by, n), dim3(256), 0, s, mt, at, b, nr, (const int32_t *)scratch);
    if (at.M) {
        unsigned cx = (unsigned)((at.ld + 255) / 256);
        hipLaunchKernelGGL(k_bb_art_objective, dim3(cx, 1, n), dim3(256), 0, s, at, b, nr, (const int32_t *)scratch);
    }
}
