// kernels_bb.inc -- branch-and-bound node tableaux assembled in HBM (host_bb.inc drives them).
//
// A node of the search is the problem with d extra rows `var <= bound` / `var >= bound` (newest
// first) placed between the rows build-tableau pushes for doubly-bounded variables and the
// problem's own rows (src/simplex.lisp:146, 198-202).  Its tableaux differ from the base problem's
// GENERAL-form tableau (built once on the host, uploaded once) only by those d rows, d slack
// columns inserted after the bound rows' slacks, and the artificial bookkeeping.  These kernels
// write every node's main tableau, main basis, artificial tableau and artificial basis straight
// into a batch allocation (padded `ld` layout of TabView, one LP per blockIdx.z / blockIdx.x),
// entry for entry what mi355x_build_tableau of the node problem produces.  What is this file's:
//   * base rows copied, slack columns of the problem rows shifted by d; a base row that
//     build-tableau negated (rhs < 0, :243-252) carries -0.0 in the inserted columns too;
//   * a node row: rhs - coef * offset rounded as product then difference (no FMA), negated
//     whole when its rhs is negative (sense flipped), slack +1 (`<=`) or -1 (`>=`, artificial);
//   * which rows are artificial (k_bb_rows).
// Where the entries, the artificial columns, the bases and the artificial objective row go is
// kernels_assemble.inc's (k_assemble<BbSrc>, k_art_objective).
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
    op = row_word(flip, nr.sense[i]) >> 1;
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


// the node source of k_assemble (kernels_assemble.inc): one scratch word per row, ab[]
struct BbSrc {
    BBBaseView b;
    BBNodeRows nr;
    static constexpr int kWords = 1;
    struct Row { int64_t z, R; };
    __host__ __device__ int64_t m() const { return b.rows - 1 + nr.d; }
    __host__ __device__ int64_t num_cols() const { return b.cols + nr.d; }
    __device__ Row row(int64_t z, int64_t R, const int32_t *) const { return Row{z, R}; }
    __device__ double elem(const Row &r, int64_t C) const { return bb_main_elem(b, nr, r.z, r.R, C); }
};

// per LP: ab[] (which rows are artificial and the columns dealt to them) and both bases
__global__ __launch_bounds__(kAssembleThreads) void k_bb_rows(TabView mt, TabView at, BBBaseView b, BBNodeRows nr, int32_t *scratch)
{
    const int64_t z = blockIdx.x;
    const int64_t d = nr.d, m = b.rows - 1 + d, num_cols = b.cols + d;
    int32_t *ab = scratch + z * BbSrc::kWords * m;
    for (int64_t R = threadIdx.x; R < m; R += blockDim.x) {
        int64_t bas;
        if (R >= b.nb && R < b.nb + d) {
            int kind, op; int64_t col; double rhs; bool flip;
            bb_entry_row(b, nr, z, R - b.nb, kind, col, rhs, flip, op);
            bas = op == 0 ? b.ncv + R : num_cols;
        } else {
            const int64_t bb = b.basis[R < b.nb ? R : R - d];
            bas = bb == b.cols ? num_cols : (bb >= b.ncv + b.nb ? bb + d : bb);
        }
        ab[R] = (int32_t)bas;
    }
    __syncthreads();
    if (threadIdx.x == 0) deal_artificial_columns(ab, (int)m, (int32_t)num_cols);
    __syncthreads();
    int64_t *mb = mt.basis + z * mt.zs_basis;
    int64_t *abasis = at.M ? at.basis + z * at.zs_basis : nullptr;
    for (int64_t R = threadIdx.x; R < m; R += blockDim.x) {
        mb[R] = ab_main_basis(ab[R], (int32_t)num_cols);
        if (abasis) abasis[R] = ab[R];
    }
}

void launch_node_assemble(const TabView &mt, const TabView &at, const BBBaseView &b, const BBNodeRows &nr,
                          int32_t *scratch, hipStream_t s)
{
    hipLaunchKernelGGL(k_bb_rows, dim3((unsigned)mt.n_lps), dim3(kAssembleThreads), 0, s, mt, at, b, nr, scratch);
    launch_assemble(mt, at, BbSrc{b, nr}, scratch, s);
}
