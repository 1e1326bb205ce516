// kernels_assemble.inc -- build-tableau's layout (src/simplex.lisp:243-328), ONE copy for every device-side
// assembly.  Part of simplex_kernels.hip (included there before kernels_bb.inc).  A member source (problem rows,
// or a base tableau plus node rows) classifies its constraint rows into ab[] -- per row its artificial-basis entry,
// the convention of simplex_kernels.h: row_word, deal_artificial_columns, ab_artificial, ab_main_basis -- and
// supplies the entries of the main tableau; where they go is decided here:
//   * the main tableau is the source's entries, its padding +0.0;
//   * the artificial tableau repeats the main one's structural and slack columns, then one column per artificial
//     row, 1.0 in that row (dealt in DECREASING row order: ab[]), +0.0 elsewhere, then the right-hand side;
//   * its objective row is the sum of the artificial rows in INCREASING row order from +0.0, one rounded addition
//     per row (:302-316), over the structural and slack columns and the right-hand side, +0.0 elsewhere;
//   * the main basis of an artificial row is the member's num-cols, the artificial basis is ab[] itself.
// The HBM family has ab[] in a per-member scratch plane and spreads a member over a grid: doubles (k_assemble<Src> here,
// sources in kernels_bb.inc and kernels_batch_lps.inc) and floats (k_sga_write<Src> of
// kernels_single_assemble_global.inc, the global form of a single-float batch, with quad stores and a grid of its own).
// The LDS family (floats, kernels_single_bb.inc and kernels_single_lps.inc) has ab[] in LDS, one workgroup per member.
// All three write passes state the artificial tableau's entry and its objective row's columns through art_entry and
// art_objective_column below.  The exact kernels share only the rules of simplex_kernels.h: their entries carry a
// scale and an overflow status of their own.

constexpr int kAssembleThreads = 256;

// ---- the artificial tableau, ONE statement for every write pass (T: the scalar, I: the pass's index type).
// Entry C of constraint row R, whose ab[] entry is acol (a slack column is < num_cols - 1); main(c): entry c <
// num_cols of that row of the main tableau; nac: the artificial tableau's columns.
template <class T, class I, class Main>
__device__ __forceinline__ T art_entry(I C, I num_cols, I nac, I acol, Main main)
{
    if (C < num_cols - 1) return main(C);
    if (C == nac - 1) return main(num_cols - 1);
    return C == acol ? T(1) : T(0);
}
// the columns of the artificial objective row that are a sum over the artificial rows (+0.0 elsewhere)
template <class I>
__device__ __forceinline__ bool art_objective_column(I C, I num_cols, I nac) { return C < num_cols - 1 || C == nac - 1; }

// ---- HBM family.  A source Src is passed by value and has
//   kWords                      int32 words of scratch per constraint row: plane 0 is ab[], written by the source's
//                               rows kernel; the planes behind it are the source's own
//   m(), num_cols()             constraint rows and columns of the main tableau
//   row(z, R, priv)             what elem needs of row R <= m of member z (priv: the source's planes of member z)
//   elem(row, C)                entry C < num_cols of that row of the main tableau

// every entry of both tableaux but the artificial objective row; grid (column blocks, row blocks, member)
template <class Src>
__global__ __launch_bounds__(kAssembleThreads) void k_assemble(TabView mt, TabView at, Src src, const int32_t *scratch)
{
    const int64_t z = blockIdx.z, m = src.m(), num_cols = src.num_cols();
    const int32_t *ab = scratch + z * Src::kWords * m;
    double *M = mt.M + z * mt.zs_M;
    double *A = at.M ? at.M + z * at.zs_M : nullptr;
    const int64_t nac = at.M ? at.cols : 0;
    const int64_t c0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, cstep = (int64_t)gridDim.x * blockDim.x;
    for (int64_t R = blockIdx.y; R <= m; R += gridDim.y) {
        const auto row = src.row(z, R, ab + m);
        for (int64_t C = c0; C < mt.ld; C += cstep)
            M[R * mt.ld + C] = C < num_cols ? src.elem(row, C) : 0.0;
        if (!A || R == m) continue;
        const int64_t acol = ab[R];                                         // (a slack column is < num_cols - 1)
        for (int64_t C = c0; C < at.ld; C += cstep)
            A[R * at.ld + C] = art_entry<double>(C, num_cols, nac, acol, [&](int64_t c) { return src.elem(row, c); });
    }
}

// the artificial objective row, from the rows k_assemble stored (launched behind it on the same stream)
__global__ __launch_bounds__(kAssembleThreads) void k_art_objective(TabView at, int64_t m, int64_t num_cols,
                                                                    const int32_t *scratch, int64_t words)
{
    const int64_t z = blockIdx.z, nac = at.cols;
    const int32_t *ab = scratch + z * words * m;
    double *A = at.M + z * at.zs_M;
    for (int64_t C = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; C < at.ld; C += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        if (art_objective_column(C, num_cols, nac))
            for (int64_t R = 0; R < m; ++R)
                if (ab_artificial(ab[R], (int32_t)num_cols)) s = __dadd_rn(s, A[R * at.ld + C]);
        A[m * at.ld + C] = s;
    }
}

// both kernels behind the source's rows kernel (which the caller has launched on s)
template <class Src>
void launch_assemble(const TabView &mt, const TabView &at, const Src &src, const int32_t *scratch, hipStream_t s)
{
    const unsigned n = (unsigned)mt.n_lps;
    const int64_t rows = mt.rows;
    const int64_t ld = at.M && at.ld > mt.ld ? at.ld : mt.ld;
    unsigned bx = (unsigned)((ld + kAssembleThreads - 1) / kAssembleThreads); if (bx > 16) bx = 16;
    unsigned by = (unsigned)(rows < 1024 ? rows : 1024);
    // large batches: a workgroup takes several rows instead of the grid growing past a quarter of a million workgroups
    while (by > 1 && (uint64_t)bx * by * n > (1u << 18)) by = (by + 1) / 2;
    hipLaunchKernelGGL(k_assemble<Src>, dim3(bx, by, n), dim3(kAssembleThreads), 0, s, mt, at, src, scratch);
    if (at.M) {
        const unsigned cx = (unsigned)((at.ld + kAssembleThreads - 1) / kAssembleThreads);
        hipLaunchKernelGGL(k_art_objective, dim3(cx, 1, n), dim3(kAssembleThreads), 0, s, at, src.m(), src.num_cols(), scratch,
                           (int64_t)Src::kWords);
    }
}

// ---- LDS family: one member per workgroup of kAssembleThreads threads, ab[] (m entries, dealt) in LDS and visible to
// every thread.  Where a member's tableau and basis live is a slot: sb_slot of the member view
// (kernels_single_batch.inc) makes it from a batch's view and the member's descriptor.
struct AsmSlot {
    float   *M;           // the member's first row (nullptr: no such tableau)
    int64_t *basis;       // its m basis entries
    int      ld, cols;    // leading dimension and columns, in floats
};

// elem(R, C) is entry C < num_cols of row R <= m of the main tableau.  Both tableaux over their whole leading
// dimension (padding +0.0), consecutive threads consecutive floats; at.M == nullptr: no artificial rows.
template <class Elem>
__device__ __forceinline__ void assemble_member_lds(const AsmSlot &mt, const AsmSlot &at, int m, int num_cols,
                                                    const int32_t *ab, Elem elem)
{
    const int tid = threadIdx.x;
    {
        const int ld = mt.ld;
        float *M = mt.M;
        int64_t *mb = mt.basis;
        for (int R = tid; R < m; R += kAssembleThreads) mb[R] = ab_main_basis(ab[R], num_cols);
        for (int k = tid; k < (m + 1) * ld; k += kAssembleThreads) {
            const int R = k / ld, C = k - R * ld;
            M[k] = C < num_cols ? elem(R, C) : 0.0f;
        }
    }
    if (at.M) {
        const int nac = at.cols, ld = at.ld;
        float *A = at.M;
        int64_t *abasis = at.basis;
        for (int R = tid; R < m; R += kAssembleThreads) abasis[R] = ab[R];
        for (int k = tid; k < m * ld; k += kAssembleThreads) {
            const int R = k / ld, C = k - R * ld;
            A[k] = art_entry<float>(C, num_cols, nac, (int)ab[R], [&](int c) { return elem(R, c); });
        }
        // the artificial objective row, recomputed from the entries (the rows above may not have landed yet)
        for (int C = tid; C < ld; C += kAssembleThreads) {
            float acc = 0.0f;
            if (art_objective_column(C, num_cols, nac)) {
                const int src = C == nac - 1 ? num_cols - 1 : C;
                for (int R = 0; R < m; ++R)
                    if (ab_artificial(ab[R], num_cols)) acc = acc + elem(R, src);
            }
            A[(int64_t)m * ld + C] = acc;
        }
    }
}
