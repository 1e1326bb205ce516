// kernels_single_assemble_global.inc -- the single-float assembly spread over a grid: build-tableau's layout
// (src/simplex.lisp:243-328) written into the members of two GLOBAL-form batches of single-float tableaux
// (capi_single_lps.inc and capi_single_bb.inc drive it: mi355x_sbatch_create_lps_global / _create_nodes_global).
// Part of simplex_kernels.hip (ONE translation unit: included there after kernels_single_lps.inc, inside namespace
// mi355x).  No double appears in this file; it holds no product, every difference and sum is one rounded float
// operation (-ffp-contract=off), and -(0.0f) is never computed.
//
// The single-float member of what kernels_assemble.inc calls the HBM family: ab[] and the source's own per-row words
// live in a per-member scratch plane in device memory (Src::kWords int32 words per constraint row, plane 0 ab[]), a
// member is spread over a grid of column blocks x row blocks x members (the member in the grid's x, the one extent
// that holds 2^30 of them; rows in y, columns in z), and what is written are SbView members under
// the float rules of the LDS family (assemble_member_lds): padding +0.0 over the whole leading dimension, the
// artificial tableau repeating the structural and slack columns, one 1.0 per artificial row dealt in DECREASING row
// order, both bases from ab[] (ab_main_basis), the artificial objective row per column the float sum of the artificial
// rows in INCREASING row order from +0.0f, one rounded addition per row, +0.0 in the artificial columns.
//
//   k_sga_lps_rows      row pass from problem rows: k_blp_rows' job under k_slp_assemble's rules (a)-(c) -- a row whose
//                       right-hand side is < 0.0f (false for -0.0 and NaN) flips, slack columns in row order, the
//                       artificial ranks from prefix counts.  One workgroup per member; a thread owns a chunk of rows
//                       and the counts before the chunk come through LDS, so any m goes.
//   k_sga_node_rows     row pass for node rows: k_sbb_assemble's classification (sbb_node_row: rhs = float(bound) -
//                       offset, the flip, the base's artificial rows renumbered) with the same chunks and prefix counts in
//                       place of the serial deal.  Its LDS is static (two counts per thread): it has NO limit of the
//                       kind k_sbb_assemble has (m + 3 d words in 48 KiB), every m and depth go.
//   k_sga_write<Src>    the ONE write pass, templated over the source as k_assemble<Src> is: every entry of both
//                       tableaux but the artificial objective row.  Rows start on 128-byte boundaries (ld is a
//                       multiple of 32 floats), so a lane writes whole 16-byte quads, consecutive lanes consecutive
//                       quads; the grid is two-dimensional inside a member, so no entry costs an integer division.  A
//                       member is below 2^32 bytes (sgbatch_available), so offsets inside it are 32-bit; q * stride
//                       stays 64-bit.
//   k_sga_art_objective the artificial objective row, a launch of its own behind the write pass: one thread per
//                       column walks the stored rows in order (consecutive lanes read consecutive floats of a row).
//
// Ordering between the three comes from launches on ONE stream only: the row pass has finished before the write pass
// reads its planes, the write pass before the objective row reads its rows.  No flags, no atomics, no spinning; a
// workgroup never waits for another, and all loads and stores are plain.

constexpr int kSgaThreads = 256;
constexpr unsigned kSgaMaxColBlocks = 8;          // column blocks of a member's grid: past them a workgroup strides
constexpr unsigned kSgaMaxRowBlocks = 1024;       // row blocks of a member's grid: past them a workgroup strides
constexpr uint64_t kSgaMaxWorkgroups = 1u << 16;  // of the write launch: past them a workgroup takes several rows

// a thread's counts (slack rows, artificial rows of its chunk) -> those of the chunks before it, and the artificial
// rows of the whole member.  Every thread of the workgroup calls it once.
__device__ __forceinline__ void sga_counts_before(int32_t ns, int32_t na, int32_t &slack_before, int32_t &art_before,
                                                  int32_t &art_all)
{
    __shared__ int32_t n_slack_of[kSgaThreads], n_art_of[kSgaThreads];
    n_slack_of[threadIdx.x] = ns;
    n_art_of[threadIdx.x] = na;
    __syncthreads();
    slack_before = art_before = art_all = 0;
    for (int t = 0; t < kSgaThreads; ++t) {
        if (t < (int)threadIdx.x) { slack_before += n_slack_of[t]; art_before += n_art_of[t]; }
        art_all += n_art_of[t];
    }
}

// the rows [i0, i1) of thread t when m rows are dealt to the workgroup in chunks
__device__ __forceinline__ void sga_chunk(int m, int &i0, int &i1)
{
    const int chunk = (m + kSgaThreads - 1) / kSgaThreads;
    const int64_t lo = (int64_t)threadIdx.x * chunk;
    i0 = lo < m ? (int)lo : m;
    i1 = i0 + chunk < m ? i0 + chunk : m;
}

// ---- source: problem rows.  Per row in scratch: ab[], the row's word (row_word), its slack column (-1: none)
struct SgaLpsSrc {
    SlpView sp;
    static constexpr int kWords = 3;
    struct Row { const float *Lr; int word, scol; };
    __host__ __device__ int m() const { return (int)sp.m; }
    __host__ __device__ int num_cols() const { return (int)(sp.ncv + sp.n_slack + 1); }
    __device__ Row row(int64_t z, int R, const int32_t *priv) const
    {
        const int m = (int)sp.m;
        const float *Lr = sp.L + (z * (m + 1) + R) * (sp.ncv + 1);
        return R < m ? Row{Lr, priv[R], priv[m + R]} : Row{Lr, 0, -1};
    }
    __device__ float elem(const Row &r, int C) const { return slp_main_elem(r.Lr, (int)sp.ncv, r.word, r.scol, C, num_cols()); }
};

__device__ __forceinline__ int sga_lps_word(const SlpView &sp, int64_t z, int i)
{
    return row_word(sp.L[(z * (sp.m + 1) + i) * (sp.ncv + 1) + sp.ncv] < 0.0f, sp.sense[z * sp.m + i]);     // :243
}

// Member blockIdx.x: flips, senses, slack columns, ab[] and both bases.  at.M == nullptr: no artificial rows.
__global__ __launch_bounds__(kSgaThreads) void k_sga_lps_rows(SbView mt, SbView at, SlpView sp, int32_t *scratch)
{
    const int64_t z = blockIdx.x;
    const int m = (int)sp.m, ncv = (int)sp.ncv, cols = ncv + (int)sp.n_slack + 1;
    int32_t *ab = scratch + z * SgaLpsSrc::kWords * m, *word = ab + m, *scol = word + m;
    int i0, i1;
    sga_chunk(m, i0, i1);
    int32_t ns = 0, na = 0;
    for (int i = i0; i < i1; ++i) {
        const int op = sga_lps_word(sp, z, i) >> 1;
        ns += op != 2;
        na += op != 0;
    }
    int32_t slack_before, art_through, art_all;
    sga_counts_before(ns, na, slack_before, art_through, art_all);
    int64_t *mb = mt.basis + z * m;
    int64_t *abasis = at.M ? at.basis + z * m : nullptr;
    for (int i = i0; i < i1; ++i) {
        const int w = sga_lps_word(sp, z, i), op = w >> 1;
        art_through += op != 0;
        int32_t sc, a;
        slp_row_columns(w, ncv, cols, slack_before, art_through, art_all, sc, a);
        slack_before += op != 2;
        ab[i] = a; word[i] = w; scol[i] = sc;
        mb[i] = ab_main_basis(a, cols);
        if (abasis) abasis[i] = a;
    }
}

// ---- source: a base tableau plus node rows.  Per row in scratch: ab[], and for a node row the words of SbbRow
// (kernels_single_bb.inc: right-hand side after the flip as float bits, the variable's first column, the flags), one
// plane each, read only at the node rows.  The classification and the entries are that file's sbb_node_row / sbb_elem.
struct SgaNodeSrc {
    SbbBaseView b;
    int d;
    static constexpr int kWords = 4;
    using Row = SbbRow;
    __host__ __device__ int m() const { return (int)(b.rows - 1) + d; }
    __host__ __device__ int num_cols() const { return (int)b.cols + d; }
    __device__ Row row(int64_t, int R, const int32_t *priv) const
    {
        const int nb = (int)b.nb, mm = m();
        if (R >= nb && R < nb + d)
            return Row{nullptr, __int_as_float(priv[R]), priv[mm + R], priv[2 * mm + R], (int)b.ncv + R};
        return Row{b.B + (int64_t)(R < nb ? R : R - d) * b.cols, 0.0f, 0, 0, -1};   // base row (rows_b - 1: objective)
    }
    __device__ float elem(const Row &r, int C) const { return sbb_elem(b, d, r, C); }
};

// Node blockIdx.x: the node rows' words, ab[] and both bases.  at.M == nullptr: no artificial rows.
__global__ __launch_bounds__(kSgaThreads) void k_sga_node_rows(SbView mt, SbView at, SbbBaseView b, XbbNodeRows nr, int32_t *scratch)
{
    const int64_t q = blockIdx.x;
    const int d = (int)nr.d, m = (int)(b.rows - 1) + d, num_cols = (int)b.cols + d;
    const SbbNode nd = sbb_node(nr, q);
    auto classify = [&](int R, float &rhs, int32_t &col, int32_t &flags) {
        return sbb_node_row(b, nd.var, nd.sense, nd.bound, d, R, rhs, col, flags);
    };
    int32_t *ab = scratch + q * SgaNodeSrc::kWords * m, *rhs_w = ab + m, *col_w = rhs_w + m, *flags_w = col_w + m;
    int i0, i1;
    sga_chunk(m, i0, i1);
    float rhs = 0.0f;
    int32_t col = 0, flags = 0, na = 0;
    for (int R = i0; R < i1; ++R) na += classify(R, rhs, col, flags) == num_cols;
    int32_t unused, art_through, art_all;
    sga_counts_before(0, na, unused, art_through, art_all);
    int64_t *mb = mt.basis + q * m;
    int64_t *abasis = at.M ? at.basis + q * m : nullptr;
    for (int R = i0; R < i1; ++R) {
        rhs = 0.0f; col = 0; flags = 0;
        int32_t a = classify(R, rhs, col, flags);
        if (a == num_cols) {
            ++art_through;
            a = num_cols - 1 + (art_all - art_through);                     // what deal_artificial_columns leaves
        }
        ab[R] = a; rhs_w[R] = __float_as_int(rhs); col_w[R] = col; flags_w[R] = flags;
        mb[R] = ab_main_basis(a, num_cols);
        if (abasis) abasis[R] = a;
    }
}

// ---- the write pass: every entry of both tableaux but the artificial objective row; grid (member, row blocks, column
// blocks).  A lane writes quads: 4 consecutive columns, 16 bytes.
template <class Src>
__global__ __launch_bounds__(kSgaThreads) void k_sga_write(SbView mt, SbView at, Src src, const int32_t *scratch)
{
    const int64_t z = blockIdx.x;
    const int m = src.m(), num_cols = src.num_cols();
    const int32_t *ab = scratch + z * Src::kWords * m;
    float *M = mt.M + z * mt.stride;                                        // (64-bit: q * stride)
    float *A = at.M ? at.M + z * at.stride : nullptr;
    const unsigned ldm = (unsigned)mt.ld, lda = at.M ? (unsigned)at.ld : 0u;
    const int nac = at.M ? (int)at.cols : 0;
    const unsigned c0 = 4u * (blockIdx.z * kSgaThreads + threadIdx.x), cstep = 4u * gridDim.z * kSgaThreads;
    for (unsigned R = blockIdx.y; R <= (unsigned)m; R += gridDim.y) {
        const auto row = src.row(z, (int)R, ab + m);
        auto main_at = [&](int C) { return C < num_cols ? src.elem(row, C) : 0.0f; };
        for (unsigned C = c0; C < ldm; C += cstep) {                        // (ld is a multiple of 4: whole quads)
            const int c = (int)C;
            const float4 v = make_float4(main_at(c), main_at(c + 1), main_at(c + 2), main_at(c + 3));
            *reinterpret_cast<float4 *>(M + (R * ldm + C)) = v;             // (32-bit inside a member)
        }
        if (!A || R == (unsigned)m) continue;
        const int acol = ab[R];                                             // (a slack column is < num_cols - 1)
        auto art_at = [&](int C) { return art_entry<float>(C, num_cols, nac, acol, [&](int c) { return src.elem(row, c); }); };
        for (unsigned C = c0; C < lda; C += cstep) {
            const int c = (int)C;
            const float4 v = make_float4(art_at(c), art_at(c + 1), art_at(c + 2), art_at(c + 3));
            *reinterpret_cast<float4 *>(A + (R * lda + C)) = v;
        }
    }
}

// the artificial objective row, from the rows k_sga_write stored (launched behind it on the same stream): one thread
// per column, the rows in increasing order from +0.0f
__global__ __launch_bounds__(kSgaThreads) void k_sga_art_objective(SbView at, int m, int num_cols, const int32_t *scratch,
                                                                   int words)
{
    const int64_t z = blockIdx.x;
    const int32_t *ab = scratch + z * words * m;
    float *A = at.M + z * at.stride;
    const unsigned ld = (unsigned)at.ld, nac = (unsigned)at.cols;
    for (unsigned C = blockIdx.z * kSgaThreads + threadIdx.x; C < ld; C += gridDim.z * kSgaThreads) {
        float s = 0.0f;
        if (art_objective_column(C, (unsigned)num_cols, nac))
            for (unsigned R = 0; R < (unsigned)m; ++R)
                if (ab_artificial(ab[R], num_cols)) s = s + A[R * ld + C];
        A[(unsigned)m * ld + C] = s;
    }
}

// all three passes of a source on s: `rows` launches the source's row pass.  ev (measurement aid, may be nullptr): four
// events recorded in front of the row pass and behind each of the three passes
template <class Src, class Rows>
void sga_launch(const SbView &mt, const SbView &at, const Src &src, int32_t *scratch, hipStream_t s, Rows rows,
                hipEvent_t *ev = nullptr)
{
    const unsigned n = (unsigned)mt.n_lps;
    if (ev) (void)hipEventRecord(ev[0], s);
    rows(n);
    if (ev) (void)hipEventRecord(ev[1], s);
    const unsigned quads = (unsigned)((at.M && at.ld > mt.ld ? at.ld : mt.ld) / 4);
    unsigned bz = (quads + kSgaThreads - 1) / kSgaThreads; if (bz > kSgaMaxColBlocks) bz = kSgaMaxColBlocks;
    unsigned by = (unsigned)(mt.rows < kSgaMaxRowBlocks ? mt.rows : kSgaMaxRowBlocks);
    // many members: a workgroup takes several rows instead of the grid growing past kSgaMaxWorkgroups
    while (by > 1 && (uint64_t)bz * by * n > kSgaMaxWorkgroups) by = (by + 1) / 2;
    hipLaunchKernelGGL(k_sga_write<Src>, dim3(n, by, bz), dim3(kSgaThreads), 0, s, mt, at, src, (const int32_t *)scratch);
    if (ev) (void)hipEventRecord(ev[2], s);
    if (at.M) {
        unsigned cz = (unsigned)((at.ld + kSgaThreads - 1) / kSgaThreads); if (cz > 4 * kSgaMaxColBlocks) cz = 4 * kSgaMaxColBlocks;
        hipLaunchKernelGGL(k_sga_art_objective, dim3(n, 1, cz), dim3(kSgaThreads), 0, s, at, src.m(), src.num_cols(),
                           (const int32_t *)scratch, (int)Src::kWords);
    }
    if (ev) (void)hipEventRecord(ev[3], s);
}

size_t sga_lps_scratch_bytes(int64_t n_lps, int64_t m) { return (size_t)n_lps * SgaLpsSrc::kWords * (size_t)m * sizeof(int32_t); }
size_t sga_nodes_scratch_bytes(int64_t n_nodes, int64_t m) { return (size_t)n_nodes * SgaNodeSrc::kWords * (size_t)m * sizeof(int32_t); }

void launch_sga_lps(const SbView &mt, const SbView &at, const SlpView &sp, int32_t *scratch, hipStream_t s, hipEvent_t *ev)
{
    sga_launch(mt, at, SgaLpsSrc{sp}, scratch, s, [&](unsigned n) {
        hipLaunchKernelGGL(k_sga_lps_rows, dim3(n), dim3(kSgaThreads), 0, s, mt, at, sp, scratch);
    }, ev);
}

void launch_sga_nodes(const SbView &mt, const SbView &at, const SbbBaseView &b, const XbbNodeRows &nr, int32_t *scratch,
                      hipStream_t s)
{
    sga_launch(mt, at, SgaNodeSrc{b, (int)nr.d}, scratch, s, [&](unsigned n) {
        hipLaunchKernelGGL(k_sga_node_rows, dim3(n), dim3(kSgaThreads), 0, s, mt, at, b, nr, scratch);
    });
}
