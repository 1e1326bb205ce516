// kernels_single_bb.inc -- single-float branch-and-bound (simplex-solver, src/simplex.lisp:462-542): node
// tableaux written in float straight into the padded members of two batches of single-float tableaux, and the
// light read-back of a solved batch.
// Part of simplex_kernels.hip (ONE translation unit: included there after kernels_single_batch.inc, inside
// namespace mi355x).  No double appears in this file; it holds no product, and every difference and sum is one
// rounded float operation (-ffp-contract=off).
//
//   k_sbb_assemble   one workgroup per node of a group (same depth d, same number of artificial rows): the
//                    single-float counterpart of k_xbb_assemble.  Rows, columns, bases and the order in which
//                    artificial columns are dealt are those of the header of kernels_bb.inc (src/simplex.lisp:146,
//                    198-202, 243-265, 292-325).  The base problem's general-form tableau comes as floats; a node
//                    row `var <= / >= bound` has
//                      rhs = float(bound) - offset_v   (one rounding; no offset for a free variable, :230-237),
//                    and when rhs < 0 the row is negated and its sense flipped (:243-252).  What Lisp negates
//                    there are integer zeros, so the row's other entries are +0.0 -- they are written as such,
//                    never computed as -(0.0f).  The d columns inserted into base rows are integer zeros in Lisp
//                    as well: +0.0 also in a base row that build-tableau negated (unlike kernels_bb.inc's f64
//                    rows).  The artificial objective row (:302-316) is the column sum over the artificial rows
//                    in increasing row order from 0.0f, recomputed from the entries; the host lets a group in only
//                    when every integer partial sum of it is exact in a float (capi_single_bb.inc: the guard).
//                    The write pass is assemble_member_lds (kernels_assemble.inc).
//   k_sb_readback    per member: the right-hand-side column, the objective row and the basis, gathered into
//                    one buffer -- what tableau-objective-value and tableau-variable read (src/simplex.lisp:74-107).

constexpr int kSbbThreads = 256;

// ---- the node source's rules, ONE copy for both assembly families (k_sbb_assemble here, k_sga_node_rows and
// SgaNodeSrc of kernels_single_assemble_global.inc).
// What an entry of row R <= m needs, asked through accessors so that each family reads a word where it has it.  A node
// row: its right-hand side after the flip, its variable's first column, its flags (kind bits 0-1, flipped bit 2, sense
// after the flip bit 3: 1 `>=`), its slack column.  A base row (rows_b - 1: the objective row): where it starts.
// SbbRow holds the words, loaded once per row (the grid family walks a row); SbbLdsRow reads them from the LDS planes
// of k_sbb_assemble, indexed by the node row's number, only in the branch that needs them (an entry there has its own
// row).
struct SbbRow {
    const float *Br;      // nullptr: a node row
    float w_rhs;
    int   w_col, w_flags, w_scol;
    __device__ bool node() const { return !Br; }
    __device__ const float *base() const { return Br; }
    __device__ float rhs() const { return w_rhs; }
    __device__ int col() const { return w_col; }
    __device__ int flags() const { return w_flags; }
    __device__ int scol() const { return w_scol; }
};
struct SbbLdsRow {
    const SbbBaseView &b;
    int d, R;
    const float   *p_rhs;
    const int32_t *p_col, *p_flags;
    __device__ bool node() const { return R >= (int)b.nb && R < (int)b.nb + d; }
    __device__ const float *base() const { return b.B + (int64_t)(R < (int)b.nb ? R : R - d) * (int)b.cols; }
    __device__ float rhs() const { return p_rhs[R - (int)b.nb]; }
    __device__ int col() const { return p_col[R - (int)b.nb]; }
    __device__ int flags() const { return p_flags[R - (int)b.nb]; }
    __device__ int scol() const { return (int)b.ncv + R; }
};

// Row R of a node of depth d (var, sense, bound: the node's own d entries, newest first) before the artificial columns
// are dealt: its ab[] entry (num_cols for an artificial row) and, for a node row, rhs / col / flags of SbbRow.
__device__ __forceinline__ int32_t sbb_node_row(const SbbBaseView &b, const int64_t *var, const int32_t *sense,
                                                const int64_t *bound, int d, int R, float &rhs_out, int32_t &col, int32_t &flags)
{
    const int nb = (int)b.nb, ncv = (int)b.ncv, num_cols = (int)b.cols + d;
    if (R >= nb && R < nb + d) {
        const int k = R - nb;
        const int64_t v = var[k];
        const int kind = b.kind[v];
        float rhs = (float)bound[k];                                        // (a floor or ceiling of a float: exact)
        if (kind != 2) rhs = rhs - b.voff[v];                               // coef 1, :230-237
        const bool flip = rhs < 0.0f;
        const int op = row_word(flip, sense[k]) >> 1;
        rhs_out = flip ? -rhs : rhs;
        col = (int32_t)b.vcol[v];
        flags = kind | (flip ? 4 : 0) | (op ? 8 : 0);
        return op ? num_cols : ncv + R;
    }
    const int64_t bb = b.basis[R < nb ? R : R - d];
    return (int32_t)(bb == b.cols ? num_cols : (bb >= ncv + nb ? bb + d : bb));
}

// entry C < cols_b + d of that row of the main tableau
template <class Row>
__device__ __forceinline__ float sbb_elem(const SbbBaseView &b, int d, const Row &r, int C)
{
    const int nb = (int)b.nb, ncv = (int)b.ncv, cols_b = (int)b.cols, last = cols_b + d - 1;
    if (r.node()) {
        const int f = r.flags(), kind = f & 3;
        const bool flip = (f & 4) != 0;
        if (C == last) return r.rhs();
        if (C == r.col()) return ((kind == 1) != flip) ? -1.0f : 1.0f;
        if (kind == 2 && C == r.col() + 1) return flip ? 1.0f : -1.0f;
        if (C == r.scol()) return (f & 8) ? -1.0f : 1.0f;
        return 0.0f;
    }
    const float *row = r.base();
    if (C == last) return row[cols_b - 1];
    if (C < ncv + nb) return row[C];
    if (C < ncv + nb + d) return 0.0f;                                       // (+0.0 also in a row build-tableau negated)
    return row[C - d];
}

// the node rows of a batch: every node at one depth (XbbNodeRows), or each at its own (a ragged batch)
struct SbbNode { const int64_t *var; const int32_t *sense; const int64_t *bound; int d; };
__device__ __forceinline__ SbbNode sbb_node(const XbbNodeRows &nr, int64_t q)
{
    return SbbNode{nr.var + q * nr.d, nr.sense + q * nr.d, nr.bound + q * nr.d, (int)nr.d};
}
__device__ __forceinline__ SbbNode sbb_node(const SrbbNodeRows &nr, int64_t q)
{
    const SrbbNode nd = nr.nodes[q];
    return SbbNode{nr.var + nd.off, nr.sense + nd.off, nr.bound + nd.off, nd.d};
}

// One node, the whole workgroup: its rows and the base's classified into lds (m + 3 d words, m = base constraint rows
// + d: ab[], then per node row rhs, column, flags), the artificial columns dealt, then the write pass into the node's
// slots.
__device__ __forceinline__ void sbb_assemble_member(const AsmSlot &mt, const AsmSlot &at, const SbbBaseView &b, const SbbNode &nd,
                                                    int32_t *lds)
{
    const int tid = threadIdx.x;
    const int nb = (int)b.nb, d = nd.d;
    const int m = (int)(b.rows - 1) + d, num_cols = (int)b.cols + d;
    int32_t *ab = lds, *col = lds + m + d, *flags = lds + m + 2 * d;
    float *rhs = reinterpret_cast<float *>(lds + m);
    for (int R = tid; R < m; R += kSbbThreads) {
        float r = 0.0f;
        int32_t c = 0, f = 0;
        ab[R] = sbb_node_row(b, nd.var, nd.sense, nd.bound, d, R, r, c, f);
        if (R >= nb && R < nb + d) { rhs[R - nb] = r; col[R - nb] = c; flags[R - nb] = f; }
    }
    __syncthreads();
    if (tid == 0) deal_artificial_columns(ab, m, num_cols);
    __syncthreads();
    assemble_member_lds(mt, at, m, num_cols, ab, [&](int R, int C) {
        return sbb_elem(b, d, SbbLdsRow{b, d, R, rhs, col, flags}, C);
    });
}

// The node the workgroup owns (blockIdx.x).  at.M == nullptr: no node has artificial rows.  Dynamic LDS:
// sbb_assemble_lds of the launch's largest node.
template <class View, class Nodes>
__global__ __launch_bounds__(kSbbThreads) void k_sbb_assemble(View mt, View at, SbbBaseView b, Nodes nr)
{
    extern __shared__ __attribute__((aligned(16))) int32_t sbb_lds[];
    const int64_t q = blockIdx.x;
    const SbbNode nd = sbb_node(nr, q);
    const SrMember dm = sb_descriptor(mt, q), da = sb_descriptor_art(at, q, dm);
    sbb_assemble_member(sb_slot(mt, dm), sb_slot(at, da), b, nd, sbb_lds);
}

// The member the workgroup owns: its last column at rhs + (the rows of the members before it), its last row at obj +
// (their columns), its basis at basis + (their rows - 1) -- three concatenated planes, member-major.
__device__ __forceinline__ int64_t sb_cols_before(const SbView &v, const int64_t *, int64_t q) { return q * v.cols; }
__device__ __forceinline__ int64_t sb_cols_before(const SrView &, const int64_t *col_off, int64_t q) { return col_off[q]; }
__device__ __forceinline__ int64_t sb_rows_before(const SbView &v, const SrMember &, int64_t q) { return q * v.rows; }
__device__ __forceinline__ int64_t sb_rows_before(const SrView &, const SrMember &d, int64_t q) { return d.basis_off + q; }
template <class View>
__global__ __launch_bounds__(kSbbThreads) void k_sb_readback(View v, const int64_t *col_off, float *rhs, float *obj, int64_t *basis)
{
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const SrMember d = sb_descriptor(v, q);
    const int64_t R = d.rows, C = d.cols, m = R - 1, co = sb_cols_before(v, col_off, q), ro = sb_rows_before(v, d, q);
    const float *M = v.M + d.m_off;
    for (int64_t i = tid; i < R; i += kSbbThreads) rhs[ro + i] = M[i * d.ld + C - 1];
    for (int64_t j = tid; j < C; j += kSbbThreads) obj[co + j] = M[m * d.ld + j];
    for (int64_t i = tid; i < m; i += kSbbThreads) basis[d.basis_off + i] = v.basis[d.basis_off + i];
}

size_t sbb_assemble_lds(int64_t m, int64_t d)
{
    return ((size_t)(m + 3 * d) * sizeof(int32_t) + 15) & ~(size_t)15;
}
namespace {
template <class View, class Nodes>
void sbb_assemble_launch(const View &mt, const View &at, const SbbBaseView &b, const Nodes &nr, size_t lds, hipStream_t s)
{
    hipLaunchKernelGGL((k_sbb_assemble<View, Nodes>), dim3((unsigned)mt.n_lps), dim3(kSbbThreads), lds, s, mt, at, b, nr);
}
template <class View>
void sb_readback_launch(const View &v, const int64_t *col_off, float *rhs, float *obj, int64_t *basis, hipStream_t s)
{
    hipLaunchKernelGGL((k_sb_readback<View>), dim3((unsigned)v.n_lps), dim3(kSbbThreads), 0, s, v, col_off, rhs, obj, basis);
}
}  // namespace
void launch_sbb_assemble(const SbView &mt, const SbView &at, const SbbBaseView &b, const XbbNodeRows &nr, hipStream_t s)
{
    sbb_assemble_launch(mt, at, b, nr, sbb_assemble_lds(mt.rows - 1, nr.d), s);
}
void launch_sbb_assemble(const SrView &mt, const SrView &at, const SbbBaseView &b, const SrbbNodeRows &nr, size_t lds, hipStream_t s)
{
    sbb_assemble_launch(mt, at, b, nr, lds, s);
}
void launch_sb_readback(const SbView &v, float *rhs, float *obj, int64_t *basis, hipStream_t s)
{
    sb_readback_launch(v, nullptr, rhs, obj, basis, s);
}
void launch_sb_readback(const SrView &v, const int64_t *col_off, float *rhs, float *obj, int64_t *basis, hipStream_t s)
{
    sb_readback_launch(v, col_off, rhs, obj, basis, s);
}
