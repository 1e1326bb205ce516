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

// LDS of k_sbb_assemble: per constraint row its artificial-basis entry, per node row (rhs, column, flags)
struct SbbLds {
    int32_t *ab;          // m
    float   *rhs;         // d: the right-hand side after the flip
    int32_t *col;         // d: the variable's first column
    int32_t *flags;       // d: kind (bits 0-1), flipped (bit 2), sense after the flip (bit 3: 1 `>=`)
};

__device__ __forceinline__ float sbb_main_elem(const SbbBaseView &b, const SbbLds &l, int d, int R, int C)
{
    const int nb = (int)b.nb, ncv = (int)b.ncv, cols_b = (int)b.cols, last = cols_b + d - 1;
    if (R >= nb && R < nb + d) {
        const int k = R - nb, f = l.flags[k], kind = f & 3;
        const bool flip = (f & 4) != 0;
        if (C == last) return l.rhs[k];
        if (C == l.col[k]) return ((kind == 1) != flip) ? -1.0f : 1.0f;
        if (kind == 2 && C == l.col[k] + 1) return flip ? 1.0f : -1.0f;
        if (C == ncv + R) return (f & 8) ? -1.0f : 1.0f;
        return 0.0f;
    }
    const float *row = b.B + (int64_t)(R < nb ? R : R - d) * cols_b;       // base row (rows_b - 1: objective)
    if (C == last) return row[cols_b - 1];
    if (C < ncv + nb) return row[C];
    if (C < ncv + nb + d) return 0.0f;
    return row[C - d];
}

// One node of depth d, the whole workgroup: its rows (var, sense, bound: the node's own d entries, newest first) and
// the base's classified into lds (m + 3 d words, m = base constraint rows + d), the artificial columns dealt, then the
// write pass into the node's slots.
__device__ __forceinline__ void sbb_assemble_member(const AsmSlot &mt, const AsmSlot &at, const SbbBaseView &b, const int64_t *var,
                                                    const int32_t *sense, const int64_t *bound, int d, int32_t *lds)
{
    const int tid = threadIdx.x;
    const int nb = (int)b.nb, ncv = (int)b.ncv;
    const int m = (int)(b.rows - 1) + d, num_cols = (int)b.cols + d;
    SbbLds l;
    l.ab = lds;
    l.rhs = reinterpret_cast<float *>(lds + m);
    l.col = lds + m + d;
    l.flags = lds + m + 2 * d;
    for (int k = tid; k < d; k += kSbbThreads) {
        const int64_t v = var[k];
        const int kind = b.kind[v];
        float rhs = (float)bound[k];                                        // (a floor or ceiling of a float: exact)
        if (kind != 2) rhs = rhs - b.voff[v];                               // coef 1, :230-237
        const bool flip = rhs < 0.0f;
        const int op = row_word(flip, sense[k]) >> 1;
        l.rhs[k] = flip ? -rhs : rhs;
        l.col[k] = (int32_t)b.vcol[v];
        l.flags[k] = kind | (flip ? 4 : 0) | (op ? 8 : 0);
    }
    __syncthreads();
    for (int R = tid; R < m; R += kSbbThreads) {
        int64_t bas;
        if (R >= nb && R < nb + d) {
            bas = (l.flags[R - nb] & 8) ? num_cols : ncv + R;
        } else {
            const int64_t bb = b.basis[R < nb ? R : R - d];
            bas = bb == b.cols ? num_cols : (bb >= ncv + nb ? bb + d : bb);
        }
        l.ab[R] = (int32_t)bas;
    }
    __syncthreads();
    if (tid == 0) deal_artificial_columns(l.ab, m, num_cols);
    __syncthreads();
    assemble_member_lds(mt, at, m, num_cols, l.ab, [&](int R, int C) { return sbb_main_elem(b, l, d, R, C); });
}

// Member blockIdx.x.  at.M == nullptr: the group has no artificial rows.  Dynamic LDS: sbb_assemble_lds(m, d).
__global__ __launch_bounds__(kSbbThreads) void k_sbb_assemble(SbView mt, SbView at, SbbBaseView b, XbbNodeRows nr)
{
    extern __shared__ __attribute__((aligned(16))) int32_t sbb_lds[];
    const int64_t q = blockIdx.x;
    const int d = (int)nr.d, m = (int)(b.rows - 1) + d;
    sbb_assemble_member(sb_slot(mt, q, m), sb_slot(at, q, m), b, nr.var + q * d, nr.sense + q * d, nr.bound + q * d, d, sbb_lds);
}

// Member blockIdx.x: rhs + q * rows its last column, obj + q * cols its last row, basis + q * (rows - 1) its basis.
__global__ __launch_bounds__(kSbbThreads) void k_sb_readback(SbView v, float *rhs, float *obj, int64_t *basis)
{
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x, R = v.rows, C = v.cols, m = R - 1;
    const float *M = v.M + q * v.stride;
    for (int64_t i = tid; i < R; i += kSbbThreads) rhs[q * R + i] = M[i * v.ld + C - 1];
    for (int64_t j = tid; j < C; j += kSbbThreads) obj[q * C + j] = M[m * v.ld + j];
    for (int64_t i = tid; i < m; i += kSbbThreads) basis[q * m + i] = v.basis[q * m + i];
}

size_t sbb_assemble_lds(int64_t m, int64_t d)
{
    return ((size_t)(m + 3 * d) * sizeof(int32_t) + 15) & ~(size_t)15;
}
void launch_sbb_assemble(const SbView &mt, const SbView &at, const SbbBaseView &b, const XbbNodeRows &nr, hipStream_t s)
{
    hipLaunchKernelGGL(k_sbb_assemble, dim3((unsigned)mt.n_lps), dim3(kSbbThreads), sbb_assemble_lds(mt.rows - 1, nr.d), s,
                       mt, at, b, nr);
}
void launch_sb_readback(const SbView &v, float *rhs, float *obj, int64_t *basis, hipStream_t s)
{
    hipLaunchKernelGGL(k_sb_readback, dim3((unsigned)v.n_lps), dim3(kSbbThreads), 0, s, v, rhs, obj, basis);
}
