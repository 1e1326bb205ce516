// kernels_single_lps.inc -- batches of single-float LPs assembled from the members' problem rows: build-tableau's
// steps src/simplex.lisp:243-328 under Lisp's int / single-float contagion, written in float straight into the
// padded members of two batches of single-float tableaux (capi_single_lps.inc drives it).
// Part of simplex_kernels.hip (ONE translation unit: included there after kernels_single_bb.inc, inside namespace
// mi355x).  No double appears in this file; it holds no product, and every sum is one rounded float addition
// (-ffp-contract=off).
//
//   k_slp_assemble   one 256-thread workgroup per member, the form of k_sbb_assemble.  A member arrives in column
//                    space as for kernels_batch_lps.inc, in floats: m rows of ncv structural coefficients and the
//                    right-hand side (offsets already subtracted, :189-241), then the objective row (:270-283), one
//                    sense per row.  What it writes is what build_tableau_single makes of the problem, bit for bit:
//                      (a) a row whose right-hand side is < 0.0f (false for -0.0 and NaN) is negated and its sense
//                          flipped (:243-252).  Lisp's matrix starts as INTEGER zeros and (- 0) is 0, so the slack
//                          columns of a negated row and the coefficients the problem never mentions stay +0.0:
//                          the kernel writes x == 0 ? +0.0f : -x and never computes -(0.0f).  (The double rows of
//                          kernels_batch_lps.inc carry -0.0 there.)  A zero of a negated row is therefore read as Lisp's
//                          integer zero; a member with a single-float zero in such a row is not for this kernel.
//                      (b) slack columns in row order for the rows that are not `=` (:254-265); the bases, the
//                          artificial columns and the artificial objective row (a float sum in increasing row
//                          order, :302-316) as kernels_assemble.inc lays them out.
//                      (c) Lisp keeps integers exact among themselves in that sum; the host lets a member in only
//                          when every integer partial sum is exact in a float (capi_single_lps.inc: the guard).
//                    Row pass: thread R owns constraint row R.  One trip of the workgroup covers every member a batch
//                    can hold: a batch of m rows has a tableau (main, or artificial when there are artificial rows)
//                    of m + 1 rows and at least m + 2 columns, and the LDS budget of the solve (kSingleLdsBudget,
//                    single_lds_bytes) declines that from m = 197 on (198 x 199 floats stored as 198 x 200, plus the
//                    pivot row and the column snapshot: 160 000 bytes > 159 744), so m <= 196 < 256; the launcher's
//                    caller checks m <= kSlpMaxRows all the same.  Per row three LDS words: flip and sense after the
//                    flip, slack column, artificial-basis entry; the slack columns and artificial ranks are a workgroup
//                    prefix count (one ballot per wave, the four wave totals through LDS).
//                    Write pass: assemble_member_lds (kernels_assemble.inc).

constexpr int kSlpThreads = 256;

// entry (R, C) of the main tableau, C < cols: Lr the member's row R, word / scol row R's (objective row: 0 / -1)
__device__ __forceinline__ float slp_main_elem(const float *Lr, int ncv, int word, int scol, int C, int cols)
{
    if (C < ncv || C == cols - 1) {
        const float x = Lr[C < ncv ? C : ncv];
        if (!(word & 1)) return x;
        return x == 0.0f ? 0.0f : -x;                                       // (a): Lisp's (- 0) is 0
    }
    if (C == scol) return (word >> 1) == 0 ? 1.0f : -1.0f;
    return 0.0f;
}

// per row of a member: its word (row_word), slack column (-1: none), artificial-basis entry (simplex_kernels.h); the
// wave totals of the prefix counts
struct SlpLds {
    int32_t word[kSlpMaxRows], scol[kSlpMaxRows], ab[kSlpMaxRows];
    int32_t wave_slack[kSlpThreads / 64], wave_art[kSlpThreads / 64];
};

// ONE copy of a problem row's columns, for both assembly families (slp_assemble_member here, k_sga_lps_rows of
// kernels_single_assemble_global.inc): from the row's word, the rows before it that are not `=`, the artificial rows
// up to and including it and those of the whole member -> its slack column (-1: none) and its ab[] entry, which for an
// artificial row is what deal_artificial_columns leaves: cols - 1 + the artificial rows with a greater index.
__device__ __forceinline__ void slp_row_columns(int word, int ncv, int cols, int slack_before, int art_through, int art_all,
                                                int32_t &scol, int32_t &ab)
{
    scol = (word >> 1) != 2 ? ncv + slack_before : -1;
    ab = row_word_artificial(word) ? cols - 1 + (art_all - art_through) : scol;
}

// the rows of a batch's members: every member of one shape (SlpView), or each of its own (a ragged batch)
struct SlpMember { const float *L; const int32_t *sense; int m, ncv, cols; };       // cols: ncv + slack columns + 1
__device__ __forceinline__ SlpMember slp_member(const SlpView &sp, int64_t q)
{
    const int m = (int)sp.m, ncv = (int)sp.ncv;
    return SlpMember{sp.L + q * (int64_t)(m + 1) * (ncv + 1), sp.sense + q * m, m, ncv, ncv + (int)sp.n_slack + 1};
}
__device__ __forceinline__ SlpMember slp_member(const SrlpView &sp, int64_t q)
{
    const SrlpMember d = sp.members[q];
    return SlpMember{sp.L + d.l_off, sp.sense + d.s_off, d.m, d.ncv, d.ncv + d.n_slack + 1};
}

// One member, the whole workgroup: the row pass over its m <= kSlpMaxRows rows (L, sense: the member's own, tight),
// then the write pass into its slots.
__device__ __forceinline__ void slp_assemble_member(const AsmSlot &mt, const AsmSlot &at, const SlpMember &sp, SlpLds &l)
{
    const float *L = sp.L;
    const int m = sp.m, ncv = sp.ncv, cols = sp.cols;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = ncv + 1;
    // ---- the row pass
    int w = 0;
    bool slack = false, art = false;
    if (tid < m) {
        w = row_word(L[(int64_t)tid * W + ncv] < 0.0f, sp.sense[tid]);              // :243
        slack = (w >> 1) != 2;
        art = row_word_artificial(w);
    }
    const unsigned long long bs = __ballot(slack), ba = __ballot(art), below = (1ull << lane) - 1ull;
    if (lane == 0) {
        l.wave_slack[wave] = __popcll(bs);
        l.wave_art[wave] = __popcll(ba);
    }
    __syncthreads();
    int slack_before = __popcll(bs & below), art_through = __popcll(ba & below) + (art ? 1 : 0), art_all = 0;
    for (int k = 0; k < kSlpThreads / 64; ++k) {
        if (k < wave) { slack_before += l.wave_slack[k]; art_through += l.wave_art[k]; }
        art_all += l.wave_art[k];
    }
    if (tid < m) {
        l.word[tid] = w;
        slp_row_columns(w, ncv, cols, slack_before, art_through, art_all, l.scol[tid], l.ab[tid]);
    }
    __syncthreads();
    // ---- the write pass
    assemble_member_lds(mt, at, m, cols, l.ab, [&](int R, int C) {
        return slp_main_elem(L + (int64_t)R * W, ncv, R < m ? l.word[R] : 0, R < m ? l.scol[R] : -1, C, cols);
    });
}

// The member the workgroup owns (blockIdx.x).  at.M == nullptr: no member has artificial rows.  Every m <= kSlpMaxRows.
template <class View, class Rows>
__global__ __launch_bounds__(kSlpThreads) void k_slp_assemble(View mt, View at, Rows sp)
{
    __shared__ SlpLds l;
    const int64_t q = blockIdx.x;
    const SlpMember rows = slp_member(sp, q);
    const SrMember dm = sb_descriptor(mt, q), da = sb_descriptor_art(at, q, dm);
    slp_assemble_member(sb_slot(mt, dm), sb_slot(at, da), rows, l);
}

namespace {
template <class View, class Rows> void slp_assemble_launch(const View &mt, const View &at, const Rows &sp, hipStream_t s)
{
    hipLaunchKernelGGL((k_slp_assemble<View, Rows>), dim3((unsigned)mt.n_lps), dim3(kSlpThreads), 0, s, mt, at, sp);
}
}  // namespace
void launch_slp_assemble(const SbView &mt, const SbView &at, const SlpView &sp, hipStream_t s) { slp_assemble_launch(mt, at, sp, s); }
void launch_slp_assemble(const SrView &mt, const SrView &at, const SrlpView &sp, hipStream_t s) { slp_assemble_launch(mt, at, sp, s); }
