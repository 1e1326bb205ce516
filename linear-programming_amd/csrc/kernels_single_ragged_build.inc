// kernels_single_ragged_build.inc -- RAGGED batches of single-float tableaux BUILT ON THE DEVICE, from the members'
// problem rows (build-tableau, src/simplex.lisp:243-328) or from a base problem and branch-and-bound node rows
// (:214-221, :230-237), every member with its own shape, and the light read-back of a ragged batch (what
// tableau-objective-value and tableau-variable read, :74-107).
// There is no second copy of a rule here: the row pass and the write pass of a member from rows are
// slp_assemble_member (kernels_single_lps.inc), those of a node sbb_assemble_member (kernels_single_bb.inc), both
// around assemble_member_lds (kernels_assemble.inc).  This file only says where a ragged member lives (sr_slot) and
// where its input does (the descriptors).  A descriptor is wave-uniform and loaded once at the top of a kernel, so it
// and everything derived from it stay in scalar registers.
// No double appears in this file; it holds no product (-ffp-contract=off as in its siblings); every store is a plain
// C++ store.
// Part of simplex_kernels.hip (ONE translation unit: included there after kernels_single_lps.inc, inside namespace
// mi355x).

// where member `d` of a ragged batch lives (b.M == nullptr: there is no such batch)
__device__ __forceinline__ AsmSlot sr_slot(const SrView &b, const SrMember &d)
{
    return AsmSlot{b.M ? b.M + d.m_off : nullptr, b.basis + d.basis_off, (int)d.ld, (int)d.cols};
}

// Member blockIdx.x from its rows.  at.M == nullptr: no member has artificial rows.  Every m <= kSlpMaxRows.
__global__ __launch_bounds__(kSlpThreads) void k_srlp_assemble(SrView mt, SrView at, const float *L, const int32_t *sense,
                                                               const SrlpMember *members)
{
    __shared__ SlpLds l;
    const int64_t q = blockIdx.x;
    const SrlpMember sp = members[q];
    const SrMember dm = mt.members[q];
    SrMember da = dm;
    if (at.M) da = at.members[q];
    slp_assemble_member(sr_slot(mt, dm), sr_slot(at, da), L + sp.l_off, sense + sp.s_off, sp.m, sp.ncv,
                        sp.ncv + sp.n_slack + 1, l);
}

// Node blockIdx.x of its own depth.  at.M == nullptr: no node has artificial rows.  Dynamic LDS: sbb_assemble_lds of
// the create's largest member.
__global__ __launch_bounds__(kSbbThreads) void k_srbb_assemble(SrView mt, SrView at, SbbBaseView b, const int64_t *var,
                                                               const int32_t *sense, const int64_t *bound, const SrbbNode *nodes)
{
    extern __shared__ __attribute__((aligned(16))) int32_t srbb_lds[];
    const int64_t q = blockIdx.x;
    const SrbbNode nd = nodes[q];
    const SrMember dm = mt.members[q];
    SrMember da = dm;
    if (at.M) da = at.members[q];
    sbb_assemble_member(sr_slot(mt, dm), sr_slot(at, da), b, var + nd.off, sense + nd.off, bound + nd.off, nd.d, srbb_lds);
}

// Member blockIdx.x: its last column at rhs + (the rows of the members before it), its last row at obj + col_off[q],
// its basis at basis + (their rows - 1) -- three concatenated planes.
__global__ __launch_bounds__(kSbbThreads) void k_sr_readback(SrView v, const int64_t *col_off, float *rhs, float *obj,
                                                             int64_t *basis)
{
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const SrMember d = v.members[q];
    const int64_t R = d.rows, C = d.cols, m = R - 1, co = col_off[q];
    const float *M = v.M + d.m_off;
    for (int64_t i = tid; i < R; i += kSbbThreads) rhs[d.basis_off + q + i] = M[i * d.ld + C - 1];
    for (int64_t j = tid; j < C; j += kSbbThreads) obj[co + j] = M[m * d.ld + j];
    for (int64_t i = tid; i < m; i += kSbbThreads) basis[d.basis_off + i] = v.basis[d.basis_off + i];
}

void launch_srlp_assemble(const SrView &mt, const SrView &at, const float *L, const int32_t *sense, const SrlpMember *members,
                          hipStream_t s)
{
    hipLaunchKernelGGL(k_srlp_assemble, dim3((unsigned)mt.n_lps), dim3(kSlpThreads), 0, s, mt, at, L, sense, members);
}
void launch_srbb_assemble(const SrView &mt, const SrView &at, const SbbBaseView &b, const int64_t *var, const int32_t *sense,
                          const int64_t *bound, const SrbbNode *nodes, size_t lds, hipStream_t s)
{
    hipLaunchKernelGGL(k_srbb_assemble, dim3((unsigned)mt.n_lps), dim3(kSbbThreads), lds, s, mt, at, b, var, sense, bound, nodes);
}
void launch_sr_readback(const SrView &v, const int64_t *col_off, float *rhs, float *obj, int64_t *basis, hipStream_t s)
{
    hipLaunchKernelGGL(k_sr_readback, dim3((unsigned)v.n_lps), dim3(kSbbThreads), 0, s, v, col_off, rhs, obj, basis);
}
