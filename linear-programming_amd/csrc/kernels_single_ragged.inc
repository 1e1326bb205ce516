// kernels_single_ragged.inc -- RAGGED batches of single-float tableaux: every member has its own shape and sense, one
// workgroup still owns one member for its whole solve.  The loop is s_solve_in_lds of kernels_single.inc and the step
// between the phases (src/simplex.lisp:402-461) is sb_between_member of kernels_single_batch.inc: there is no second
// copy of either here, only the member's view (sr_member) and the member list of a launch.  A launch has ONE
// dynamic-LDS size, so the host sorts the members into occupancy classes and launches each class at its own size.
// No double appears in this file; -ffp-contract=off (a product is rounded, then the difference is rounded).
// Part of simplex_kernels.hip (ONE translation unit: included there, after kernels_single_batch.inc, inside namespace
// mi355x).

__device__ __forceinline__ SView sr_member(const SrView &b, int64_t q, const SrMember &d)
{
    SView t;
    t.M = b.M + d.m_off;
    t.ld = d.ld; t.rows = d.rows; t.cols = d.cols;
    t.basis = b.basis + d.basis_off;
    t.col = nullptr; t.prow = nullptr;                         // (the LDS forms keep both in LDS)
    t.ctl = b.ctl + q;
    t.trace_ec = b.trace_ec + q * b.trace_cap;
    t.trace_cr = b.trace_cr + q * b.trace_cap;
    t.trace_cap = b.trace_cap;
    return t;
}

// One member per workgroup: n-solve-tableau on member members[blockIdx.x] (members nullptr: the one class of all
// members, member blockIdx.x) under the member's own sense, at most `cap` pivots in this launch.  gate: as
// k_sb_solve's.  The descriptor is loaded in front of the gate and status tests, so its load is in flight beside
// theirs and a workgroup starts its tableau load after as many dependent loads as k_sb_solve's does.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_sr_solve(SrView b, const int32_t *members, float price_tol, float ratio_thr,
                                                      int cap, const int32_t *gate)
{
    const int64_t q = members ? members[blockIdx.x] : blockIdx.x;
    const SrMember d = b.members[q];
    if (gate && gate[2 * q] != 1) return;
    if (b.ctl[q].status != kRunning) return;
    s_solve_in_lds<THREADS>(sr_member(b, q, d), d.sgn, price_tol, ratio_thr, cap);
}

// Between the phases, member members[blockIdx.x] of a pair of ragged batches (the list is a class of the ARTIFICIAL
// batch: the step's LDS is never more than the artificial member's single_lds_bytes).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_sr_between(SrView ab, SrView mb, const int32_t *members, int32_t *phase,
                                                        float feasible_tol, int64_t max_pivots)
{
    const int64_t q = members ? members[blockIdx.x] : blockIdx.x;
    const SrMember da = ab.members[q], dm = mb.members[q];
    if (phase[2 * q] != 0) return;
    sb_between_member<THREADS>(sr_member(ab, q, da), sr_member(mb, q, dm), phase + 2 * q, feasible_tol, max_pivots);
}

// ------------------------------------------------------------------ host-side launchers
namespace {
template <int THREADS> bool sr_raise_t()
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sr_solve<THREADS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSingleLdsBudget);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sr_between<THREADS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSingleLdsBudget);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;
}
template <int THREADS> bool sr_occupancy_t(size_t lds, int *members_per_cu)
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_sr_solve<THREADS>, THREADS, lds) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    *members_per_cu = nb;
    return true;
}
}  // namespace
// false: the dynamic-LDS attribute of the two kernels could not be raised (once per handle, on the handle's device)
bool sragged_raise(int threads) { return threads == 256 ? sr_raise_t<256>() : sr_raise_t<1024>(); }
// workgroups of k_sr_solve resident per compute unit at this dynamic-LDS size
bool sragged_occupancy(int threads, size_t lds, int *members_per_cu)
{
    return threads == 256 ? sr_occupancy_t<256>(lds, members_per_cu) : sr_occupancy_t<1024>(lds, members_per_cu);
}
// one class: `count` members listed at `members` (device; nullptr: members 0 .. count - 1), `lds` the dynamic LDS of
// the class's largest member
void launch_sr_solve(const SrView &b, const int32_t *members, int64_t count, size_t lds, int threads, double f, int cap,
                     const int32_t *gate, hipStream_t s)
{
    const SingleThresholds th = single_thresholds(f);
    if (threads == 256)
        hipLaunchKernelGGL(k_sr_solve<256>, dim3((unsigned)count), dim3(256), lds, s, b, members, th.price, th.ratio, cap, gate);
    else
        hipLaunchKernelGGL(k_sr_solve<1024>, dim3((unsigned)count), dim3(1024), lds, s, b, members, th.price, th.ratio, cap, gate);
}
void launch_sr_between(const SrView &art, const SrView &mb, const int32_t *members, int64_t count, size_t lds, int threads,
                       int32_t *phase, double f, int64_t max_pivots, hipStream_t s)
{
    const float feasible = single_thresholds(f).feasible;
    if (threads == 256)
        hipLaunchKernelGGL(k_sr_between<256>, dim3((unsigned)count), dim3(256), lds, s, art, mb, members, phase, feasible, max_pivots);
    else
        hipLaunchKernelGGL(k_sr_between<1024>, dim3((unsigned)count), dim3(1024), lds, s, art, mb, members, phase, feasible, max_pivots);
}
