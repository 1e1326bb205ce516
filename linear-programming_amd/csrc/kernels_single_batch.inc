// kernels_single_batch.inc -- BATCHES of single-float tableaux, of one shape (SbView) or RAGGED (SrView: every member
// its own shape and sense): one workgroup owns one member for its whole solve.  The loop is s_solve_in_lds of
// kernels_single.inc (the member's tableau, pivot row and column snapshot in LDS), so a member ends with exactly what
// k_s_solve gives it alone; between the phases of a two-phase pair one workgroup per member does
// src/simplex.lisp:405-451 in the order of capi_single.inc's stab_handover.  A launch has ONE dynamic-LDS size, so
// the host sorts the members of a ragged batch into occupancy classes and launches each class at its own size.
// No double appears in this file; -ffp-contract=off (a product is rounded, then the difference is rounded).
// Part of simplex_kernels.hip (ONE translation unit: included there, after kernels_single.inc, inside namespace mi355x).

// ---- the member view: what a kernel asks of a batch, said ONCE, as overloads on SbView (a batch of one shape: the
// descriptor is computed, sb_descriptor of simplex_kernels.h) and SrView (a ragged batch: one load of members[q]).
// Every kernel of the family is a template over the view and is instantiated for the forms that exist.
// which member the workgroup owns: blockIdx.x, or through the member list of an occupancy class (ragged batches)
__device__ __forceinline__ int64_t sb_owned(const SbView &, const int32_t *) { return blockIdx.x; }
__device__ __forceinline__ int64_t sb_owned(const SrView &, const int32_t *members)
{
    return members ? members[blockIdx.x] : blockIdx.x;
}
// (wave-uniform and loaded once at the top of a kernel: it and everything derived from it stay in scalar registers)
__device__ __forceinline__ SrMember sb_descriptor(const SrView &b, int64_t q) { return b.members[q]; }
// the artificial batch's descriptor beside the main batch's dm (at.M == nullptr: no such batch, nothing is loaded)
template <class View>
__device__ __forceinline__ SrMember sb_descriptor_art(const View &at, int64_t q, const SrMember &dm)
{
    SrMember d = dm;
    if (at.M) d = sb_descriptor(at, q);
    return d;
}
// the sense a member is solved under: the call's, or the ragged member's own
__device__ __forceinline__ float sb_sense(const SbView &, const SrMember &, float call_sgn) { return call_sgn; }
__device__ __forceinline__ float sb_sense(const SrView &, const SrMember &d, float) { return d.sgn; }
template <class View>
__device__ __forceinline__ SView sb_member(const View &b, int64_t q, const SrMember &d)
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
// where the assemblies write member `d` (AsmSlot, kernels_assemble.inc; b.M == nullptr: there is no such batch)
template <class View>
__device__ __forceinline__ AsmSlot sb_slot(const View &b, const SrMember &d)
{
    return AsmSlot{b.M ? b.M + d.m_off : nullptr, b.basis + d.basis_off, (int)d.ld, (int)d.cols};
}

// What a call arms: the members it carries on (left unfinished by a cancel, or stopped by the cap of an earlier call)
// start the call's pivot count at zero under the call's cap; a finished member is not touched.  phase: nullptr, or
// the two-phase state of the pair -- want_phase 0 arms the artificial members still in phase 1 (an OPTIMAL one
// included: it is priced again, makes no pivot and goes through the step between the phases), want_phase 1 the main
// members that were handed over in an earlier call.
__global__ __launch_bounds__(256) void k_sb_begin(Ctl *ctl, int64_t n_lps, int64_t max_pivots, const int32_t *phase, int want_phase)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_lps) return;
    if (phase && phase[2 * q] != want_phase) return;
    const int32_t st = ctl[q].status;
    if (st == kRunning || st == 3 || (phase && want_phase == 0 && st == 0)) {
        ctl[q].status = kRunning;
        ctl[q].n_pivots = 0;
        ctl[q].max_pivots = max_pivots;
    }
}

// One member per workgroup: n-solve-tableau on the member the workgroup owns (members: the list of a ragged batch's
// occupancy class, or nullptr) under the view's sense, at most `cap` pivots in this launch.  Loop: where the member's
// tableau lives during the solve (SolveInLds; SolveInHbm of kernels_single_global.inc).
// gate: nullptr, or the two-phase state of the pair this batch is the main batch of -- a member runs once handed over.
// The descriptor comes in front of the gate and status tests: a ragged batch's load of it is in flight beside theirs,
// so a workgroup starts its tableau load after as many dependent loads as that of a batch of one shape, which loads
// nothing here.
struct SolveInLds {
    template <int THREADS>
    static __device__ __forceinline__ void run(const SView &t, float sgn, float price_tol, float ratio_thr, int cap)
    {
        s_solve_in_lds<THREADS>(t, sgn, price_tol, ratio_thr, cap);
    }
};
template <int THREADS, class View, class Loop>
__global__ __launch_bounds__(THREADS) void k_sb_solve(View b, float sgn, float price_tol, float ratio_thr, int cap,
                                                      const int32_t *gate, const int32_t *members)
{
    const int64_t q = sb_owned(b, members);
    const SrMember d = sb_descriptor(b, q);
    if (gate && gate[2 * q] != 1) return;
    if (b.ctl[q].status != kRunning) return;
    Loop::template run<THREADS>(sb_member(b, q, d), sb_sense(b, d, sgn), price_tol, ratio_thr, cap);
}

// Between the phases (src/simplex.lisp:405-451), member blockIdx.x of a pair of batches, in global memory; for every
// member in phase 1 whose artificial tableau is OPTIMAL.  The operations and their order are stab_handover's:
// (fp= 0 objective), the drive-out pivots for i ascending (exact /= 0 tests, the lowest non-basic column, the forced
// n-pivot-row recorded in the member's trace and counted in phase 1), the copy, the basis, the objective-row
// elimination sequential in i (every column sees the reference's operation sequence), the cap that is left for
// phase 2.  phase[2q] becomes 1 (handed over) or 2 (ended here, phase[2q+1] = MI_INFEASIBLE / MI_ART_NONZERO /
// MI_ART_STUCK).  Dynamic LDS: a basic-column flag per main column, a row (pivot row, then the objective row) and the
// column snapshot -- never more than the artificial shape's single_lds_bytes.
// The body is sb_between_member; phase_q: the member's two entries of the pair's state.
template <int THREADS>
__device__ __forceinline__ void sb_between_member(const SView &a, const SView &mt, int32_t *phase_q, float feasible_tol,
                                                  int64_t max_pivots)
{
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    __shared__ int s_best;
    if (a.ctl->status != 0) return;
    const int rows = (int)a.rows, m = rows - 1, acols = (int)a.cols, nav = acols - 1, nv = (int)mt.cols - 1;
    const int ldl = (acols + 3) / 4 * 4;
    int   *flag = reinterpret_cast<int *>(s_lds);             // nv <= ldl entries
    float *prow = s_lds + ldl;                                 // ldl
    float *col  = prow + ldl;                                  // rows
    float *A = a.M;
    const int64_t ald = a.ld, mld = mt.ld;
    const int tid = threadIdx.x;

    const float art_obj = A[(int64_t)m * ald + nav];
    const float diff = 0.0f - art_obj;
    if (!((diff < 0.0f ? -diff : diff) <= feasible_tol)) {
        if (tid == 0) { phase_q[0] = 2; phase_q[1] = 2; }              // MI_INFEASIBLE
        return;
    }
    for (int j = tid; j < nv; j += THREADS) flag[j] = 0;
    __syncthreads();
    for (int i = tid; i < m; i += THREADS) {
        const int64_t bc = a.basis[i];
        if (bc >= 0 && bc < nv) flag[bc] = 1;
    }
    __syncthreads();
    int64_t n = a.ctl->n_pivots, trace_n = a.ctl->trace_n;      // (every thread: read before thread 0 writes them back)
    for (int i = 0; i < m; ++i) {
        if (a.basis[i] < nv) continue;
        if (A[(int64_t)i * ald + nav] != 0.0f) {
            if (tid == 0) {
                a.ctl->n_pivots = n; a.ctl->trace_n = trace_n;
                phase_q[0] = 2; phase_q[1] = 4;                         // MI_ART_NONZERO
            }
            return;
        }
        if (tid == 0) s_best = nv;
        __syncthreads();
        int mine = nv;
        for (int j = tid; j < nv; j += THREADS)
            if (A[(int64_t)i * ald + j] != 0.0f && !flag[j]) { mine = j; break; }
        if (mine < nv) atomicMin(&s_best, mine);
        __syncthreads();
        const int ec = s_best;
        if (ec >= nv) {
            if (tid == 0) {
                a.ctl->n_pivots = n; a.ctl->trace_n = trace_n;
                phase_q[0] = 2; phase_q[1] = 5;                         // MI_ART_STUCK
            }
            return;
        }
        // the forced n-pivot-row (src/simplex.lisp:337-359): column snapshot, prow = row / pivot, then the update
        const float piv = A[(int64_t)i * ald + ec];
        for (int r = tid; r < rows; r += THREADS) col[r] = A[(int64_t)r * ald + ec];
        for (int c = tid; c < acols; c += THREADS) prow[c] = A[(int64_t)i * ald + c] / piv;
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const float s = col[r];
            for (int c = tid; c < acols; c += THREADS) {
                const float p = prow[c];
                const float prod = s * p;                                       // rounded product ...
                const float o = A[(int64_t)r * ald + c] - prod;                 // ... then the rounded difference
                A[(int64_t)r * ald + c] = (r == i) ? p : o;
            }
        }
        if (tid == 0) {
            a.basis[i] = ec;
            flag[ec] = 1;
            if (trace_n < a.trace_cap) { a.trace_ec[trace_n] = ec; a.trace_cr[trace_n] = i; }
            a.ctl->ec = ec; a.ctl->cr = i;
        }
        ++n; ++trace_n;
        __syncthreads();
    }
    // the copy (:437-441) and the basis; the objective row goes through LDS
    for (int r = 0; r < m; ++r)
        for (int c = tid; c <= nv; c += THREADS)
            mt.M[(int64_t)r * mld + c] = A[(int64_t)r * ald + (c < nv ? c : nav)];
    for (int i = tid; i < m; i += THREADS) mt.basis[i] = a.basis[i];
    float *obj = prow;
    for (int c = tid; c <= nv; c += THREADS) obj[c] = mt.M[(int64_t)m * mld + c];
    __syncthreads();
    for (int i = 0; i < m; ++i) {                                               // :444-451, sequential in i
        const float scale = obj[a.basis[i]];
        __syncthreads();                                                        // every thread has read the scale
        if (scale != 0.0f) {
            const float *ri = mt.M + (int64_t)i * mld;
            for (int c = tid; c <= nv; c += THREADS) {
                const float prod = scale * ri[c];
                obj[c] = obj[c] - prod;
            }
        }
        __syncthreads();
    }
    for (int c = tid; c <= nv; c += THREADS) mt.M[(int64_t)m * mld + c] = obj[c];
    if (tid == 0) {
        a.ctl->status = 0;                                                      // phase 1 ended MI_OPTIMAL
        a.ctl->n_pivots = n; a.ctl->trace_n = trace_n;
        // mi355x_stab_solve_two_phase: MI_MAX_PIVOTS once phase 1 and the drive-outs used the cap up, else what is left
        Ctl *mc = mt.ctl;
        mc->n_pivots = 0;
        if (max_pivots > 0 && n >= max_pivots) { mc->status = 3; mc->max_pivots = max_pivots; }
        else { mc->status = kRunning; mc->max_pivots = max_pivots > 0 ? max_pivots - n : 0; }
        phase_q[0] = 1; phase_q[1] = 0;
    }
}
// members: a class of the ARTIFICIAL batch (the step's LDS is never more than the artificial member's single_lds_bytes)
template <int THREADS, class View>
__global__ __launch_bounds__(THREADS) void k_sb_between(View ab, View mb, const int32_t *members, int32_t *phase,
                                                        float feasible_tol, int64_t max_pivots)
{
    const int64_t q = sb_owned(ab, members);
    const SrMember da = sb_descriptor(ab, q), dm = sb_descriptor(mb, q);
    if (phase[2 * q] != 0) return;
    sb_between_member<THREADS>(sb_member(ab, q, da), sb_member(mb, q, dm), phase + 2 * q, feasible_tol, max_pivots);
}

// ------------------------------------------------------------------ host-side launchers
// The ONE rule: which workgroup a batch of this shape takes.  Four 256-thread members fit a CU where one 1024-thread
// member does, so small members take 256 threads; beyond kSbatchQuads1024 stored quads a member would take 1024
// (measured: no shape inside the LDS budget is there, simplex_kernels.h).
int sbatch_threads_for(int64_t rows, int64_t cols)
{
    return rows * ((cols + 3) / 4) <= kSbatchQuads1024 ? 256 : 1024;
}
size_t sbatch_lds_bytes(const SbView &b)
{
    SView t{};
    t.rows = b.rows; t.cols = b.cols;
    return single_lds_bytes(t);
}
namespace {
// threads -> the instantiation, decided HERE for every kernel of the family: f(std::integral_constant<int, THREADS>)
template <class F> auto sb_by_threads(int threads, F f)
{
    return threads == 256 ? f(std::integral_constant<int, 256>{}) : f(std::integral_constant<int, 1024>{});
}
// The solve kernel of (View, Loop) and the step between the phases of View.  raise: their dynamic-LDS attribute goes up
// to the budget; members_per_cu (may be nullptr): the solve kernel's resident workgroups per compute unit at `lds`.
template <class View, class Loop> bool sb_kernel_attributes(int threads, bool raise, size_t lds, int *members_per_cu)
{
    return sb_by_threads(threads, [&](auto T) {
        constexpr int THREADS = decltype(T)::value;
        hipError_t e = hipSuccess;
        if (raise) {
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sb_solve<THREADS, View, Loop>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSingleLdsBudget);
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sb_between<THREADS, View>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSingleLdsBudget);
        }
        int nb = 0;
        if (e == hipSuccess && members_per_cu)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_sb_solve<THREADS, View, Loop>, THREADS, lds);
        if (e != hipSuccess) { (void)hipGetLastError(); return false; }
        if (members_per_cu) *members_per_cu = nb;
        return true;
    });
}
// `count` workgroups: the members listed at `members` (device; nullptr: members 0 .. count - 1), `lds` bytes each
template <class View, class Loop>
void sb_solve_launch(const View &b, const int32_t *members, int64_t count, size_t lds, int threads, int is_max, double f,
                     int cap, const int32_t *gate, hipStream_t s)
{
    const SingleThresholds th = single_thresholds(f);
    sb_by_threads(threads, [&](auto T) {
        constexpr int THREADS = decltype(T)::value;
        hipLaunchKernelGGL((k_sb_solve<THREADS, View, Loop>), dim3((unsigned)count), dim3(THREADS), lds, s, b,
                           s_sgn_of(is_max), th.price, th.ratio, cap, gate, members);
        return 0;
    });
}
template <class View>
void sb_between_launch(const View &art, const View &mb, const int32_t *members, int64_t count, size_t lds, int threads,
                       int32_t *phase, double f, int64_t max_pivots, hipStream_t s)
{
    const float feasible = single_thresholds(f).feasible;
    sb_by_threads(threads, [&](auto T) {
        constexpr int THREADS = decltype(T)::value;
        hipLaunchKernelGGL((k_sb_between<THREADS, View>), dim3((unsigned)count), dim3(THREADS), lds, s, art, mb, members,
                           phase, feasible, max_pivots);
        return 0;
    });
}
}  // namespace
// false: the shape does not fit the budget, or the attribute could not be raised (create declines the shape)
bool sbatch_available(const SbView &b, int threads, int *members_per_cu)
{
    const size_t lds = sbatch_lds_bytes(b);
    if (lds > kSingleLdsBudget || b.cols < 2) return false;
    return sb_kernel_attributes<SbView, SolveInLds>(threads, true, lds, members_per_cu);
}
// false: the dynamic-LDS attribute of the two kernels could not be raised (once per handle, on the handle's device)
bool sragged_raise(int threads) { return sb_kernel_attributes<SrView, SolveInLds>(threads, true, 0, nullptr); }
// workgroups of the ragged solve kernel resident per compute unit at this dynamic-LDS size
bool sragged_occupancy(int threads, size_t lds, int *members_per_cu)
{
    return sb_kernel_attributes<SrView, SolveInLds>(threads, false, lds, members_per_cu);
}
void launch_sb_ctl_reset(const SbView &b, hipStream_t s)
{
    hipLaunchKernelGGL(k_ctl_reset, dim3((unsigned)b.n_lps), dim3(1), 0, s, b.ctl, (int64_t)0, 1);
}
void launch_sb_begin(const SbView &b, int64_t max_pivots, const int32_t *phase, int want_phase, hipStream_t s)
{
    hipLaunchKernelGGL(k_sb_begin, dim3((unsigned)((b.n_lps + 255) / 256)), dim3(256), 0, s, b.ctl, b.n_lps, max_pivots,
                       phase, want_phase);
}
void launch_sb_solve(const SbView &b, int threads, int is_max, double f, int cap, const int32_t *gate, hipStream_t s)
{
    sb_solve_launch<SbView, SolveInLds>(b, nullptr, b.n_lps, sbatch_lds_bytes(b), threads, is_max, f, cap, gate, s);
}
void launch_sb_between(const SbView &art, const SbView &mb, int threads, int32_t *phase, double f, int64_t max_pivots, hipStream_t s)
{
    sb_between_launch(art, mb, nullptr, art.n_lps, sbatch_lds_bytes(art), threads, phase, f, max_pivots, s);
}
// a ragged batch, one occupancy class: `count` members listed at `members` (device; nullptr: members 0 .. count - 1),
// `lds` the dynamic LDS of the class's largest member; the sense is each member's own
void launch_sb_solve(const SrView &b, const int32_t *members, int64_t count, size_t lds, int threads, double f, int cap,
                     const int32_t *gate, hipStream_t s)
{
    sb_solve_launch<SrView, SolveInLds>(b, members, count, lds, threads, /*is_max=*/0, f, cap, gate, s);
}
void launch_sb_between(const SrView &art, const SrView &mb, const int32_t *members, int64_t count, size_t lds, int threads,
                       int32_t *phase, double f, int64_t max_pivots, hipStream_t s)
{
    sb_between_launch(art, mb, members, count, lds, threads, phase, f, max_pivots, s);
}
