// capi_single_lps.inc -- mi355x_sbatch_create_lps: batches of single-float LPs whose tableaux the device builds from
// the members' problem rows (build-tableau, src/simplex.lisp:243-328, under Lisp's int / single-float contagion:
// kernels_single_lps.inc).  Part of simplex_capi.hip (ONE translation unit: included there after capi_single_bb.inc;
// the handle, sb_pair_build and SbDeviceMem are capi_single_batch.inc's, kSbbExactInts capi_single_bb.inc's, lps_check
// capi_assemble.inc's).
//
// A zero in a negated row is read as Lisp's INTEGER zero and comes out +0.0; a single-float zero the user wrote
// there would come out -0.0, and this entry cannot tell the two apart: the caller keeps such members out
// (single_lps.py: "float zero").
//
// The guard.  Lisp sums the artificial objective row (:302-316) with integers exact among themselves; the kernel
// sums floats.  The two agree when every integer partial sum is exact in a float, which holds while the sum of the
// absolute values of a column's integer entries is at most 2^24.  The caller hands in that sum per member and
// column (col_int_sum, over the constraint rows); a member with a column beyond 2^24 declines the call
// (MI_UNSUPPORTED): the host builds those members itself.

namespace {

// The guard of one member from rows (sums: its ncv + 1 column sums; see the head of this file), with its message
int slp_guard(int64_t q, int64_t ncv, const double *sums)
{
    for (int64_t c = 0; c <= ncv; ++c)
        if (!(sums[c] <= kSbbExactInts))
            return fail(MI_UNSUPPORTED, "member %lld: the integer entries of column %lld sum beyond 2^24: the float "
                        "sum of the artificial objective row would not be the reference's", (long long)q, (long long)c);
    return MI_OK;
}

// mi355x_sbatch_lps_global_timing (measurement aid): HIP events around the three passes of the global form's assembly
std::atomic<int> g_slpg_timing{0};
std::mutex       g_slpg_mutex;
double           g_slpg_ms[3] = {0.0, 0.0, 0.0};                            // the last timed create: rows, write, objective row

// mi355x_sbatch_create_lps / _create_lps_global: the checks, the guard, the pair of the form, the assembly
int slp_create(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n_lps, int64_t m, int64_t ncv, const float *lps,
               const int32_t *sense, const double *col_int_sum, int device, int form)
{
    if (!out_main || !out_art) return fail(MI_BAD_ARG, "out is NULL");
    *out_main = *out_art = nullptr;
    int64_t n_eq = 0, n_art = 0;
    int rc = lps_check(n_lps, 30, m, ncv, lps, sense, &n_eq, &n_art);
    if (rc != MI_OK) return rc;
    for (int64_t q = 0; col_int_sum && q < n_lps; ++q)                      // the guard (NULL: no entry is an integer)
        if (slp_guard(q, ncv, col_int_sum + q * (ncv + 1)) != MI_OK) return MI_UNSUPPORTED;
    const int64_t rows = m + 1, cols = ncv + (m - n_eq) + 1;
    if (form == kSbFormLds && m > kSlpMaxRows)                              // (no tableau of so many rows fits the budget)
        return fail(MI_UNSUPPORTED, "a %lldx%lld single-float member does not fit the LDS budget of %lld bytes",
                    (long long)rows, (long long)cols, (long long)kSingleLdsBudget);
    SbDeviceMem d;                                                          // rows, senses, the global form's scratch planes
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timed = form == kSbFormGlobal && g_slpg_timing.load(std::memory_order_relaxed);
    rc = sb_pair_build(out_main, out_art, n_lps, rows, cols, n_art, device, "assembly from rows",
                         [&](hipStream_t s, const SbView &mv, const SbView &av) {
        const size_t bL = (size_t)n_lps * (size_t)rows * (size_t)(ncv + 1) * sizeof(float), bS = (size_t)n_lps * (size_t)m * sizeof(int32_t);
        const size_t oS = sb_align(bL), oW = sb_align(oS + bS);
        hipError_t e = hipMalloc(&d.mem, form == kSbFormGlobal ? oW + sga_lps_scratch_bytes(n_lps, m) : oS + bS);
        const float *dL = (const float *)d.mem;
        const int32_t *dS = (const int32_t *)((const char *)d.mem + oS);
        if (e == hipSuccess) e = hipMemcpyAsync(d.mem, lps, bL, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync((char *)d.mem + oS, sense, bS, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            const SlpView sp{dL, dS, m, ncv, m - n_eq, n_art};
            for (int k = 0; k < 4 && timed; ++k) timed = hipEventCreate(&ev[k]) == hipSuccess;
            if (form == kSbFormGlobal) launch_sga_lps(mv, av, sp, (int32_t *)((char *)d.mem + oW), s, timed ? ev : nullptr);
            else launch_slp_assemble(mv, av, sp, s);
        }
        return e;
    }, form);
    if (rc == MI_OK && timed) {                                              // (sb_pair_build has waited for the stream)
        std::lock_guard<std::mutex> lock(g_slpg_mutex);
        for (int k = 0; k < 3; ++k) {
            float ms = 0.0f;
            g_slpg_ms[k] = hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess ? (double)ms : -1.0;
        }
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

}  // namespace

extern "C" {

int mi355x_sbatch_create_lps(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n_lps, int64_t m, int64_t ncv,
                             const float *lps, const int32_t *sense, const double *col_int_sum, int device)
{
    return slp_create(out_main, out_art, n_lps, m, ncv, lps, sense, col_int_sum, device, kSbFormLds);
}

int mi355x_sbatch_create_lps_global(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n_lps, int64_t m, int64_t ncv,
                                    const float *lps, const int32_t *sense, const double *col_int_sum, int device)
{
    return slp_create(out_main, out_art, n_lps, m, ncv, lps, sense, col_int_sum, device, kSbFormGlobal);
}

// measurement aid (include/mi355x_simplex_tune.h)
int mi355x_sbatch_lps_global_timing(int enable, double *rows_ms, double *write_ms, double *objective_ms)
{
    std::lock_guard<std::mutex> lock(g_slpg_mutex);
    if (rows_ms) *rows_ms = g_slpg_ms[0];
    if (write_ms) *write_ms = g_slpg_ms[1];
    if (objective_ms) *objective_ms = g_slpg_ms[2];
    g_slpg_timing.store(enable ? 1 : 0, std::memory_order_relaxed);
    return MI_OK;
}

// test aid (include/mi355x_simplex_tune.h): member k as stored, padding columns included
int mi355x_sbatch_debug_stored(mi355x_sbatch *b, int64_t k, float *out, int64_t *ld)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    const SbView &v = b->v;
    if (k < 0 || k >= v.n_lps) return fail(MI_BAD_ARG, "lp_index %lld out of range", (long long)k);
    const SrMember d = sb_host_member(b, k);
    if (ld) *ld = d.ld;
    if (!out) return MI_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpyAsync(out, v.M + d.m_off, (size_t)(d.rows * d.ld) * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return MI_OK;
}

}  // extern "C"
