// capi_single_lps.inc -- mi355x_sbatch_create_lps: batches of single-float LPs whose tableaux the device builds from
// the members' problem rows (build-tableau, src/simplex.lisp:243-328, under Lisp's int / single-float contagion:
// kernels_single_lps.inc).  Part of simplex_capi.hip (ONE translation unit: included there after capi_single_bb.inc;
// the handle, sb_new, sb_fresh_ctl and free_sbatch are capi_single_batch.inc's, kSbbExactInts capi_single_bb.inc's).
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

// the argument checks (no device is looked for): the numbers of `=` rows and of artificial rows every member has.
// O(m) per member: only the signs of the right-hand sides are read.
int slp_check(int64_t n_lps, int64_t m, int64_t ncv, const float *lps, const int32_t *sense, int64_t *n_eq_out,
              int64_t *n_art_out)
{
    if (!lps) return fail(MI_BAD_ARG, "lps is NULL");
    if (!sense) return fail(MI_BAD_ARG, "sense is NULL");
    if (n_lps < 1 || n_lps > (1LL << 30)) return fail(MI_BAD_ARG, "n_lps=%lld must be in [1, 2^30]", (long long)n_lps);
    if (m < 1 || ncv < 1) return fail(MI_BAD_ARG, "m=%lld ncv=%lld must be >= 1", (long long)m, (long long)ncv);
    if (m > (1 << 24) || ncv > (1 << 24)) return fail(MI_BAD_ARG, "m=%lld ncv=%lld out of range", (long long)m, (long long)ncv);
    const int64_t W = ncv + 1, per = (m + 1) * W;
    int64_t n_eq = -1, n_art = -1;
    for (int64_t q = 0; q < n_lps; ++q) {
        int64_t e = 0, a = 0;
        for (int64_t i = 0; i < m; ++i) {
            const int32_t s = sense[q * m + i];
            if (s < 0 || s > 2) return fail(MI_BAD_ARG, "member %lld: sense %d of row %lld", (long long)q, (int)s, (long long)i);
            const bool flip = lps[q * per + i * W + ncv] < 0.0f;             // :243-252
            e += s == 2;
            a += s == 2 || (flip ? 1 - s : s) == 1;
        }
        if (n_eq >= 0 && (e != n_eq || a != n_art))
            return fail(MI_BAD_ARG, "member %lld has %lld `=` and %lld artificial rows, the members before it %lld and %lld",
                        (long long)q, (long long)e, (long long)a, (long long)n_eq, (long long)n_art);
        n_eq = e; n_art = a;
    }
    *n_eq_out = n_eq; *n_art_out = n_art;
    return MI_OK;
}

// the members' rows and senses on the device (one allocation), freed with the scope
struct SlpRows {
    void *mem = nullptr;
    ~SlpRows() { (void)hipFree(mem); }
};

}  // namespace

extern "C" {

int mi355x_sbatch_create_lps(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n_lps, int64_t m, int64_t ncv,
                             const float *lps, const int32_t *sense, const double *col_int_sum, int device)
{
    if (!out_main || !out_art) return fail(MI_BAD_ARG, "out is NULL");
    *out_main = *out_art = nullptr;
    int64_t n_eq = 0, n_art = 0;
    int rc = slp_check(n_lps, m, ncv, lps, sense, &n_eq, &n_art);
    if (rc != MI_OK) return rc;
    if (col_int_sum)                                                        // the guard (NULL: no entry is an integer)
        for (int64_t q = 0; q < n_lps; ++q)
            for (int64_t c = 0; c <= ncv; ++c)
                if (!(col_int_sum[q * (ncv + 1) + c] <= kSbbExactInts))
                    return fail(MI_UNSUPPORTED, "member %lld: the integer entries of column %lld sum beyond 2^24: the float "
                                "sum of the artificial objective row would not be the reference's", (long long)q, (long long)c);
    const int64_t rows = m + 1, cols = ncv + (m - n_eq) + 1;
    if (m > kSlpMaxRows)                                                    // (no tableau of so many rows fits the budget)
        return fail(MI_UNSUPPORTED, "a %lldx%lld single-float member does not fit the LDS budget of %lld bytes",
                    (long long)rows, (long long)cols, (long long)kSingleLdsBudget);
    mi355x_sbatch *mt = nullptr, *art = nullptr;
    // (the larger shape first: a pair the budget declines allocates nothing)
    if (n_art) rc = sb_new(&art, n_lps, rows, cols + n_art, device, /*zero_padding=*/false);
    if (rc == MI_OK) rc = sb_new(&mt, n_lps, rows, cols, device, /*zero_padding=*/false);
    auto undo = [&](int code) { free_sbatch(mt); free_sbatch(art); return code; };
    if (rc != MI_OK) return undo(rc);
    SlpRows d;
    const size_t bL = (size_t)n_lps * (size_t)rows * (size_t)(ncv + 1) * sizeof(float), bS = (size_t)n_lps * (size_t)m * sizeof(int32_t);
    hipStream_t s = mt->stream;
    const size_t oS = (bL + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(&d.mem, oS + bS);
    const float *dL = (const float *)d.mem;
    const int32_t *dS = (const int32_t *)((const char *)d.mem + oS);
    if (e == hipSuccess) e = hipMemcpyAsync(d.mem, lps, bL, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync((char *)d.mem + oS, sense, bS, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        launch_slp_assemble(mt->v, art ? art->v : SbView{}, SlpView{dL, dS, m, ncv, m - n_eq, n_art}, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = sb_fresh_ctl(mt);                              // (waits for the assembly as well: `d` may go)
    if (e == hipSuccess && art) e = sb_fresh_ctl(art);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return undo(fail(e == hipErrorOutOfMemory ? MI_NO_MEMORY : MI_HIP_ERROR, "assembly from rows failed: %s", hipGetErrorString(e)));
    }
    *out_main = mt;
    *out_art = art;
    return MI_OK;
}

// test aid (include/mi355x_simplex_tune.h): member k as stored, padding columns included
int mi355x_sbatch_debug_stored(mi355x_sbatch *b, int64_t k, float *out, int64_t *ld)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    const SbView &v = b->v;
    if (k < 0 || k >= v.n_lps) return fail(MI_BAD_ARG, "lp_index %lld out of range", (long long)k);
    if (ld) *ld = v.ld;
    if (!out) return MI_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpyAsync(out, v.M + k * v.stride, (size_t)v.stride * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return MI_OK;
}

}  // extern "C"
