// capi_batch_lps.inc -- mi355x_batch_create_lps / mi355x_multibatch_create_lps: double-precision batches whose
// tableaux the device builds from the members' problem rows (build-tableau, src/simplex.lisp:243-328, as
// kernels_batch_lps.inc), and mi355x_batch_readback / mi355x_multibatch_readback: all the read-back functions
// need of every member in one copy per sub-batch.
// Part of simplex_capi.hip (ONE translation unit: included there after capi_exact_lps.inc; ensure_dense is
// capi_tab_impl.inc's, lps_check, tab_pair_build and multibatch_pair_build capi_assemble.inc's).

namespace {

// mi355x_batch_lps_timing (measurement aid): HIP events around the assembly kernels of every sub-batch built since
std::atomic<int> g_blp_timing{0};
std::mutex       g_blp_mutex;
double           g_blp_ms = 0.0;
int64_t          g_blp_n = 0;

// n members (checked) on one device: t[0] the main batch, t[1] the artificial one or NULL (tab_pair_build).  The rows,
// the senses and the kernels' scratch live on the device until the assembly is over.
int blp_build(mi355x_tab *t[2], int64_t n, int64_t m, int64_t ncv, int64_t n_eq, int64_t n_art, const double *lps,
              const int32_t *sense, int device)
{
    hipEvent_t ev[2] = {nullptr, nullptr};
    const bool timed = g_blp_timing.load(std::memory_order_relaxed) && hipSetDevice(device) == hipSuccess &&
                       hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t bL = (size_t)n * (size_t)(m + 1) * (size_t)(ncv + 1) * sizeof(double), bS = (size_t)n * (size_t)m * sizeof(int32_t);
    const size_t oS = al(bL), oX = al(oS + bS), total = al(oX + 3 * bS);
    const int rc = tab_pair_build(t, n, m + 1, ncv + (m - n_eq) + 1, n_art, device, total,
                                  [&](hipStream_t st, const TabView &mv, const TabView &av, char *p) {
        HIP_TRY(hipMemcpyAsync(p, lps, bL, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(p + oS, sense, bS, hipMemcpyHostToDevice, st));
        const BatchLpsView sp{(const double *)p, (const int32_t *)(p + oS), m, ncv, m - n_eq, n_art};
        if (timed) (void)hipEventRecord(ev[0], st);
        launch_batch_lps_assemble(mv, av, sp, (int32_t *)(p + oX), st);
        if (timed) (void)hipEventRecord(ev[1], st);
        return (int)MI_OK;
    });
    float ms = 0.0f;
    if (timed && rc == MI_OK && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) {
        std::lock_guard<std::mutex> lock(g_blp_mutex);
        g_blp_ms += ms;
        g_blp_n++;
    }
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
    return rc;
}

// one sub-batch's planes to the host: last rows (n x cols), last columns (n x rows), bases (n x (rows - 1))
int blp_readback(mi355x_tab *t, double *last_rows, double *last_cols, int64_t *bases)
{
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    const TabView &v = t->v;
    const size_t n = (size_t)v.n_lps, nr = n * (size_t)v.cols, nc = n * (size_t)v.rows, nb = n * (size_t)(v.rows - 1);
    void *mem = nullptr;
    HIP_TRY(hipMalloc(&mem, (nr + nc + nb + 1) * 8));
    std::vector<int64_t> host;
    try { host.resize(nr + nc + nb); } catch (...) { (void)hipFree(mem); return fail(MI_NO_MEMORY, "host allocation failed"); }
    double *d = (double *)mem;
    launch_batch_readback(v, d, d + nr, (int64_t *)(d + nr + nc), t->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), mem, (nr + nc + nb) * 8, hipMemcpyDeviceToHost, t->stream);
    if (e == hipSuccess) e = wait_stream(t->stream);
    (void)hipFree(mem);
    if (e != hipSuccess) return fail(MI_HIP_ERROR, "batch read-back failed: %s", hipGetErrorString(e));
    if (last_rows) memcpy(last_rows, host.data(), nr * 8);
    if (last_cols) memcpy(last_cols, host.data() + nr, nc * 8);
    if (bases && nb) memcpy(bases, host.data() + nr + nc, nb * 8);
    return MI_OK;
}

}  // namespace

extern "C" {

// build-tableau's steps :243-328 for n_lps members of one shape on `device` (what mi355x_build_tableau +
// mi355x_batch_create do on the host, per member, one or two dense matrices each)
int mi355x_batch_create_lps(mi355x_batch **out_main, mi355x_batch **out_art, int64_t n_lps, int64_t m, int64_t ncv,
                            const double *lps, const int32_t *sense, int device)
{
    if (!out_main || !out_art) return fail(MI_BAD_ARG, "out is NULL");
    *out_main = *out_art = nullptr;
    int64_t n_eq = 0, n_art = 0;
    int rc = lps_check(n_lps, 0, m, ncv, lps, sense, &n_eq, &n_art);
    if (rc != MI_OK) return rc;
    mi355x_tab *t[2];
    rc = blp_build(t, n_lps, m, ncv, n_eq, n_art, lps, sense, device);
    if (rc != MI_OK) return rc;
    mi355x_batch *b0 = batch_of(t[0]), *b1 = t[1] ? batch_of(t[1]) : nullptr;
    if (!b0 || (t[1] && !b1)) {
        free_tab(t[0]); free_tab(t[1]);
        delete b0; delete b1;
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    *out_main = b0;
    *out_art = b1;
    return MI_OK;
}

// the same over several devices: the split of mi355x_multibatch_create (:243-328 per member on its sub-batch's
// device; replaces n_lps mi355x_build_tableau calls and the upload of their matrices)
int mi355x_multibatch_create_lps(mi355x_multibatch **out_main, mi355x_multibatch **out_art, int64_t n_lps, int64_t m,
                                 int64_t ncv, const double *lps, const int32_t *sense, int n_devices, const int *device_ids)
{
    if (!out_main || !out_art) return fail(MI_BAD_ARG, "out is NULL");
    *out_main = *out_art = nullptr;
    int64_t n_eq = 0, n_art = 0;
    int rc = lps_check(n_lps, 0, m, ncv, lps, sense, &n_eq, &n_art);
    if (rc != MI_OK) return rc;
    const int64_t rows = m + 1, cols = ncv + (m - n_eq) + 1, per = rows * (ncv + 1);
    return multibatch_pair_build(out_main, out_art, n_lps, rows, cols, n_art, n_devices, device_ids,
                                 [&](mi355x_tab *t[2], int64_t k0, int64_t count, int device) {
        return blp_build(t, count, m, ncv, n_eq, n_art, lps + k0 * per, sense + k0 * m, device);
    });
}

// tableau-objective-value / tableau-variable / tableau-reduced-cost (src/simplex.lisp:74-120) read the last row, the
// last column and the basis: those of every member at once (k_batch_readback; replaces three copies per member of
// mi355x_batch_download)
int mi355x_batch_readback(mi355x_batch *b, double *last_rows, double *last_cols, int64_t *bases)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    return blp_readback(b->t, last_rows, last_cols, bases);
}

int mi355x_multibatch_readback(mi355x_multibatch *mb, double *last_rows, double *last_cols, int64_t *bases)
{
    if (!mb) return fail(MI_BAD_ARG, "handle is NULL");
    for (size_t d = 0; d < mb->sub.size(); ++d) {
        const int64_t k0 = mb->first[d];
        const int rc = blp_readback(mb->sub[d]->t, last_rows ? last_rows + k0 * mb->cols : nullptr,
                                    last_cols ? last_cols + k0 * mb->rows : nullptr, bases ? bases + k0 * (mb->rows - 1) : nullptr);
        if (rc != MI_OK) return rc;
    }
    return MI_OK;
}

// test aid (include/mi355x_simplex_tune.h): member k as stored, padding columns included
int mi355x_batch_debug_stored(mi355x_batch *b, int64_t k, double *out, int64_t *ld)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    mi355x_tab *t = b->t;
    const TabView &v = t->v;
    if (k < 0 || k >= v.n_lps) return fail(MI_BAD_ARG, "lp_index %lld out of range", (long long)k);
    if (ld) *ld = v.ld;
    if (!out) return MI_OK;
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipMemcpy2DAsync(out, v.ld * sizeof(double), v.M + k * v.rows * v.ld, v.ld * sizeof(double),
                             v.ld * sizeof(double), v.rows, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(wait_stream(t->stream));
    return MI_OK;
}

// measurement aid (include/mi355x_simplex_tune.h): device time of the assembly kernels
int mi355x_batch_lps_timing(int enable, double *sum_ms, int64_t *n_sub_batches)
{
    std::lock_guard<std::mutex> lock(g_blp_mutex);
    if (sum_ms) *sum_ms = g_blp_ms;
    if (n_sub_batches) *n_sub_batches = g_blp_n;
    g_blp_ms = 0.0; g_blp_n = 0;
    g_blp_timing.store(enable ? 1 : 0, std::memory_order_relaxed);
    return MI_OK;
}

}  // extern "C"
