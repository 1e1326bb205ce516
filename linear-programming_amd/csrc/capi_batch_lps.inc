// capi_batch_lps.inc -- mi355x_batch_create_lps / mi355x_multibatch_create_lps: double-precision batches whose
// tableaux the device builds from the members' problem rows (build-tableau, src/simplex.lisp:243-328, as
// kernels_batch_lps.inc), and mi355x_batch_readback / mi355x_multibatch_readback: all the read-back functions
// need of every member in one copy per sub-batch.
// Part of simplex_capi.hip (ONE translation unit: included there after capi_exact_lps.inc; alloc_tab, free_tab,
// ensure_dense are capi_tab_impl.inc's, mb_layout and mb_free capi_batch.inc's).

namespace {

// the argument checks of both create entries (no device is looked for): the numbers of `=` rows and of artificial
// rows every member has.  O(m) per member: only the signs of the right-hand sides are read.
int blp_check(int64_t n_lps, int64_t m, int64_t ncv, const double *lps, const int32_t *sense, int64_t *n_eq_out,
              int64_t *n_art_out)
{
    if (!lps) return fail(MI_BAD_ARG, "lps is NULL");
    if (!sense) return fail(MI_BAD_ARG, "sense is NULL");
    if (n_lps < 1) return fail(MI_BAD_ARG, "n_lps=%lld must be >= 1", (long long)n_lps);
    if (m < 1 || ncv < 1) return fail(MI_BAD_ARG, "m=%lld ncv=%lld must be >= 1", (long long)m, (long long)ncv);
    if (m > (1 << 24) || ncv > (1 << 24)) return fail(MI_BAD_ARG, "m=%lld ncv=%lld out of range", (long long)m, (long long)ncv);
    const int64_t W = ncv + 1, per = (m + 1) * W;
    int64_t n_eq = -1, n_art = -1;
    for (int64_t q = 0; q < n_lps; ++q) {
        int64_t e = 0, a = 0;
        for (int64_t i = 0; i < m; ++i) {
            const int32_t s = sense[q * m + i];
            if (s < 0 || s > 2) return fail(MI_BAD_ARG, "member %lld: sense %d of row %lld", (long long)q, (int)s, (long long)i);
            const bool flip = lps[q * per + i * W + ncv] < 0.0;              // :243-252
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

// mi355x_batch_lps_timing (measurement aid): HIP events around the assembly kernels of every sub-batch built since
std::atomic<int> g_blp_timing{0};
std::mutex       g_blp_mutex;
double           g_blp_ms = 0.0;
int64_t          g_blp_n = 0;

// n members (checked) on one device: t[0] the main batch, t[1] the artificial one or NULL, both in the state
// upload() leaves.  The rows, the senses and the kernels' scratch live on the device until the assembly is over.
int blp_build(mi355x_tab *t[2], int64_t n, int64_t m, int64_t ncv, int64_t n_eq, int64_t n_art, const double *lps,
              const int32_t *sense, int device)
{
    t[0] = t[1] = nullptr;
    const int64_t rows = m + 1, cols = ncv + (m - n_eq) + 1;
    int rc = alloc_tab(&t[0], rows, cols, device, n);
    if (rc == MI_OK && n_art) rc = alloc_tab(&t[1], rows, cols + n_art, device, n);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t bL = (size_t)n * (size_t)rows * (size_t)(ncv + 1) * sizeof(double), bS = (size_t)n * (size_t)m * sizeof(int32_t);
    const size_t oS = al(bL), oX = al(oS + bS), total = al(oX + 3 * bS);
    void *mem = nullptr;
    hipError_t e = hipSuccess;
    if (rc == MI_OK) e = hipMalloc(&mem, total);
    hipEvent_t ev[2] = {nullptr, nullptr};
    const bool timed = rc == MI_OK && g_blp_timing.load(std::memory_order_relaxed) &&
                       hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    // alloc_tab left memsets of the artificial batch's basis and control blocks on ITS stream; the assembly below
    // writes both from the main batch's stream, so those memsets have to be over first (capi_bb.inc)
    if (rc == MI_OK && e == hipSuccess && t[1]) e = hipStreamSynchronize(t[1]->stream);
    if (rc == MI_OK && e == hipSuccess) {
        char *p = (char *)mem;
        hipStream_t st = t[0]->stream;
        e = hipMemcpyAsync(p, lps, bL, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(p + oS, sense, bS, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            TabView none{};
            const BatchLpsView sp{(const double *)p, (const int32_t *)(p + oS), m, ncv, m - n_eq, n_art};
            if (timed) (void)hipEventRecord(ev[0], st);
            launch_batch_lps_assemble(t[0]->v, t[1] ? t[1]->v : none, sp, (int32_t *)(p + oX), st);
            if (timed) (void)hipEventRecord(ev[1], st);
            launch_ctl_reset(t[0]->v, 0, 1, st);
            if (t[1]) launch_ctl_reset(t[1]->v, 0, 1, st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);          // (the caller's arrays and `mem` may go)
    }
    float ms = 0.0f;
    if (timed && rc == MI_OK && e == hipSuccess && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) {
        std::lock_guard<std::mutex> lock(g_blp_mutex);
        g_blp_ms += ms;
        g_blp_n++;
    }
    for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x);
    if (mem) (void)hipFree(mem);
    if (rc == MI_OK && e != hipSuccess)
        rc = fail(e == hipErrorOutOfMemory ? MI_NO_MEMORY : MI_HIP_ERROR, "assembly from rows failed: %s", hipGetErrorString(e));
    if (rc != MI_OK) {
        free_tab(t[0]); free_tab(t[1]);
        t[0] = t[1] = nullptr;
        return rc;
    }
    for (int w = 0; w < 2 && t[w]; ++w) {
        // what upload() leaves behind: the dense logical tableau, defined by the caller
        t[w]->n_part = 0; t[w]->compact = false; t[w]->compact_failed = false; t[w]->unit_basis = false;
    }
    return MI_OK;
}

mi355x_batch *blp_wrap(mi355x_tab *t)
{
    mi355x_batch *b = new (std::nothrow) mi355x_batch;
    if (b) b->t = t;
    return b;
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
    int rc = blp_check(n_lps, m, ncv, lps, sense, &n_eq, &n_art);
    if (rc != MI_OK) return rc;
    mi355x_tab *t[2];
    rc = blp_build(t, n_lps, m, ncv, n_eq, n_art, lps, sense, device);
    if (rc != MI_OK) return rc;
    mi355x_batch *b0 = blp_wrap(t[0]), *b1 = t[1] ? blp_wrap(t[1]) : nullptr;
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
    int rc = blp_check(n_lps, m, ncv, lps, sense, &n_eq, &n_art);
    if (rc != MI_OK) return rc;
    const int64_t rows = m + 1, cols = ncv + (m - n_eq) + 1, per = rows * (ncv + 1);
    mi355x_multibatch *mb[2] = {new (std::nothrow) mi355x_multibatch, n_art ? new (std::nothrow) mi355x_multibatch : nullptr};
    auto cleanup = [&](int code) { mb_free(mb[0]); mb_free(mb[1]); return code; };
    if (!mb[0] || (n_art && !mb[1])) return cleanup(fail(MI_NO_MEMORY, "host allocation failed"));
    std::vector<int> devs;
    int nd = n_devices;
    rc = mb_layout(mb[0], n_lps, rows, cols, &nd, device_ids, devs);
    if (rc == MI_OK && mb[1]) { int nd2 = n_devices; std::vector<int> dv2; rc = mb_layout(mb[1], n_lps, rows, cols + n_art, &nd2, device_ids, dv2); }
    if (rc != MI_OK) return cleanup(rc);
    std::vector<int64_t> f2;
    for (int s = 0; s < nd; ++s) {
        const int64_t k0 = mb[0]->first[(size_t)s], k1 = mb[0]->first[(size_t)s + 1];
        if (k1 <= k0) continue;                                   // (an empty sub-batch: first[] keeps only the boundaries in use)
        mi355x_tab *t[2];
        rc = blp_build(t, k1 - k0, m, ncv, n_eq, n_art, lps + k0 * per, sense + k0 * m, devs[(size_t)s]);
        if (rc != MI_OK) return cleanup(rc);
        for (int w = 0; w < 2 && t[w]; ++w) {
            mi355x_batch *bt = blp_wrap(t[w]);
            if (!bt) { free_tab(t[w]); rc = fail(MI_NO_MEMORY, "host allocation failed"); continue; }
            mb[w]->sub.push_back(bt);
        }
        if (rc != MI_OK) return cleanup(rc);
        f2.push_back(k0);
    }
    f2.push_back(n_lps);
    mb[0]->first = f2;
    if (mb[1]) mb[1]->first = f2;
    *out_main = mb[0];
    *out_art = mb[1];
    return MI_OK;
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
