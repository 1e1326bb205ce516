// capi_single.inc -- mi355x_stab_*: one SINGLE-FLOAT tableau behind a handle (kernels_single.inc).  The reference's
// single-float path: IEEE binary32 arithmetic and single-float-epsilon thresholds (src/utils.lisp:84-124).  No double
// touches a tableau entry here either: uploads and downloads are float copies, the hand-over's scans and the
// objective-row elimination are float operations in the reference's order on downloaded rows.
// Part of simplex_capi.hip (ONE translation unit: included there, in this order).

namespace {
int g_single_form = 0;                    // tuning / test hook: 0 auto (LDS when it fits the budget), 1 pair, 2 LDS
constexpr int64_t kSingleLdAlign = 32;    // floats: rows start on 128-byte boundaries
}  // namespace

struct mi355x_stab {
    int         device = 0;
    SView       v{};
    hipStream_t stream = nullptr;
    bool        lds = false;              // the form this handle's solves take: k_s_solve (else k_s_select + k_s_update)
    Ctl         h_ctl{};
    bool        handed_over = false;      // artificial tableau of a two-phase pair: the hand-over has been made
};

namespace {

void free_stab(mi355x_stab *t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    (void)hipFree(t->v.M);
    (void)hipFree(t->v.basis);
    (void)hipFree(t->v.col);
    (void)hipFree(t->v.prow);
    (void)hipFree(t->v.ctl);
    (void)hipFree(t->v.trace_ec);
    (void)hipFree(t->v.trace_cr);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}

int stab_read_ctl(mi355x_stab *t)
{
    HIP_TRY(hipMemcpyAsync(&t->h_ctl, t->v.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return MI_OK;
}

int stab_use(const mi355x_stab *t)
{
    HIP_TRY(hipSetDevice(t->device));
    return MI_OK;
}

// n-pivot-row with a caller-chosen pivot: k_prepare_pivot's float twin, then k_s_update
int stab_forced_pivot(mi355x_stab *t, int64_t ec, int64_t cr)
{
    launch_s_prepare_pivot(t->v, ec, cr, t->stream);
    launch_s_update(t->v, t->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    return MI_OK;
}

}  // namespace

extern "C" {

/* single-float-epsilon, exactly, as a double */
double mi355x_epsilon_single(void) { return (double)kClEpsilonSingle; }

int mi355x_stab_create(mi355x_stab **out, int64_t rows, int64_t cols, const float *matrix_rowmajor,
                       const int64_t *basis, int device)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (!matrix_rowmajor) return fail(MI_BAD_ARG, "matrix_rowmajor is NULL");
    if (rows < 1 || cols < 1) return fail(MI_BAD_ARG, "rows=%lld cols=%lld must be >= 1", (long long)rows, (long long)cols);
    if (rows > 65535LL * 16) return fail(MI_BAD_ARG, "rows=%lld exceeds the supported 1048560", (long long)rows);
    if (cols > (1LL << 30)) return fail(MI_BAD_ARG, "cols=%lld exceeds the supported 2^30", (long long)cols);
    if (rows > 1 && !basis) return fail(MI_BAD_ARG, "basis is NULL");
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(MI_BAD_ARG, "device %d out of range [0,%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    mi355x_stab *t = new (std::nothrow) mi355x_stab;
    if (!t) return fail(MI_NO_MEMORY, "host allocation failed");
    t->device = device;
    SView &v = t->v;
    v.rows = rows;
    v.cols = cols;
    v.ld = (cols + kSingleLdAlign - 1) / kSingleLdAlign * kSingleLdAlign;
    v.trace_cap = kTraceCap;
    const int64_t nb = std::max<int64_t>(rows - 1, 1);
    hipError_t e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&v.M, (size_t)rows * v.ld * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&v.basis, nb * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&v.col, (size_t)(rows + 3) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&v.prow, (size_t)v.ld * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&v.ctl, sizeof(Ctl));
    if (e == hipSuccess) e = hipMalloc((void **)&v.trace_ec, kTraceCap * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&v.trace_cr, kTraceCap * sizeof(int64_t));
    if (e == hipSuccess && v.ld != v.cols) e = hipMemsetAsync(v.M, 0, (size_t)rows * v.ld * sizeof(float), t->stream);
    if (e == hipSuccess) e = hipMemsetAsync(v.prow, 0, (size_t)v.ld * sizeof(float), t->stream);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(v.M, v.ld * sizeof(float), matrix_rowmajor, cols * sizeof(float), cols * sizeof(float), rows,
                             hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess && rows > 1) e = hipMemcpyAsync(v.basis, basis, (rows - 1) * sizeof(int64_t), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) { launch_s_ctl_reset(v, 0, 1, t->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        free_stab(t);
        return fail(e == hipErrorOutOfMemory ? MI_NO_MEMORY : MI_HIP_ERROR, "single-float tableau upload failed: %s", hipGetErrorString(e));
    }
    // the form: LDS when the stored bytes plus scratch fit the budget (and the kernel may have them), else the pair
    t->lds = g_single_form != 1 && single_lds_available(v);
    *out = t;
    return MI_OK;
}

void mi355x_stab_destroy(mi355x_stab *t) { free_stab(t); }

int mi355x_stab_info(const mi355x_stab *t, int64_t *rows, int64_t *cols, int64_t *ld, int *form, int64_t *lds_budget_bytes)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (rows) *rows = t->v.rows;
    if (cols) *cols = t->v.cols;
    if (ld) *ld = t->v.ld;
    if (form) *form = t->lds ? 2 : 1;
    if (lds_budget_bytes) *lds_budget_bytes = (int64_t)kSingleLdsBudget;
    return MI_OK;
}

int mi355x_stab_price(mi355x_stab *t, int is_max, double f, int64_t *col)
{
    if (!t || !col) return fail(MI_BAD_ARG, "NULL argument");
    int rc = stab_use(t);
    if (rc != MI_OK) return rc;
    launch_s_price_only(t->v, is_max, f, t->stream);
    HIP_TRY(hipGetLastError());
    rc = stab_read_ctl(t);
    if (rc != MI_OK) return rc;
    *col = t->h_ctl.ec;
    return MI_OK;
}

int mi355x_stab_ratio(mi355x_stab *t, int64_t ec, double f, int64_t *row)
{
    if (!t || !row) return fail(MI_BAD_ARG, "NULL argument");
    if (ec < 0 || ec >= t->v.cols) return fail(MI_BAD_ARG, "entering column %lld out of range", (long long)ec);
    int rc = stab_use(t);
    if (rc != MI_OK) return rc;
    launch_s_ratio_only(t->v, ec, f, t->stream);
    HIP_TRY(hipGetLastError());
    rc = stab_read_ctl(t);
    if (rc != MI_OK) return rc;
    *row = t->h_ctl.cr;
    return MI_OK;
}

int mi355x_stab_pivot(mi355x_stab *t, int64_t ec, int64_t cr)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (ec < 0 || ec >= t->v.cols || cr < 0 || cr >= t->v.rows)
        return fail(MI_BAD_ARG, "pivot (col %lld, row %lld) outside %lldx%lld", (long long)ec, (long long)cr,
                    (long long)t->v.rows, (long long)t->v.cols);
    int rc = stab_use(t);
    if (rc != MI_OK) return rc;
    return stab_forced_pivot(t, ec, cr);
}

int mi355x_stab_solve(mi355x_stab *t, int is_max, double f, int64_t max_pivots, int64_t *n_pivots)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    int rc = stab_use(t);
    if (rc != MI_OK) return rc;
    launch_s_ctl_reset(t->v, max_pivots, 0, t->stream);
    if (t->lds) {
        // the whole loop with the tableau in LDS: bounded launches, one status read-back each
        do {
            launch_s_solve(t->v, is_max, f, kSingleLaunchCap, t->stream);
            HIP_TRY(hipGetLastError());
            rc = stab_read_ctl(t);
            if (rc != MI_OK) return rc;
        } while (t->h_ctl.status == kRunning);
    } else {
        // blind enqueue in growing chunks, one status read-back per chunk; the stream always ends on a select,
        // and an update is a no-op unless the preceding select chose a pivot (mi355x_tab_solve's loop)
        launch_s_select(t->v, is_max, f, t->stream);
        int64_t chunk = 16;
        for (;;) {
            for (int64_t i = 0; i < chunk; ++i) {
                launch_s_update(t->v, t->stream);
                launch_s_select(t->v, is_max, f, t->stream);
            }
            HIP_TRY(hipGetLastError());
            rc = stab_read_ctl(t);
            if (rc != MI_OK) return rc;
            if (t->h_ctl.status != kRunning) break;
            if (chunk < 512) chunk *= 2;
        }
    }
    if (n_pivots) *n_pivots = t->h_ctl.n_pivots;
    return (int)t->h_ctl.status;
}

// Between the phases (src/simplex.lisp:405-451), `art` holding the OPTIMAL artificial tableau: (fp= 0 objective) with
// single-float-epsilon, the drive-out pivots (exact /= 0 tests at :423, :427), the copy (:437-441), the basis and the
// objective-row elimination (:444-451: sequential in i, every decf a rounded float product and a rounded float
// difference) on the downloaded rows.
static int stab_handover(mi355x_stab *art, mi355x_stab *mt, double f, int64_t *n_driveout)
{
    *n_driveout = 0;
    const SView &a = art->v, &mv = mt->v;
    const int64_t m = mv.rows - 1, nv = mv.cols - 1, nav = a.cols - 1;
    float art_obj = 0.0f;
    HIP_TRY(hipMemcpyAsync(&art_obj, a.M + m * a.ld + nav, sizeof(float), hipMemcpyDeviceToHost, art->stream));
    HIP_TRY(hipStreamSynchronize(art->stream));
    if (!tp_feasible(art_obj, single_thresholds(f).feasible)) return MI_INFEASIBLE;
    std::vector<int64_t> basis((size_t)std::max<int64_t>(m, 1));
    if (m > 0) {
        HIP_TRY(hipMemcpyAsync(basis.data(), a.basis, m * sizeof(int64_t), hipMemcpyDeviceToHost, art->stream));
        HIP_TRY(hipStreamSynchronize(art->stream));
    }
    const int rc = tp_drive_out<float>(
        m, nv, nav, basis.data(), [](float x) { return x == 0.0f; },
        [&](int64_t i, std::vector<float> &row) { return fetch_row(a.M + i * a.ld, a.cols, art->stream, row); },
        [&](int64_t col, int64_t i) { return stab_forced_pivot(art, col, i); }, [&] { ++*n_driveout; });
    if (rc != MI_OK) return rc;
    HIP_TRY(hipStreamSynchronize(mt->stream));
    launch_s_handover_copy(a, mv, art->stream);
    HIP_TRY(hipGetLastError());
    if (m > 0) HIP_TRY(hipMemcpyAsync(mv.basis, a.basis, m * sizeof(int64_t), hipMemcpyDeviceToDevice, art->stream));
    std::vector<float> H((size_t)mv.rows * mv.cols);
    HIP_TRY(hipMemcpy2DAsync(H.data(), mv.cols * sizeof(float), mv.M, mv.ld * sizeof(float), mv.cols * sizeof(float), mv.rows,
                             hipMemcpyDeviceToHost, art->stream));
    HIP_TRY(hipStreamSynchronize(art->stream));
    float *obj = H.data() + (size_t)m * mv.cols;
    for (int64_t i = 0; i < m; ++i) {
        const float scale = obj[basis[i]];
        if (scale != 0.0f) {
            const float *ri = H.data() + (size_t)i * mv.cols;
            for (int64_t c = 0; c <= nv; ++c) {
                const float prod = scale * ri[c];              // rounded product ...
                obj[c] = obj[c] - prod;                        // ... then the rounded difference (-ffp-contract=off)
            }
        }
    }
    HIP_TRY(hipMemcpyAsync(mv.M + m * mv.ld, obj, mv.cols * sizeof(float), hipMemcpyHostToDevice, art->stream));
    HIP_TRY(hipStreamSynchronize(art->stream));
    return MI_OK;
}

// n-solve-tableau's two-phase branch (src/simplex.lisp:402-452) in single-float, resumable: max_pivots (0: none)
// caps the pivots of THIS call, both phases and the drive-out pivots together; a call that ends with MI_MAX_PIVOTS is
// continued by the next one on the same pair, and the calls together make the pivots of one long call.
// pivots_out[0]: phase 1 + drive-outs, pivots_out[1]: phase 2, of this call.
int mi355x_stab_solve_two_phase(mi355x_stab *art, mi355x_stab *mt, int main_is_max, double f, int64_t max_pivots,
                                int64_t *pivots_out)
{
    if (!art || !mt) return fail(MI_BAD_ARG, "NULL handle");
    if (art == mt) return fail(MI_BAD_ARG, "artificial and main tableau are the same handle");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    if (art->v.rows != mt->v.rows || art->v.cols < mt->v.cols || art->device != mt->device)
        return fail(MI_BAD_ARG, "artificial and main tableau do not match");
    if (pivots_out) { pivots_out[0] = 0; pivots_out[1] = 0; }
    int rc = stab_use(art);
    if (rc != MI_OK) return rc;
    int64_t n1 = 0, n2 = 0, nd = 0;
    if (!art->handed_over) {
        rc = mi355x_stab_solve(art, /*is_max=*/0, f, max_pivots, &n1);          // simplex.lisp:403
        if (pivots_out) pivots_out[0] = n1;
        if (rc != MI_OPTIMAL) return rc;
        rc = stab_handover(art, mt, f, &nd);
        n1 += nd;
        if (pivots_out) pivots_out[0] = n1;
        if (rc != MI_OK) return rc;
        art->handed_over = true;
        if (max_pivots > 0 && n1 >= max_pivots) return MI_MAX_PIVOTS;
    }
    rc = mi355x_stab_solve(mt, main_is_max, f, max_pivots > 0 ? max_pivots - n1 : 0, &n2);   // simplex.lisp:452
    if (pivots_out) pivots_out[1] = n2;
    return rc;
}

int mi355x_stab_download(mi355x_stab *t, float *hm, int64_t *hb, float *last_row, float *last_col)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = stab_use(t);
    if (rc != MI_OK) return rc;
    const SView &v = t->v;
    rc = download_parts(v.M, v.ld, v.rows, v.cols, v.basis, t->stream, hm, hb, last_row, last_col);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipStreamSynchronize(t->stream));
    return MI_OK;
}

int mi355x_stab_trace(mi355x_stab *t, int64_t *ecs, int64_t *crs, int64_t cap, int64_t *n)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = stab_use(t);
    if (rc != MI_OK) return rc;
    rc = stab_read_ctl(t);
    if (rc != MI_OK) return rc;
    return download_trace(t->v.trace_ec, t->v.trace_cr, t->h_ctl.trace_n, kTraceCap, t->stream, ecs, crs, cap, n);
}

// measurement (tools/single_rate.py): the forced pivot (ec, cr) prepared once, then k_s_update launched `reps` times
// between two events -- *avg_ms per launch; *bytes = what one launch reads and writes (rows x ld floats each way).
// The tableau is left as the repeated updates made it.
int mi355x_stab_debug_update_time(mi355x_stab *t, int64_t ec, int64_t cr, int reps, double *avg_ms, int64_t *bytes)
{
    if (!t || !avg_ms) return fail(MI_BAD_ARG, "NULL argument");
    if (ec < 0 || ec >= t->v.cols || cr < 0 || cr >= t->v.rows || reps < 1) return fail(MI_BAD_ARG, "bad pivot or reps");
    int rc = stab_use(t);
    if (rc != MI_OK) return rc;
    hipEvent_t a = nullptr, b = nullptr;
    HIP_TRY(hipEventCreate(&a));
    hipError_t e = hipEventCreate(&b);
    if (e == hipSuccess) {
        launch_s_prepare_pivot(t->v, ec, cr, t->stream);
        launch_s_update(t->v, t->stream);                      // warm
        e = hipEventRecord(a, t->stream);
    }
    for (int i = 0; i < reps && e == hipSuccess; ++i) launch_s_update(t->v, t->stream);
    if (e == hipSuccess) e = hipEventRecord(b, t->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    if (e != hipSuccess) return fail(MI_HIP_ERROR, "timing k_s_update failed: %s", hipGetErrorString(e));
    *avg_ms = (double)ms / reps;
    if (bytes) *bytes = 2 * t->v.rows * t->v.ld * (int64_t)sizeof(float);
    return MI_OK;
}

int mi355x_tune_set_single_form(int form)
{
    if (form < 0 || form > 2) return fail(MI_BAD_ARG, "form must be 0 (auto), 1 (pair) or 2 (LDS)");
    g_single_form = form;
    return MI_OK;
}

}  // extern "C"
