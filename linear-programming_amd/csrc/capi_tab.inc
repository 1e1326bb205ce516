// capi_tab.inc -- mi355x_tab_*: create / upload / solve / two-phase / download of one tableau, streamed creation, mi355x_init.
// Part of simplex_capi.hip (ONE translation unit: included there, in this order).

extern "C" {

int mi355x_abi_version(void) { return MI355X_SIMPLEX_ABI_VERSION; }
int mi355x_device_count(void) { return device_count_checked(); }
const char *mi355x_last_error(void) { return g_err.c_str(); }
// for host_problem.cpp / mps_reader.cpp (same library, not exported)
__attribute__((visibility("hidden"))) void mi355x_set_last_error_(const char *msg) { g_err = msg ? msg : ""; }
double mi355x_epsilon(void) { return kClEpsilon; }
const char *mi355x_update_kernel_name(void) { return update_kernel_symbol(); }

int mi355x_tab_create(mi355x_tab **out, int64_t rows, int64_t cols, const double *host_matrix,
                      const int64_t *host_basis, int device)
{
    if (!host_matrix) return fail(MI_BAD_ARG, "host_matrix is NULL");
    mi355x_tab *t = nullptr;
    int rc = alloc_tab(&t, rows, cols, device);
    if (rc != MI_OK) return rc;
    rc = upload(t, host_matrix, host_basis);
    if (rc != MI_OK) { free_tab(t); return rc; }
    *out = t;
    return MI_OK;
}

// everything of a compact handle but the stored matrix itself: allocations, column maps, basis,
// zeroed padding, control block -- enqueued on the handle's stream, not waited for
static int compact_prepare(mi355x_tab **out, int64_t rows, int64_t var_count, int64_t n_stored,
                           const int64_t *stored_cols, const int64_t *host_basis, int device)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    const int64_t m = rows - 1;
    if (!stored_cols || !host_basis || m < 1 || n_stored < 1 || n_stored + m != var_count)
        return fail(MI_BAD_ARG, "compact upload needs rows >= 2 and n_stored + (rows-1) == var_count");
    std::vector<int64_t> l2p((size_t)var_count, -2);                 // -2: not yet accounted for
    for (int64_t i = 0; i < m; ++i) {
        const int64_t b = host_basis[i];
        if (b < 0 || b >= var_count || l2p[(size_t)b] != -2) return fail(MI_BAD_ARG, "bad basis entry %lld", (long long)b);
        l2p[(size_t)b] = -1;
    }
    for (int64_t j = 0; j < n_stored; ++j) {
        const int64_t g = stored_cols[j];
        if (g < 0 || g >= var_count || l2p[(size_t)g] != -2) return fail(MI_BAD_ARG, "bad stored column %lld", (long long)g);
        l2p[(size_t)g] = j;
    }
    mi355x_tab *t = nullptr;
    int rc = alloc_tab(&t, rows, var_count + 1, device, 1, /*defer_dense=*/true);
    if (rc != MI_OK) return rc;
    TabView &v = t->v;
    t->c = v;
    t->c.M = nullptr; t->c.p2l = nullptr; t->c.l2p = nullptr;
    t->c.cols = n_stored + 1;
    t->c.ld = padded_ld(n_stored + 1);
    hipError_t e = hipMalloc((void **)&t->c.M, (size_t)rows * t->c.ld * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&t->c.p2l, n_stored * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&t->c.l2p, var_count * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&t->brow, var_count * sizeof(int64_t));
    if (e == hipSuccess && t->c.ld != t->c.cols)                     // (the padding columns only)
        e = hipMemset2DAsync(t->c.M + t->c.cols, t->c.ld * sizeof(double), 0, (t->c.ld - t->c.cols) * sizeof(double),
                             rows, t->stream);
    // (pageable sources: these copies have left the host buffers when the calls return)
    if (e == hipSuccess) e = hipMemcpyAsync(t->c.p2l, stored_cols, n_stored * sizeof(int64_t), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(t->c.l2p, l2p.data(), var_count * sizeof(int64_t), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(v.basis, host_basis, m * sizeof(int64_t), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) { launch_ctl_reset(v, 0, 1, t->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);        // l2p is a local
    if (e != hipSuccess) {
        free_tab(t);
        return fail(e == hipErrorOutOfMemory ? MI_NO_MEMORY : MI_HIP_ERROR, "compact upload failed: %s", hipGetErrorString(e));
    }
    *out = t;
    return MI_OK;
}

int mi355x_tab_create_compact(mi355x_tab **out, int64_t rows, int64_t var_count, int64_t n_stored,
                              const double *host_stored, const int64_t *stored_cols,
                              const int64_t *host_basis, int device)
{
    if (out) *out = nullptr;
    if (!host_stored) return fail(MI_BAD_ARG, "host_stored is NULL");
    mi355x_tab *t = nullptr;
    int rc = compact_prepare(&t, rows, var_count, n_stored, stored_cols, host_basis, device);
    if (rc != MI_OK) return rc;
    hipError_t e = hipMemcpy2DAsync(t->c.M, t->c.ld * sizeof(double), host_stored, t->c.cols * sizeof(double),
                                    t->c.cols * sizeof(double), rows, hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) {
        free_tab(t);
        return fail(MI_HIP_ERROR, "compact upload failed: %s", hipGetErrorString(e));
    }
    t->compact = true;
    t->unit_basis = true;
    *out = t;
    return MI_OK;
}

// ---- the same with the stored matrix PRODUCED chunk by chunk (host_problem.cpp: build-tableau's rows
// are independent) into pinned staging buffers and copied while later rows are still being assembled:
// assembly, PCIe and nothing else overlap; no pageable 268 MB intermediate.  The staging pool is
// process-wide and kept (page-locking memory costs more than the copies it serves).
namespace {
// Pinned staging buffers, process-wide: a streamed build checks out what its workers need and hands
// them back, so builds on different devices run side by side (pinned host memory is not tied to a
// device).  Never freed: page-locking costs more than the copies it serves, and at library teardown
// the HIP runtime may be gone already.
struct StagePool {
    std::mutex mu;
    std::vector<double *> free_bufs;
};
StagePool *stage_pool() { static StagePool *p = new StagePool; return p; }
constexpr size_t kStageBytes = 4u << 20;
constexpr int    kStageBuffersPerWorker = 2, kStageMaxWorkers = 16;

// n buffers of kStageBytes into `out` (all or nothing)
int stage_pool_checkout(int n, std::vector<double *> &out)
{
    StagePool &sp = *stage_pool();
    std::lock_guard<std::mutex> lk(sp.mu);
    out.clear();
    while ((int)out.size() < n) {
        double *b = nullptr;
        if (!sp.free_bufs.empty()) { b = sp.free_bufs.back(); sp.free_bufs.pop_back(); }
        else {
            const hipError_t e = hipHostMalloc((void **)&b, kStageBytes);
            if (e != hipSuccess) {
                (void)hipGetLastError();              // (sticky: the caller takes the plain path and carries on)
                for (double *x : out) sp.free_bufs.push_back(x);
                out.clear();
                return fail(MI_NO_MEMORY, "hipHostMalloc(%zu) failed: %s", kStageBytes, hipGetErrorString(e));
            }
        }
        out.push_back(b);
    }
    return MI_OK;
}
void stage_pool_checkin(std::vector<double *> &bufs)
{
    StagePool &sp = *stage_pool();
    std::lock_guard<std::mutex> lk(sp.mu);
    for (double *b : bufs) sp.free_bufs.push_back(b);
    bufs.clear();
}
}  // namespace

extern "C" __attribute__((visibility("hidden")))
int mi355x_tab_create_compact_streamed_(mi355x_tab **out, int64_t rows, int64_t var_count, int64_t n_stored,
                                        const int64_t *stored_cols, const int64_t *host_basis, int device,
                                        void (*produce)(void *ctx, int64_t r0, int64_t r1, double *dst), void *ctx,
                                        int n_workers)
{
    if (out) *out = nullptr;
    if (!produce) return fail(MI_BAD_ARG, "no row producer");
    mi355x_tab *t = nullptr;
    int rc = compact_prepare(&t, rows, var_count, n_stored, stored_cols, host_basis, device);
    if (rc != MI_OK) return rc;
    const int64_t w = n_stored + 1;
    const int64_t rows_per_chunk = std::max<int64_t>(1, (int64_t)(kStageBytes / (w * sizeof(double))));
    const int64_t n_chunks = (rows + rows_per_chunk - 1) / rows_per_chunk;
    n_workers = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(n_workers, kStageMaxWorkers), n_chunks));
    std::vector<double *> stage;
    if ((size_t)w * sizeof(double) > kStageBytes ||                 // a row does not fit a staging buffer
        (rc = stage_pool_checkout(n_workers * kStageBuffersPerWorker, stage)) != MI_OK) {
        // plain path: assemble everything, one copy
        std::unique_ptr<double[]> P(new (std::nothrow) double[(size_t)rows * w]);
        if (!P) { free_tab(t); return fail(MI_NO_MEMORY, "host allocation failed"); }
        produce(ctx, 0, rows, P.get());
        hipError_t e = hipMemcpy2DAsync(t->c.M, t->c.ld * sizeof(double), P.get(), w * sizeof(double), w * sizeof(double),
                                        rows, hipMemcpyHostToDevice, t->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
        if (e != hipSuccess) { free_tab(t); return fail(MI_HIP_ERROR, "compact upload failed: %s", hipGetErrorString(e)); }
    } else {
        std::atomic<int64_t> next{0};
        std::atomic<int> failed{0};
        auto worker = [&](int wi) {
            if (hipSetDevice(device) != hipSuccess) { failed = 1; return; }
            hipStream_t cs = nullptr;
            hipEvent_t ev[kStageBuffersPerWorker] = {};
            bool used[kStageBuffersPerWorker] = {};
            if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) { failed = 1; return; }
            for (auto &e : ev) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) failed = 1;
            for (int turn = 0; !failed; ++turn) {
                const int64_t c = next.fetch_add(1);
                if (c >= n_chunks) break;
                const int b = turn % kStageBuffersPerWorker;
                double *buf = stage[(size_t)(wi * kStageBuffersPerWorker + b)];
                if (used[b] && hipEventSynchronize(ev[b]) != hipSuccess) { failed = 1; break; }   // its previous copy has left it
                const int64_t r0 = c * rows_per_chunk, r1 = std::min(rows, r0 + rows_per_chunk);
                produce(ctx, r0, r1, buf);
                if (hipMemcpy2DAsync(t->c.M + r0 * t->c.ld, t->c.ld * sizeof(double), buf, w * sizeof(double),
                                     w * sizeof(double), r1 - r0, hipMemcpyHostToDevice, cs) != hipSuccess ||
                    hipEventRecord(ev[b], cs) != hipSuccess) { failed = 1; break; }
                used[b] = true;
            }
            if (hipStreamSynchronize(cs) != hipSuccess) failed = 1;
            for (auto &e : ev) if (e) (void)hipEventDestroy(e);
            (void)hipStreamDestroy(cs);
        };
        std::vector<std::thread> pool;
        for (int k = 1; k < n_workers; ++k) pool.emplace_back(worker, k);
        worker(0);
        for (auto &th : pool) th.join();
        stage_pool_checkin(stage);
        (void)hipSetDevice(device);
        if (failed) {
            (void)hipGetLastError();
            free_tab(t);
            return fail(MI_HIP_ERROR, "streamed compact upload failed");
        }
    }
    t->compact = true;
    t->unit_basis = true;
    *out = t;
    return MI_OK;
}

// Optional: pay the one-off costs now instead of inside the first solve -- the HIP context of
// `device`, the library's code object (loaded with the first launch), the pinned staging pool of
// the streamed uploads.  Idempotent.
int mi355x_init(int device)
{
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(MI_BAD_ARG, "device %d out of range [0,%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    mi355x_tab *t = nullptr;
    const double M[6] = {1.0, 1.0, 1.0, -1.0, 0.0, 0.0};            // max x, x <= 1: [A | I | b ; -c | 0 | 0]
    const int64_t b[1] = {1};
    int64_t k = 0;
    int rc = mi355x_tab_create(&t, 2, 3, M, b, device);
    if (rc != MI_OK) return rc;
    rc = mi355x_tab_solve(t, 1, 1024.0, 0, &k);
    mi355x_tab_destroy(t);
    if (rc != MI_OPTIMAL || k != 1) return rc < 0 ? rc : fail(MI_HIP_ERROR, "warm-up solve ended with status %d after %lld pivots", rc, (long long)k);
    {
        std::vector<double *> stage;
        rc = stage_pool_checkout(kStageMaxWorkers * kStageBuffersPerWorker, stage);
        stage_pool_checkin(stage);
    }
    return rc;
}

int mi355x_tab_upload(mi355x_tab *t, const double *host_matrix, const int64_t *host_basis)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    return upload(t, host_matrix, host_basis);
}

int mi355x_tab_copy(mi355x_tab **out, const mi355x_tab *src)
{
    if (!src) return fail(MI_BAD_ARG, "src is NULL");
    if (src->v.p2l)                         // a compact column shard has no dense logical form
        return fail(MI_UNSUPPORTED, "copy-tableau of a compact column shard is not supported");
    mi355x_tab *t = nullptr;
    int rc = use_device(src);
    if (rc != MI_OK) return rc;
    rc = ensure_dense(const_cast<mi355x_tab *>(src));
    if (rc != MI_OK) return rc;
    rc = alloc_tab(&t, src->v.rows, src->v.cols, src->device);
    if (rc != MI_OK) return rc;
    hipError_t e = hipStreamSynchronize(src->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(t->v.M, src->v.M, (size_t)src->v.rows * src->v.ld * sizeof(double),
                           hipMemcpyDeviceToDevice, t->stream);
    if (e == hipSuccess && src->v.rows > 1)
        e = hipMemcpyAsync(t->v.basis, src->v.basis, (src->v.rows - 1) * sizeof(int64_t),
                           hipMemcpyDeviceToDevice, t->stream);
    if (e == hipSuccess) { launch_ctl_reset(t->v, 0, 1, t->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) { free_tab(t); return fail(MI_HIP_ERROR, "copy failed: %s", hipGetErrorString(e)); }
    *out = t;
    return MI_OK;
}

int mi355x_tab_create_synthetic(mi355x_tab **out, int64_t n_vars, int64_t n_cons, uint64_t seed,
                                int64_t col_begin, int64_t col_end, int device)
{
    if (n_vars < 1 || n_cons < 1) return fail(MI_BAD_ARG, "n_vars and n_cons must be >= 1");
    const int64_t vc = n_vars + n_cons;
    if (col_end < 0) col_end = vc;
    if (col_begin < 0 || col_begin >= col_end || col_end > vc)
        return fail(MI_BAD_ARG, "bad column slice [%lld,%lld) of %lld", (long long)col_begin,
                    (long long)col_end, (long long)vc);
    mi355x_tab *t = nullptr;
    int rc = alloc_tab(&t, n_cons + 1, (col_end - col_begin) + 1, device);
    if (rc != MI_OK) return rc;
    launch_synth_fill(t->v, n_vars, n_cons, seed, nullptr, col_begin, col_end, t->stream);
    launch_ctl_reset(t->v, 0, 1, t->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) { free_tab(t); return fail(MI_HIP_ERROR, "synthetic fill failed: %s", hipGetErrorString(e)); }
    *out = t;
    return MI_OK;
}

void mi355x_tab_destroy(mi355x_tab *t) { free_tab(t); }

int mi355x_tab_shape(const mi355x_tab *t, int64_t *rows, int64_t *cols, int64_t *ld)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (rows) *rows = t->v.rows;
    if (cols) *cols = t->v.cols;
    if (ld) *ld = t->v.ld;
    return MI_OK;
}

int mi355x_tab_layout(const mi355x_tab *t, int *compact, int64_t *stored_cols, int64_t *stored_ld)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    const TabView &v = t->compact ? t->c : t->v;
    if (compact) *compact = t->compact ? 1 : 0;
    if (stored_cols) *stored_cols = v.cols;
    if (stored_ld) *stored_ld = v.ld;
    return MI_OK;
}

int mi355x_tab_pivot(mi355x_tab *t, int64_t ec, int64_t cr)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (ec < 0 || ec >= t->v.cols || cr < 0 || cr >= t->v.rows)
        return fail(MI_BAD_ARG, "pivot (col %lld, row %lld) outside %lldx%lld", (long long)ec,
                    (long long)cr, (long long)t->v.rows, (long long)t->v.cols);
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    launch_prepare_pivot(t->v, ec, cr, t->stream);
    launch_update(t->v, 1.0, 0, t->stream);
    t->n_part = 0;
    t->unit_basis = false;                // a caller-chosen pivot may be anything
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));
    return MI_OK;
}

int mi355x_tab_price(mi355x_tab *t, int is_max, double f, int64_t *col)
{
    if (!t || !col) return fail(MI_BAD_ARG, "NULL argument");
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    launch_price_only(t->v, is_max, f, t->stream);
    HIP_TRY(hipGetLastError());
    rc = read_ctl(t);
    if (rc != MI_OK) return rc;
    *col = t->h_ctl->ec;
    return MI_OK;
}

int mi355x_tab_ratio(mi355x_tab *t, int64_t ec, double f, int64_t *row)
{
    if (!t || !row) return fail(MI_BAD_ARG, "NULL argument");
    if (ec < 0 || ec >= t->v.cols) return fail(MI_BAD_ARG, "entering column %lld out of range", (long long)ec);
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    launch_ratio_only(t->v, ec, f, t->stream);
    HIP_TRY(hipGetLastError());
    rc = read_ctl(t);
    if (rc != MI_OK) return rc;
    *row = t->h_ctl->cr;
    return MI_OK;
}

int mi355x_tab_solve_async(mi355x_tab *t, int is_max, double f, int64_t n_pivots, int reset)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (n_pivots < 0) return fail(MI_BAD_ARG, "n_pivots < 0");
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = ensure_compact(t);
    if (rc != MI_OK) return rc;
    if (reset) launch_ctl_reset(t->v, 0, 0, t->stream);
    if (resident_mode(t)) {
        // the tableau stays on chip for the whole request (one launch per 65536 pivots)
        for (int64_t left = n_pivots; left > 0; left -= 65536) {
            rc = enqueue_resident(t, is_max, f, (int)std::min<int64_t>(left, 65536));
            if (rc != MI_OK) return rc;
        }
        HIP_TRY(hipGetLastError());
        return MI_OK;
    }
    if (block_mode(t)) {
        // whole blocks, then the remainder as one shorter block (k_sweep16 for the full ones, a
        // k_sweep with as few links as the remainder needs: 20 pivots 371 us, 40 pivots 627 us), or
        // (g_tail_policy 0) the remainder spread evenly over the blocks (378 / 656 us)
        const int bk = block_size(t);
        if (bk > kMaxBlock) {
            // wide blocks: full blocks, then the remainder -- as a block of up to 16 (the sweeps of
            // short blocks) preceded by one of 16 if it is longer than that
            int64_t left = n_pivots;
            while (left > 0) {
                // (a remainder of 20 is one block too: the four-links-per-statement sweep exists for it)
                const int64_t k = left >= bk ? bk : (left == 20 ? 20 : (left > kMaxBlock ? kMaxBlock : left));
                rc = enqueue_block(t, is_max, f, (int)k);
                if (rc != MI_OK) return rc;
                left -= k;
            }
            HIP_TRY(hipGetLastError());
            return MI_OK;
        }
        const int64_t nblk = (n_pivots + bk - 1) / bk;
        for (int64_t b = 0; b < nblk; ++b) {
            int64_t k = n_pivots / nblk + (b < n_pivots % nblk ? 1 : 0);
            if (t->tn.tail_policy == 1) k = (b + 1 < nblk || n_pivots % bk == 0) ? bk : n_pivots % bk;
            rc = enqueue_block(t, is_max, f, (int)k);
            if (rc != MI_OK) return rc;
        }
        HIP_TRY(hipGetLastError());
        return MI_OK;
    }
    for (int64_t i = 0; i < n_pivots; ++i) {
        rc = enqueue_iteration(t, is_max, f);
        if (rc != MI_OK) return rc;
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

int mi355x_tab_reset(mi355x_tab *t, int64_t max_pivots)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    launch_ctl_reset(t->v, max_pivots, 0, t->stream);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

int mi355x_tab_sync(mi355x_tab *t, int64_t *n_pivots)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = read_ctl(t);
    if (rc != MI_OK) return rc;
    if (t->h_ctl->status == kSyncLost) {              // see recover_lost_exchange: the request may
        rc = recover_lost_exchange(t);                // have been cut short (fewer pivots than asked
        if (rc != MI_OK) return rc;                   // for); the count reported is what was applied
        rc = read_ctl(t);
        if (rc != MI_OK) return rc;
        if (n_pivots) *n_pivots = t->h_ctl->n_pivots;
        return MI_RUNNING;
    }
    if (n_pivots) *n_pivots = t->h_ctl->n_pivots;
    if (t->h_ctl->status == kNeedDense) {             // see fall_back_to_dense: further
        rc = fall_back_to_dense(t);                   // iterations continue on the dense tableau
        if (rc != MI_OK) return rc;
        return MI_RUNNING;
    }
    if (t->h_ctl->status == kResidentStuck)
        return fail(MI_HIP_ERROR, "the resident solve lost an exchange after its first one (hung GPU?): the tableau in HBM "
                                  "is as it was before that launch, but the request was not carried out");
    return status_to_rc(t->h_ctl->status);
}

int mi355x_tab_solve(mi355x_tab *t, int is_max, double f, int64_t max_pivots, int64_t *n_pivots)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    CancelScope cancel_scope(t);
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = ensure_compact(t);
    if (rc != MI_OK) return rc;
    launch_ctl_reset(t->v, max_pivots, 0, t->stream);
    if (resident_mode(t)) {
        // the whole solve with the tableau on chip: one launch per 65536 pivots, one read-back each
        for (;;) {
            rc = enqueue_resident(t, is_max, f, 65536);
            if (rc != MI_OK) return rc;
            HIP_TRY(hipGetLastError());
            rc = read_ctl(t);
            if (rc != MI_OK) return rc;
            const int32_t st = t->h_ctl->status;
            if (st == kRunning) {                     // (a launch ends with the tableau written back)
                if (take_cancel(t)) { if (n_pivots) *n_pivots = t->h_ctl->n_pivots; return MI_CANCELLED; }
                continue;
            }
            if (st == kSyncLost) {                    // its workgroups were not co-resident: nothing happened
                rc = recover_lost_exchange(t);
                if (rc != MI_OK) return rc;
                break;                                // the established paths below
            }
            if (st == kResidentStuck)
                return fail(MI_HIP_ERROR, "the resident solve lost an exchange after its first one (hung GPU?)");
            if (st == kNeedDense) {
                rc = fall_back_to_dense(t);           // redo that pivot, and the rest, densely (below)
                if (rc != MI_OK) return rc;
                break;
            }
            if (n_pivots) *n_pivots = t->h_ctl->n_pivots;
            return (int)st;
        }
    }
    if (block_mode(t)) {
        // blocks of g_block_k pivots, blind enqueue in growing chunks of blocks; a block whose
        // look-ahead terminates the solve still sweeps (applies what was selected before)
        int64_t blocks = 2;
        for (;;) {
            for (int64_t i = 0; i < blocks; ++i) {
                rc = enqueue_block(t, is_max, f, block_size(t));
                if (rc != MI_OK) return rc;
            }
            HIP_TRY(hipGetLastError());
            rc = read_ctl(t);
            if (rc != MI_OK) return rc;
            if (t->h_ctl->status == kSyncLost) {      // see recover_lost_exchange
                rc = recover_lost_exchange(t);
                if (rc != MI_OK) return rc;
                continue;
            }
            if (t->h_ctl->status != kRunning) break;
            // (every block ends with its sweep: the tableau is whole whenever the host looks)
            if (take_cancel(t)) { if (n_pivots) *n_pivots = t->h_ctl->n_pivots; return MI_CANCELLED; }
            if (blocks < 64) blocks *= 2;
        }
        if (t->h_ctl->status != kNeedDense) {
            if (n_pivots) *n_pivots = t->h_ctl->n_pivots;
            return (int)t->h_ctl->status;
        }
        rc = fall_back_to_dense(t);                   // redo that pivot, and the rest, densely
        if (rc != MI_OK) return rc;
    }
    // Blind enqueue in growing chunks, one status read-back per chunk.  The stream always
    // ends on a select (it is the select that detects optimality / unboundedness / the cap);
    // an update is a no-op unless the preceding select chose a pivot, so iterations enqueued
    // past termination cost a few empty launches and nothing else.
    enqueue_select(t, is_max, f);
    int64_t chunk = 16;
    for (;;) {
        for (int64_t i = 0; i < chunk; ++i) {
            rc = enqueue_update(t, is_max);
            if (rc != MI_OK) return rc;
            enqueue_select(t, is_max, f);
        }
        HIP_TRY(hipGetLastError());
        rc = read_ctl(t);
        if (rc != MI_OK) return rc;
        if (t->h_ctl->status == kNeedDense) {         // redo that pivot, and the rest, densely
            rc = fall_back_to_dense(t);
            if (rc != MI_OK) return rc;
            enqueue_select(t, is_max, f);
            continue;
        }
        if (t->h_ctl->status != kRunning) break;
        if (take_cancel(t)) {
            // the chunk ended on a select that chose a pivot (basis, column maps and pivot count
            // already say so): apply it, then the tableau is whole
            rc = enqueue_update(t, is_max);
            if (rc != MI_OK) return rc;
            HIP_TRY(hipGetLastError());
            rc = read_ctl(t);
            if (rc != MI_OK) return rc;
            if (n_pivots) *n_pivots = t->h_ctl->n_pivots;
            return MI_CANCELLED;
        }
        if (chunk < 512) chunk *= 2;
    }
    if (n_pivots) *n_pivots = t->h_ctl->n_pivots;
    return (int)t->h_ctl->status;
}

// for host_problem.cpp (same library, not exported): the two tableaux of a two-phase job look at each
// other's cancel flag for the job's lifetime; a step that ends takes its request with it
extern "C" __attribute__((visibility("hidden"))) void mi355x_tab_link_cancel_(mi355x_tab *a, mi355x_tab *b)
{
    if (a) { a->cancel_peer = b ? &b->cancel : nullptr; a->cancel_scoped_outside = b != nullptr; }
    if (b) { b->cancel_peer = a ? &a->cancel : nullptr; b->cancel_scoped_outside = a != nullptr; }
}
extern "C" __attribute__((visibility("hidden"))) void mi355x_tab_clear_cancel_(mi355x_tab *t)
{
    if (t) t->cancel.store(0, std::memory_order_release);
}

int mi355x_tab_cancel(mi355x_tab *t)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    t->cancel.store(1, std::memory_order_release);
    return MI_OK;
}

// Between the phases of n-solve-tableau (simplex.lisp:405-451), `art` holding the OPTIMAL artificial
// tableau: the feasibility test (fp= 0 objective), the drive-out pivots of artificial variables that
// are still basic (exact /= 0 tests), then rows + basis into `mt` and its objective row re-eliminated.
// *n_driveout = drive-out pivots made.  MI_OK: `mt` is ready for phase 2.
static int two_phase_handover_impl(mi355x_tab *art, mi355x_tab *mt, double f, int64_t *n_driveout)
{
    if (n_driveout) *n_driveout = 0;
    if (art->v.rows != mt->v.rows || art->v.cols < mt->v.cols || art->device != mt->device)
        return fail(MI_BAD_ARG, "artificial and main tableau do not match");
    const int64_t m = mt->v.rows - 1, num_vars = mt->v.cols - 1, num_art_vars = art->v.cols - 1;
    int rc = use_device(art);
    if (rc != MI_OK) return rc;
    rc = ensure_dense(art);                // the hand-over works on the logical tableaux
    if (rc != MI_OK) return rc;
    rc = ensure_dense(mt);
    if (rc != MI_OK) return rc;
    // (fp= 0 objective factor)                                             simplex.lisp:405-407
    double art_obj = 0.0;
    HIP_TRY(hipMemcpyAsync(&art_obj, art->v.M + m * art->v.ld + num_art_vars, sizeof(double),
                           hipMemcpyDeviceToHost, art->stream));
    HIP_TRY(hipStreamSynchronize(art->stream));
    if (!tp_feasible(art_obj, f * kClEpsilon)) return MI_INFEASIBLE;
    // degenerate artificials still basic: pivot them out               simplex.lisp:419-434
    std::vector<int64_t> basis((size_t)std::max<int64_t>(m, 1));
    if (m > 0) {
        HIP_TRY(hipMemcpyAsync(basis.data(), art->v.basis, m * sizeof(int64_t), hipMemcpyDeviceToHost,
                               art->stream));
        HIP_TRY(hipStreamSynchronize(art->stream));
    }
    rc = tp_drive_out<double>(
        m, num_vars, num_art_vars, basis.data(), [](double x) { return x == 0.0; },
        [&](int64_t i, std::vector<double> &row) { return fetch_row(art->v.M + i * art->v.ld, art->v.cols, art->stream, row); },
        [&](int64_t col, int64_t i) { return mi355x_tab_pivot(art, col, i); },
        [&] { if (n_driveout) ++*n_driveout; });
    if (rc != MI_OK) return rc;
    // copy rows + basis, re-eliminate the objective row                simplex.lisp:437-451
    HIP_TRY(hipStreamSynchronize(mt->stream));
    launch_handover(art->v, mt->v, art->unit_basis && art->tn.handover_mode != 1, art->stream);
    mt->n_part = 0;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(art->stream));
    return MI_OK;
}

int mi355x_two_phase_handover(mi355x_tab *art, mi355x_tab *mt, double f, int64_t *n_driveout)
{
    if (!art || !mt) return fail(MI_BAD_ARG, "NULL handle");
    return two_phase_handover_impl(art, mt, f, n_driveout);
}

int mi355x_solve_two_phase(mi355x_tab *art, mi355x_tab *mt, int main_is_max, double f,
                           int64_t *n_pivots)
{
    if (!art || !mt) return fail(MI_BAD_ARG, "NULL handle");
    if (art == mt) return fail(MI_BAD_ARG, "artificial and main tableau are the same handle");
    if (art->v.rows != mt->v.rows || art->v.cols < mt->v.cols || art->device != mt->device)
        return fail(MI_BAD_ARG, "artificial and main tableau do not match");
    // mi355x_tab_cancel on EITHER handle stops the call whichever phase is running: for the length of
    // the call each handle's solve loop looks at both flags, and neither phase's end clears them
    TwoPhaseCancelScope cancel_scope(art, mt);
    int64_t n1 = 0, n2 = 0, nd = 0;
    if (n_pivots) { n_pivots[0] = 0; n_pivots[1] = 0; }
    int rc = mi355x_tab_solve(art, /*is_max=*/0, f, 0, &n1);             // simplex.lisp:403
    if (n_pivots) n_pivots[0] = n1;
    if (rc != MI_OPTIMAL) return rc;
    rc = two_phase_handover_impl(art, mt, f, &nd);
    if (n_pivots) n_pivots[0] = n1 + nd;
    if (rc != MI_OK) return rc;
    // (a request that arrived between the phases)
    if (take_cancel(mt)) return MI_CANCELLED;
    rc = mi355x_tab_solve(mt, main_is_max, f, 0, &n2);                  // simplex.lisp:452
    if (n_pivots) n_pivots[1] = n2;
    return rc;
}

int mi355x_tab_download(mi355x_tab *t, double *hm, int64_t *hb, double *last_row, double *last_col)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    if (t->compact && !hm) {
        // what tableau-variable & co. need (objective row, RHS column, basis) straight from the
        // compact representation: no dense tableau is rebuilt (or even allocated)
        const TabView &c = t->c;
        const int64_t n_nb = c.cols - 1;
        if (hb && c.rows > 1)
            HIP_TRY(hipMemcpyAsync(hb, c.basis, (c.rows - 1) * sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
        if (last_col)
            HIP_TRY(hipMemcpy2DAsync(last_col, sizeof(double), c.M + n_nb, c.ld * sizeof(double),
                                     sizeof(double), c.rows, hipMemcpyDeviceToHost, t->stream));
        if (last_row) {
            std::vector<double>  obj((size_t)c.cols);
            std::vector<int64_t> p2l((size_t)std::max<int64_t>(n_nb, 1));
            HIP_TRY(hipMemcpyAsync(obj.data(), c.M + (c.rows - 1) * c.ld, c.cols * sizeof(double),
                                   hipMemcpyDeviceToHost, t->stream));
            HIP_TRY(hipMemcpyAsync(p2l.data(), c.p2l, n_nb * sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
            HIP_TRY(hipStreamSynchronize(t->stream));
            for (int64_t j = 0; j < t->v.cols; ++j) last_row[j] = 0.0;          // basic columns: +0
            for (int64_t j = 0; j < n_nb; ++j) last_row[p2l[(size_t)j]] = obj[(size_t)j];
            last_row[t->v.cols - 1] = obj[(size_t)n_nb];
        }
        HIP_TRY(hipStreamSynchronize(t->stream));
        return MI_OK;
    }
    rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    const TabView &v = t->v;
    rc = download_parts(v.M, v.ld, v.rows, v.cols, v.basis, t->stream, hm, hb, last_row, last_col);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipStreamSynchronize(t->stream));
    return MI_OK;
}

int mi355x_tab_download_block(mi355x_tab *t, int64_t row0, int64_t n_rows, int64_t col0, int64_t n_cols,
                              double *host_block)
{
    if (!t || !host_block) return fail(MI_BAD_ARG, "NULL argument");
    if (row0 < 0 || n_rows < 1 || col0 < 0 || n_cols < 1 || row0 + n_rows > t->v.rows ||
        col0 + n_cols > t->v.cols)
        return fail(MI_BAD_ARG, "block [%lld,+%lld) x [%lld,+%lld) outside %lldx%lld", (long long)row0,
                    (long long)n_rows, (long long)col0, (long long)n_cols, (long long)t->v.rows,
                    (long long)t->v.cols);
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    const TabView &v = t->v;
    HIP_TRY(hipMemcpy2DAsync(host_block, n_cols * sizeof(double), v.M + row0 * v.ld + col0,
                             v.ld * sizeof(double), n_cols * sizeof(double), n_rows,
                             hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return MI_OK;
}

int mi355x_tab_trace(mi355x_tab *t, int64_t *ecs, int64_t *crs, int64_t cap, int64_t *n)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = read_ctl(t);
    if (rc != MI_OK) return rc;
    return download_trace(t->v.trace_ec, t->v.trace_cr, t->h_ctl->trace_n, kTraceCap, t->stream, ecs, crs, cap, n);
}

int mi355x_tab_set_stream(mi355x_tab *t, void *hip_stream, int use_own)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipStreamSynchronize(t->stream));
    t->stream = use_own ? t->own_stream : (hipStream_t)hip_stream;   // NULL = HIP's null stream
    return MI_OK;
}

int mi355x_tab_timing_enable(mi355x_tab *t, int enable)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    t->timing_stride = enable > 0 ? enable : 0;
    t->update_launches = 0;
    t->n_timed_la = 0;
    return MI_OK;
}

int mi355x_tab_timing_read_kind(mi355x_tab *t, int which, int64_t *n_launches, double *sum_ms, double *min_ms)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (which != 0 && which != 1) return fail(MI_BAD_ARG, "which must be 0 (update / sweep) or 1 (look-ahead)");
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipStreamSynchronize(t->stream));
    std::vector<hipEvent_t> &a = which ? t->la0 : t->ev0, &b = which ? t->la1 : t->ev1;
    int &n = which ? t->n_timed_la : t->n_timed;
    double sum = 0.0, mn = 0.0;
    for (int i = 0; i < n; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, a[i], b[i]));
        sum += ms;
        if (i == 0 || ms < mn) mn = ms;
    }
    if (n_launches) *n_launches = n;
    if (sum_ms) *sum_ms = sum;
    if (min_ms) *min_ms = mn;
    n = 0;
    return MI_OK;
}

int mi355x_tab_timing_read(mi355x_tab *t, int64_t *n_launches, double *sum_ms, double *min_ms)
{
    return mi355x_tab_timing_read_kind(t, 0, n_launches, sum_ms, min_ms);
}

}  // extern "C"
