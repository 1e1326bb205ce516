// capi_batch.inc -- mi355x_batch_* and mi355x_multibatch_*: batches of independent LPs on one device and over several, incl. the two-phase pair of batches.
// Part of simplex_capi.hip (ONE translation unit: included there, in this order).

extern "C" {

// ---- batches of independent LPs ---------------------------------------------------------
// The LPs of a batch share one shape and live stacked in one allocation; every kernel of the
// single-tableau path runs unchanged with grid.z = LP index, so the whole batch advances one
// simplex iteration per (select, update) launch pair and finished LPs simply stop.
int mi355x_batch_create(mi355x_batch **out, int64_t n_lps, int64_t rows, int64_t cols,
                        const double *host_matrices, const int64_t *host_bases, int device)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (!host_matrices) return fail(MI_BAD_ARG, "host_matrices is NULL");
    mi355x_tab *t = nullptr;
    int rc = alloc_tab(&t, rows, cols, device, n_lps);
    if (rc != MI_OK) return rc;
    rc = upload(t, host_matrices, host_bases);
    if (rc != MI_OK) { free_tab(t); return rc; }
    mi355x_batch *b = new (std::nothrow) mi355x_batch;
    if (!b) { free_tab(t); return fail(MI_NO_MEMORY, "host allocation failed"); }
    b->t = t;
    *out = b;
    return MI_OK;
}

int mi355x_batch_create_synthetic(mi355x_batch **out, int64_t n_lps, int64_t n_vars, int64_t n_cons,
                                  const uint64_t *seeds, int device)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (!seeds || n_vars < 1 || n_cons < 1) return fail(MI_BAD_ARG, "bad arguments");
    mi355x_tab *t = nullptr;
    int rc = alloc_tab(&t, n_cons + 1, n_vars + n_cons + 1, device, n_lps);
    if (rc != MI_OK) return rc;
    uint64_t *dseeds = nullptr;
    hipError_t e = hipMalloc((void **)&dseeds, n_lps * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemcpyAsync(dseeds, seeds, n_lps * sizeof(uint64_t), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) {
        launch_synth_fill(t->v, n_vars, n_cons, 0, dseeds, 0, n_vars + n_cons, t->stream);
        launch_ctl_reset(t->v, 0, 1, t->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    (void)hipFree(dseeds);
    if (e != hipSuccess) { free_tab(t); return fail(MI_HIP_ERROR, "synthetic batch fill failed: %s", hipGetErrorString(e)); }
    mi355x_batch *b = new (std::nothrow) mi355x_batch;
    if (!b) { free_tab(t); return fail(MI_NO_MEMORY, "host allocation failed"); }
    b->t = t;
    *out = b;
    return MI_OK;
}

int mi355x_batch_prepare(mi355x_batch *b)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    int rc = use_device(b->t);
    if (rc != MI_OK) return rc;
    rc = ensure_compact(b->t);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipStreamSynchronize(b->t->stream));
    return MI_OK;
}

int mi355x_batch_solve(mi355x_batch *b, int is_max, double f, int64_t max_pivots, int32_t *status,
                       int64_t *n_pivots)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    mi355x_tab *t = b->t;
    CancelScope cancel_scope(t);
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    const int64_t n = t->v.n_lps;
    rc = ensure_compact(t);
    if (rc != MI_OK) return rc;
    launch_ctl_reset(t->v, max_pivots, 0, t->stream);
    if (resident_mode(t)) {
        // every LP on chip, a few workgroups each, all LPs in one launch (they progress and finish
        // independently); whatever that launch could not finish continues on the paths below
        for (;;) {
            rc = enqueue_resident(t, is_max, f, 65536);
            if (rc != MI_OK) return rc;
            HIP_TRY(hipGetLastError());
            { const int rc_ = read_ctls(t, n); if (rc_ != MI_OK) return rc_; }
            bool running = false, other = false, lost = false;
            for (int64_t i = 0; i < n; ++i) {
                const int32_t st = t->h_ctl[i].status;
                if (st == kResidentStuck) return fail(MI_HIP_ERROR, "the resident solve lost an exchange after its first one (hung GPU?)");
                running |= st == kRunning;
                lost |= st == kSyncLost;
                other |= st == kNeedDense;
            }
            if (lost) {                               // some LP's workgroups were not co-resident
                rc = recover_lost_exchange(t);
                if (rc != MI_OK) return rc;
                break;
            }
            if (other) break;                         // an LP met an inf / NaN: the established path takes it
            if (running) {
                if (take_cancel(t)) return batch_report(t, status, n_pivots, MI_CANCELLED);
                continue;
            }
            for (int64_t i = 0; i < n; ++i) {
                if (status) status[i] = t->h_ctl[i].status;
                if (n_pivots) n_pivots[i] = t->h_ctl[i].n_pivots;
            }
            return MI_OK;
        }
    }
    // preferred: one launch, one workgroup per LP (k_batch_solve); lockstep launch pairs when
    // an LP is too large for the LDS budget (or when forced by the tuning hook)
    // measured (257x769 LPs, compact representation): one workgroup per LP 1.76 M pivots/s at
    // 128 LPs and 2.13 M at 1024 LPs; lockstep launch pairs 1.62 M and 1.25 M
    // default: blocked, with the sweep of a block as ONE launch over all LPs (every CU busy in the
    // part that moves the tableaux; the look-ahead of a block is one workgroup per LP): 128 LPs of
    // 512 x 256 3.5 -> 7.2 M pivots/s, 1024 LPs 8.2 -> 11.4 M against the all-in-one-workgroup
    // kernel.  Needs the compact representation and an LP whose block state fits the LDS.
    if ((t->tn.batch_mode == 0 || t->tn.batch_mode == 3) && t->compact) {
        bool split_ok = true;
        int64_t blocks = 2;
        for (;;) {
            for (int64_t i = 0; i < blocks && split_ok; ++i) {
                split_ok = launch_batch_block_split(t->c, is_max, f, t->stream);
                if (split_ok) t->batch_counts[0]++;
            }
            if (!split_ok) break;
            HIP_TRY(hipGetLastError());
            { const int rc_ = read_ctls(t, n); if (rc_ != MI_OK) return rc_; }
            bool running = false, need_dense = false;
            for (int64_t i = 0; i < n; ++i) {
                running |= t->h_ctl[i].status == kRunning;
                need_dense |= t->h_ctl[i].status == kNeedDense;
            }
            if (need_dense) { split_ok = false; break; }      // finish below on the dense tableaux
            if (!running) {
                t->n_part = 0;
                for (int64_t i = 0; i < n; ++i) {
                    if (status) status[i] = t->h_ctl[i].status;
                    if (n_pivots) n_pivots[i] = t->h_ctl[i].n_pivots;
                }
                return MI_OK;
            }
            if (take_cancel(t)) { t->n_part = 0; return batch_report(t, status, n_pivots, MI_CANCELLED); }
            if (blocks < 8) blocks *= 2;
        }
        if (t->compact) {                                      // an LP met an inf / NaN: the established path
            bool need_dense = false;
            for (int64_t i = 0; i < n; ++i) need_dense |= t->h_ctl[i].status == kNeedDense;
            if (need_dense) {
                rc = fall_back_to_dense(t);
                if (rc != MI_OK) return rc;
            }
        }
    }
    const bool want_persistent = t->tn.batch_mode != 1;
    bool persistent = want_persistent && launch_batch_solve(cur(t), is_max, f, t->stream);
    if (persistent) { t->n_part = 0; t->batch_counts[1]++; }
    if (!persistent) enqueue_select(t, is_max, f);
    int64_t chunk = 16;
    for (;;) {
        if (persistent) {
            HIP_TRY(hipGetLastError());
            { const int rc_ = read_ctls(t, n); if (rc_ != MI_OK) return rc_; }
            bool need_dense = false, running = false;
            for (int64_t i = 0; i < n; ++i) {
                need_dense |= t->h_ctl[i].status == kNeedDense;
                running |= t->h_ctl[i].status == kRunning;
            }
            if (need_dense) {
                rc = fall_back_to_dense(t);           // some LP met an inf / NaN: finish densely
                if (rc != MI_OK) return rc;
            } else if (!running) {
                break;
            } else if (take_cancel(t)) {              // (a launch ends after kBatchLaunchCap pivots per LP at the latest)
                return batch_report(t, status, n_pivots, MI_CANCELLED);
            }
            if (!launch_batch_solve(cur(t), is_max, f, t->stream)) return fail(MI_HIP_ERROR, "batch relaunch failed");
            t->batch_counts[1]++;
            continue;
        }
        for (int64_t i = 0; i < chunk; ++i) {
            rc = enqueue_update(t, is_max);
            if (rc != MI_OK) return rc;
            enqueue_select(t, is_max, f);
        }
        t->batch_counts[2] += chunk;
        HIP_TRY(hipGetLastError());
        { const int rc_ = read_ctls(t, n); if (rc_ != MI_OK) return rc_; }
        bool running = false, need_dense = false;
        for (int64_t i = 0; i < n; ++i) {
            running |= t->h_ctl[i].status == kRunning;
            need_dense |= t->h_ctl[i].status == kNeedDense;
        }
        if (need_dense) {
            // The chunk ended on a select: every LP that is still running has a pivot selected and
            // HALF done (on the compact representation the select already moved the leaving column
            // into the entering column's slot).  Finish those pivots before the representation
            // changes -- the update is a no-op for the LP(s) that asked for the dense tableau.
            rc = enqueue_update(t, is_max);
            if (rc != MI_OK) return rc;
            rc = fall_back_to_dense(t);
            if (rc != MI_OK) return rc;
            enqueue_select(t, is_max, f);
            continue;
        }
        if (!running) break;
        if (take_cancel(t)) {
            // the chunk ended on a select: finish the pivots it chose (see above), then report
            rc = enqueue_update(t, is_max);
            if (rc != MI_OK) return rc;
            HIP_TRY(hipGetLastError());
            { const int rc_ = read_ctls(t, n); if (rc_ != MI_OK) return rc_; }
            return batch_report(t, status, n_pivots, MI_CANCELLED);
        }
        if (chunk < 256) chunk *= 2;
    }
    return batch_report(t, status, n_pivots, MI_OK);
}

int mi355x_batch_cancel(mi355x_batch *b)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    b->t->cancel.store(1, std::memory_order_release);
    return MI_OK;
}

int mi355x_multibatch_cancel(mi355x_multibatch *mb)
{
    if (!mb) return fail(MI_BAD_ARG, "handle is NULL");
    for (mi355x_batch *b : mb->sub) b->t->cancel.store(1, std::memory_order_release);
    return MI_OK;
}

int mi355x_batch_download(mi355x_batch *b, int64_t k, double *hm, int64_t *hb, double *last_row,
                          double *last_col)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    mi355x_tab *t = b->t;
    const TabView &v = t->v;
    if (k < 0 || k >= v.n_lps) return fail(MI_BAD_ARG, "lp_index %lld out of range", (long long)k);
    int rc = use_device(t);
    if (rc != MI_OK) return rc;
    rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    rc = download_parts(v.M + k * v.rows * v.ld, v.ld, v.rows, v.cols, v.basis + k * std::max<int64_t>(v.rows - 1, 1),
                        t->stream, hm, hb, last_row, last_col);
    if (rc != MI_OK) return rc;
    HIP_TRY(wait_stream(t->stream));
    return MI_OK;
}

int mi355x_batch_timing_enable(mi355x_batch *b, int enable)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    return mi355x_tab_timing_enable(b->t, enable);
}

int mi355x_batch_timing_read(mi355x_batch *b, int64_t *n_launches, double *sum_ms, double *min_ms)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    return mi355x_tab_timing_read(b->t, n_launches, sum_ms, min_ms);
}

void mi355x_batch_destroy(mi355x_batch *b)
{
    if (!b) return;
    if (b->worker.joinable()) b->worker.join();
    free_tab(b->t);
    delete b;
}

// ---- asynchronous batch solve: the loop of mi355x_batch_solve on a worker thread ---------------
// The batch solve is host-driven (blind chunks of launches, one status read-back per chunk), so
// "asynchronous" means: the library drives it from a thread of its own while the caller's thread
// goes on -- e.g. starts the sub-batches of the other GPUs.  One solve at a time per batch.
int mi355x_batch_solve_async(mi355x_batch *b, int is_max, double f, int64_t max_pivots)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    if (b->running) return fail(MI_BAD_ARG, "a solve of this batch is already running (mi355x_batch_sync first)");
    if (b->worker.joinable()) b->worker.join();
    const int64_t n = b->t->v.n_lps;
    b->w_status.assign((size_t)n, 0);
    b->w_pivots.assign((size_t)n, 0);
    b->worker_rc = MI_OK;
    b->worker_err.clear();
    b->running = true;
    try {
        b->worker = std::thread([b, is_max, f, max_pivots]() {
            b->worker_rc = mi355x_batch_solve(b, is_max, f, max_pivots, b->w_status.data(), b->w_pivots.data());
            if (b->worker_rc != MI_OK) b->worker_err = g_err;        // g_err is thread-local
        });
    } catch (...) {
        b->running = false;
        return fail(MI_NO_MEMORY, "could not start the worker thread");
    }
    return MI_OK;
}

int mi355x_batch_sync(mi355x_batch *b, int32_t *status, int64_t *n_pivots)
{
    if (!b || !b->t) return fail(MI_BAD_ARG, "batch is NULL");
    if (!b->running) return fail(MI_BAD_ARG, "no asynchronous solve of this batch is in flight");
    if (b->worker.joinable()) b->worker.join();
    b->running = false;
    if (b->worker_rc < 0) { g_err = b->worker_err; return b->worker_rc; }
    const int64_t n = b->t->v.n_lps;
    if (status) std::copy(b->w_status.begin(), b->w_status.begin() + n, status);
    if (n_pivots) std::copy(b->w_pivots.begin(), b->w_pivots.begin() + n, n_pivots);
    return b->worker_rc;                              // MI_OK, or MI_CANCELLED (mi355x_batch_cancel)
}

// ---- one batch over several devices (BASELINE config 4: 1024 LPs over 8 GPUs) -------------------
// LP k lives in sub-batch k / ceil(n_lps / n_devices) (contiguous blocks); independent units, no
// communication.  One call solves all of them: every sub-batch's loop runs on its own worker
// thread (mi355x_batch_solve_async), the caller's thread only waits -- so a single-threaded host
// keeps all GPUs busy.  Fewer visible devices than sub-batches (device_ids == NULL): the
// sub-batches become logical sub-batches on device 0, each with its own stream.
static void mb_free(mi355x_multibatch *mb)
{
    if (!mb) return;
    for (mi355x_batch *b : mb->sub) mi355x_batch_destroy(b);
    delete mb;
}

static int mb_layout(mi355x_multibatch *mb, int64_t n_lps, int64_t rows, int64_t cols, int *n_devices,
                     const int *device_ids, std::vector<int> &devs)
{
    if (n_lps < 1 || *n_devices < 1) return fail(MI_BAD_ARG, "need n_lps >= 1 and n_devices >= 1");
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if ((int64_t)*n_devices > n_lps) *n_devices = (int)n_lps;
    devs.resize((size_t)*n_devices);
    for (int d = 0; d < *n_devices; ++d) {
        if (device_ids) {
            if (device_ids[d] < 0 || device_ids[d] >= ndev) return fail(MI_BAD_ARG, "device %d out of range [0,%d)", device_ids[d], ndev);
            devs[(size_t)d] = device_ids[d];
        } else {
            devs[(size_t)d] = ndev >= *n_devices ? d : 0;
        }
    }
    mb->n_lps = n_lps; mb->rows = rows; mb->cols = cols;
    const int64_t per = (n_lps + *n_devices - 1) / *n_devices;
    mb->first.clear();
    for (int d = 0; d < *n_devices; ++d) mb->first.push_back(std::min<int64_t>((int64_t)d * per, n_lps));
    mb->first.push_back(n_lps);
    return MI_OK;
}

int mi355x_multibatch_create(mi355x_multibatch **out, int64_t n_lps, int64_t rows, int64_t cols,
                             const double *host_matrices, const int64_t *host_bases, int n_devices,
                             const int *device_ids)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (!host_matrices) return fail(MI_BAD_ARG, "host_matrices is NULL");
    mi355x_multibatch *mb = new (std::nothrow) mi355x_multibatch;
    if (!mb) return fail(MI_NO_MEMORY, "host allocation failed");
    std::vector<int> devs;
    int rc = mb_layout(mb, n_lps, rows, cols, &n_devices, device_ids, devs);
    for (int d = 0; rc == MI_OK && d < n_devices; ++d) {
        const int64_t k0 = mb->first[(size_t)d], k1 = mb->first[(size_t)d + 1];
        if (k1 <= k0) continue;
        mi355x_batch *b = nullptr;
        rc = mi355x_batch_create(&b, k1 - k0, rows, cols, host_matrices + k0 * rows * cols,
                                 host_bases ? host_bases + k0 * std::max<int64_t>(rows - 1, 0) : nullptr, devs[(size_t)d]);
        if (rc == MI_OK) mb->sub.push_back(b);
    }
    if (rc != MI_OK) { mb_free(mb); return rc; }
    // (sub-batches that would be empty were skipped: first[] keeps only the boundaries in use)
    std::vector<int64_t> f2;
    for (size_t d = 0; d + 1 < mb->first.size(); ++d)
        if (mb->first[d + 1] > mb->first[d]) f2.push_back(mb->first[d]);
    f2.push_back(n_lps);
    mb->first = f2;
    *out = mb;
    return MI_OK;
}

int mi355x_multibatch_create_synthetic(mi355x_multibatch **out, int64_t n_lps, int64_t n_vars, int64_t n_cons,
                                       const uint64_t *seeds, int n_devices, const int *device_ids)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (!seeds) return fail(MI_BAD_ARG, "seeds is NULL");
    mi355x_multibatch *mb = new (std::nothrow) mi355x_multibatch;
    if (!mb) return fail(MI_NO_MEMORY, "host allocation failed");
    std::vector<int> devs;
    int rc = mb_layout(mb, n_lps, n_cons + 1, n_vars + n_cons + 1, &n_devices, device_ids, devs);
    std::vector<int64_t> f2;
    for (int d = 0; rc == MI_OK && d < n_devices; ++d) {
        const int64_t k0 = mb->first[(size_t)d], k1 = mb->first[(size_t)d + 1];
        if (k1 <= k0) continue;
        mi355x_batch *b = nullptr;
        rc = mi355x_batch_create_synthetic(&b, k1 - k0, n_vars, n_cons, seeds + k0, devs[(size_t)d]);
        if (rc == MI_OK) { mb->sub.push_back(b); f2.push_back(k0); }
    }
    if (rc != MI_OK) { mb_free(mb); return rc; }
    f2.push_back(n_lps);
    mb->first = f2;
    *out = mb;
    return MI_OK;
}

int mi355x_multibatch_info(const mi355x_multibatch *mb, int *n_sub_batches, int *n_devices_used)
{
    if (!mb) return fail(MI_BAD_ARG, "handle is NULL");
    if (n_sub_batches) *n_sub_batches = (int)mb->sub.size();
    if (n_devices_used) {
        std::vector<int> seen;
        for (mi355x_batch *b : mb->sub)
            if (std::find(seen.begin(), seen.end(), b->t->device) == seen.end()) seen.push_back(b->t->device);
        *n_devices_used = (int)seen.size();
    }
    return MI_OK;
}

int mi355x_multibatch_solve(mi355x_multibatch *mb, int is_max, double f, int64_t max_pivots, int32_t *status,
                            int64_t *n_pivots)
{
    if (!mb) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = MI_OK;
    size_t started = 0;
    for (; started < mb->sub.size(); ++started) {
        rc = mi355x_batch_prepare(mb->sub[started]);                 // representation change: before the worker starts
        if (rc == MI_OK) rc = mi355x_batch_solve_async(mb->sub[started], is_max, f, max_pivots);
        if (rc != MI_OK) break;
    }
    std::string err = rc != MI_OK ? g_err : std::string();
    for (size_t d = 0; d < started; ++d) {                           // wait for every worker that did start
        const int64_t k0 = mb->first[d];
        const int r2 = mi355x_batch_sync(mb->sub[d], status ? status + k0 : nullptr, n_pivots ? n_pivots + k0 : nullptr);
        if (r2 != MI_OK && rc == MI_OK) { rc = r2; err = g_err; }
    }
    if (rc != MI_OK) g_err = err;
    return rc;
}

int mi355x_multibatch_download(mi355x_multibatch *mb, int64_t k, double *hm, int64_t *hb, double *last_row,
                               double *last_col)
{
    if (!mb) return fail(MI_BAD_ARG, "handle is NULL");
    if (k < 0 || k >= mb->n_lps) return fail(MI_BAD_ARG, "lp_index %lld out of range", (long long)k);
    size_t d = 0;
    while (d + 1 < mb->sub.size() && k >= mb->first[d + 1]) ++d;
    return mi355x_batch_download(mb->sub[d], k - mb->first[d], hm, hb, last_row, last_col);
}

void mi355x_multibatch_destroy(mi355x_multibatch *mb) { mb_free(mb); }

// ---- n-solve-tableau, two-phase branch (src/simplex.lisp:402-452), for a batch -------------------
// Member k of `art` is the artificial tableau of the problem whose main tableau is member k of
// `main_mb` (build-tableau's two results, :326-328): phase 1 = the batch loop on `art` (min
// problems); per member the feasibility test (fp= 0 objective) :405-407, the drive-out pivots of
// degenerate artificials still basic (:419-434 -- row fetches and single pivots on that member's
// slice of the batch) and the hand-over :437-451 (mi355x_solve_two_phase's kernels on that member's
// slices of the two batches); phase 2 = the batch loop on `main_mb`.  A member that ends between the
// phases (MI_INFEASIBLE, MI_ART_NONZERO, MI_ART_STUCK) keeps that status; the others are not held up.
static TabView mb_member_view(const TabView &v, int64_t k)
{
    TabView s = v;
    s.M += k * v.zs_M; s.basis += k * v.zs_basis; s.col += k * v.zs_col; s.prow += k * v.zs_prow;
    s.ctl += k;
    s.n_lps = 1;
    return s;
}

static int mb_two_phase_check(mi355x_multibatch *art, mi355x_multibatch *main_mb)
{
    if (art->n_lps != main_mb->n_lps || art->rows != main_mb->rows || art->cols < main_mb->cols ||
        art->sub.size() != main_mb->sub.size() || art->first != main_mb->first)
        return fail(MI_BAD_ARG, "the artificial and the main batch do not match (members, rows, sub-batches)");
    for (size_t d = 0; d < art->sub.size(); ++d)
        if (art->sub[d]->t->device != main_mb->sub[d]->t->device)
            return fail(MI_BAD_ARG, "sub-batch %zu of the two batches lives on different devices", d);
    return MI_OK;
}

// Between the phases, member by member (simplex.lisp:405-451): feasibility test, drive-out pivots of
// artificial variables still basic (row fetches and single pivots on that member's tableau inside the
// batch -- the steps of two_phase_handover_impl on a member view), rows + basis across, objective row
// re-eliminated.  phase1_status (NULL = every member ended phase 1 MI_OPTIMAL): members with another
// status keep it.  status[k] = MI_OK: member k of main_mb is ready for phase 2; anything else is that
// member's final outcome, and its main tableau is neutralised (an all-zero objective row prices as
// optimal at once: the batch loop of phase 2 must not run on what is no consistent tableau).
int mi355x_multibatch_two_phase_handover(mi355x_multibatch *art, mi355x_multibatch *main_mb, double f,
                                         const int32_t *phase1_status, int32_t *status, int64_t *n_driveout)
{
    if (!art || !main_mb || !status) return fail(MI_BAD_ARG, "NULL argument");
    int rc = mb_two_phase_check(art, main_mb);
    if (rc != MI_OK) return rc;
    const int64_t rows = art->rows, m = rows - 1, num_vars = main_mb->cols - 1, num_art_vars = art->cols - 1;
    std::vector<double> obj;
    std::vector<int64_t> basis;
    for (size_t d = 0; d < art->sub.size(); ++d) {
        mi355x_tab *at = art->sub[d]->t, *mt = main_mb->sub[d]->t;
        const int64_t k0 = art->first[d], nd = art->first[d + 1] - k0;
        if ((rc = use_device(at)) != MI_OK || (rc = ensure_dense(at)) != MI_OK || (rc = ensure_dense(mt)) != MI_OK) return rc;
        HIP_TRY(hipStreamSynchronize(mt->stream));
        obj.resize((size_t)nd);
        basis.resize((size_t)(nd * std::max<int64_t>(m, 1)));
        // objective value (last row, last column) and basis of every member of this sub-batch
        HIP_TRY(hipMemcpy2DAsync(obj.data(), sizeof(double), at->v.M + m * at->v.ld + num_art_vars,
                                 (size_t)rows * at->v.ld * sizeof(double), sizeof(double), (size_t)nd,
                                 hipMemcpyDeviceToHost, at->stream));
        if (m > 0)
            HIP_TRY(hipMemcpyAsync(basis.data(), at->v.basis, (size_t)(nd * m) * sizeof(int64_t), hipMemcpyDeviceToHost, at->stream));
        HIP_TRY(hipStreamSynchronize(at->stream));
        for (int64_t q = 0; q < nd; ++q) {
            const int64_t k = k0 + q;
            int32_t out = phase1_status ? phase1_status[k] : MI_OPTIMAL;
            bool drove_out = false;
            if (n_driveout) n_driveout[k] = 0;
            if (out == MI_OPTIMAL) {
                if (!tp_feasible(obj[(size_t)q], f * kClEpsilon)) out = MI_INFEASIBLE;            // (fp= 0 objective factor) :405-407
            }
            if (out == MI_OPTIMAL) {
                // degenerate artificials still basic: pivot them out                             :419-434
                const TabView av = mb_member_view(at->v, q);
                out = tp_drive_out<double>(
                    m, num_vars, num_art_vars, basis.data() + q * m, [](double x) { return x == 0.0; },
                    [&](int64_t i, std::vector<double> &row) { return fetch_row(av.M + i * av.ld, av.cols, at->stream, row); },
                    [&](int64_t col, int64_t i) {
                        launch_prepare_pivot(av, col, i, at->stream);                            // = mi355x_tab_pivot on the member
                        launch_update(av, 1.0, 0, at->stream);
                        HIP_TRY(hipGetLastError());
                        return (int)MI_OK;
                    },
                    [&] { drove_out = true; if (n_driveout) n_driveout[k]++; });
                if (out < 0) return out;                                                         // (an error, not the member's outcome)
            }
            if (out == MI_OPTIMAL) {
                status[k] = MI_OK;
                launch_handover(mb_member_view(at->v, q), mb_member_view(mt->v, q),
                                !drove_out && at->unit_basis && at->tn.handover_mode != 1, at->stream);   // :437-451
            } else {
                status[k] = out;
                HIP_TRY(hipMemsetAsync(mt->v.M + q * mt->v.zs_M + m * mt->v.ld, 0, (size_t)mt->v.ld * sizeof(double), at->stream));
            }
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(at->stream));
        at->n_part = 0;
        mt->n_part = 0;
        mt->unit_basis = false;
        mt->compact_failed = false;
    }
    return MI_OK;
}

int mi355x_multibatch_solve_two_phase(mi355x_multibatch *art, mi355x_multibatch *main_mb, int main_is_max, double f,
                                      int32_t *status, int64_t *n_pivots)
{
    if (!art || !main_mb || !status) return fail(MI_BAD_ARG, "NULL argument");
    int rc = mb_two_phase_check(art, main_mb);
    if (rc != MI_OK) return rc;
    const int64_t n = art->n_lps;
    std::vector<int32_t> st1((size_t)n, 0), st2((size_t)n, 0);
    std::vector<int64_t> np1((size_t)n, 0), np2((size_t)n, 0), nd((size_t)n, 0);
    rc = mi355x_multibatch_solve(art, /*is_max=*/0, f, 0, st1.data(), np1.data());              // :403
    if (rc != MI_OK) return rc;
    rc = mi355x_multibatch_two_phase_handover(art, main_mb, f, st1.data(), status, nd.data());    // :405-451
    if (rc != MI_OK) return rc;
    rc = mi355x_multibatch_solve(main_mb, main_is_max, f, 0, st2.data(), np2.data());            // :452
    if (rc != MI_OK) return rc;
    for (int64_t k = 0; k < n; ++k) {
        const bool went = status[k] == MI_OK;
        if (went) status[k] = st2[(size_t)k];
        if (n_pivots) { n_pivots[2 * k] = np1[(size_t)k] + nd[(size_t)k]; n_pivots[2 * k + 1] = went ? np2[(size_t)k] : 0; }
    }
    return MI_OK;
}

}  // extern "C"
