// capi_tab_impl.inc -- one tableau behind a handle: allocation, representation changes, the blind enqueue of select / update / look-ahead blocks / the resident launch (internal helpers).
// Part of simplex_capi.hip (ONE translation unit: included there, in this order).

namespace {

// launch classes counted per handle (mi355x_tab_path_counts): what the dispatcher really enqueued
// the two record buffers of a handle: kMaxLaRecords transposed records for k_la_block (single tableaux), one
// 64-byte line per workgroup for k_shard_la_block (column shards): room for the larger of the two
constexpr size_t kLaRecordBytes = (kMaxShardLaWorkgroups > kMaxLaRecords ? kMaxShardLaWorkgroups : kMaxLaRecords) * sizeof(ExchRec);

enum PathCount { kPathPerPivot = 0, kPathLaPersistent, kPathLaTwoLaunch, kPathSweep16, kPathSweepWide,
                 kPathSweepShort, kPathResident, kPathSelectSplit };

int use_device(const mi355x_tab *t)
{
    HIP_TRY(hipSetDevice(t->device));
    return MI_OK;
}

// `cols` entries from `src` on (one tableau row) into `row`, synchronised: what tp_drive_out fetches per drive-out
template <class T> int fetch_row(const T *src, int64_t cols, hipStream_t s, std::vector<T> &row)
{
    row.resize((size_t)cols);
    HIP_TRY(hipMemcpyAsync(row.data(), src, cols * sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MI_OK;
}

// What every tableau download hands out, each part only where its pointer is not NULL: the matrix tightly packed,
// the basis, the objective row, the RHS column.  M and basis are the tableau's own (a batch member's: already
// offset), T its number type.  Only enqueues on `s`: the wait is the caller's.
template <class T>
int download_parts(const T *M, int64_t ld, int64_t rows, int64_t cols, const int64_t *basis, hipStream_t s, T *hm,
                   int64_t *hb, T *last_row, T *last_col)
{
    if (hm)
        HIP_TRY(hipMemcpy2DAsync(hm, cols * sizeof(T), M, ld * sizeof(T), cols * sizeof(T), rows, hipMemcpyDeviceToHost, s));
    if (hb && rows > 1) HIP_TRY(hipMemcpyAsync(hb, basis, (rows - 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (last_row) HIP_TRY(hipMemcpyAsync(last_row, M + (rows - 1) * ld, cols * sizeof(T), hipMemcpyDeviceToHost, s));
    if (last_col)
        HIP_TRY(hipMemcpy2DAsync(last_col, sizeof(T), M + (cols - 1), ld * sizeof(T), sizeof(T), rows, hipMemcpyDeviceToHost, s));
    return MI_OK;
}

// the first min(total, cap, trace_cap) pivots of a trace (total: how many there were); waits only for what it enqueued
// (on the handle's stream: a synchronous hipMemcpy on the null stream out of these 8 MB buffers left 8 MB of device
// memory unaccounted for per handle once the handle was destroyed -- found by a 37 000-handle fuzz run that ended in
// hipErrorOutOfMemory)
int download_trace(const int64_t *trace_ec, const int64_t *trace_cr, int64_t total, int64_t trace_cap, hipStream_t s,
                   int64_t *ecs, int64_t *crs, int64_t cap, int64_t *n)
{
    if (n) *n = total;
    const int64_t k = std::min<int64_t>(std::min<int64_t>(total, cap), trace_cap);
    if (k > 0 && ecs) HIP_TRY(hipMemcpyAsync(ecs, trace_ec, k * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (k > 0 && crs) HIP_TRY(hipMemcpyAsync(crs, trace_cr, k * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (k > 0 && (ecs || crs)) HIP_TRY(hipStreamSynchronize(s));
    return MI_OK;
}

void free_tab(mi355x_tab *t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->own_stream) (void)hipStreamSynchronize(t->own_stream);
    for (auto e : t->ev0) (void)hipEventDestroy(e);
    for (auto e : t->ev1) (void)hipEventDestroy(e);
    for (auto e : t->la0) (void)hipEventDestroy(e);
    for (auto e : t->la1) (void)hipEventDestroy(e);
    (void)hipFree(t->v.M);
    (void)hipFree(t->v.basis);
    (void)hipFree(t->v.col);
    (void)hipFree(t->v.prow);
    (void)hipFree(t->v.rhs);
    (void)hipFree(t->v.ctl);
    (void)hipFree(t->v.trace_ec);
    (void)hipFree(t->v.trace_cr);
    (void)hipFree(t->v.part_v);
    (void)hipFree(t->v.part_i);
    (void)hipFree(t->v.part_s);
    (void)hipFree(t->v.bk_col);
    (void)hipFree(t->v.bk_prow);
    (void)hipFree(t->v.blk);
    (void)hipFree(t->v.bk_rmask);
    (void)hipFree(t->v.bk_smask);
    (void)hipFree(t->v.bk_smask2);
    (void)hipFree(t->v.la_px);
    (void)hipFree(t->v.la_rx);
    (void)hipFree(t->c.M);
    (void)hipFree(t->c.p2l);
    (void)hipFree(t->c.l2p);
    (void)hipFree(t->v.p2l);
    (void)hipFree(t->v.l2p);
    (void)hipFree(t->brow);
    (void)hipFree(t->flag);
    (void)hipFree(t->res_x);
    if (t->h_ctl) (void)hipHostFree(t->h_ctl);
    if (t->h_seq) (void)hipHostFree(t->h_seq);
    if (t->own_stream) (void)hipStreamDestroy(t->own_stream);
    delete t;
}

// allocate an empty handle of the given shape on `device`
int alloc_tab(mi355x_tab **out, int64_t rows, int64_t cols, int device, int64_t n_lps = 1,
              bool defer_dense = false)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (rows < 1 || cols < 1) return fail(MI_BAD_ARG, "rows=%lld cols=%lld must be >= 1",
                                          (long long)rows, (long long)cols);
    if (rows > 65535LL * 16) return fail(MI_BAD_ARG, "rows=%lld exceeds the supported 1048560",
                                         (long long)rows);
    if (n_lps < 1 || n_lps > 65535) return fail(MI_BAD_ARG, "n_lps=%lld outside [1,65535]", (long long)n_lps);
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(MI_BAD_ARG, "device %d out of range [0,%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    mi355x_tab *t = new (std::nothrow) mi355x_tab;
    if (!t) return fail(MI_NO_MEMORY, "host allocation failed");
    t->device = device;
    t->v.rows = rows;
    t->v.cols = cols;
    t->v.ld = padded_ld(cols);
    t->v.n_lps = n_lps;
    const int part_cap = n_lps == 1 ? kPartCap : kBatchPartCap;
    const int64_t nb = std::max<int64_t>(rows - 1, 1);
    if (n_lps > 1) {
        t->v.zs_M = rows * t->v.ld;
        t->v.zs_basis = nb;
        t->v.zs_col = rows;
        t->v.zs_prow = t->v.ld;
        t->v.zs_part = part_cap;
    }
    t->v.trace_cap = n_lps == 1 ? kTraceCap : 0;
    const size_t mbytes = (size_t)n_lps * (size_t)rows * (size_t)t->v.ld * sizeof(double);
    hipError_t e;
#define ALLOC(ptr, bytes)                                                                  \
    if ((e = hipMalloc((void **)&(ptr), (bytes))) != hipSuccess) {                         \
        free_tab(t);                                                                       \
        return fail(e == hipErrorOutOfMemory ? MI_NO_MEMORY : MI_HIP_ERROR,                \
                    "hipMalloc(%zu bytes) failed: %s", (size_t)(bytes), hipGetErrorString(e)); \
    }
    if (!defer_dense) ALLOC(t->v.M, mbytes);         // else: allocated by ensure_dense on demand
    ALLOC(t->v.basis, n_lps * nb * sizeof(int64_t));
    ALLOC(t->v.col, n_lps * rows * sizeof(double));
    ALLOC(t->v.prow, n_lps * t->v.ld * sizeof(double));
    if (n_lps == 1) ALLOC(t->v.rhs, rows * sizeof(double));
    ALLOC(t->v.ctl, n_lps * sizeof(Ctl));
    if (n_lps == 1) {
        ALLOC(t->v.trace_ec, kTraceCap * sizeof(int64_t));
        ALLOC(t->v.trace_cr, kTraceCap * sizeof(int64_t));
    }
    ALLOC(t->v.part_v, n_lps * part_cap * sizeof(double));
    ALLOC(t->v.part_i, n_lps * part_cap * sizeof(int64_t));
    ALLOC(t->v.part_s, n_lps * part_cap * sizeof(int64_t));
    t->v.part_cap = part_cap;
    if (n_lps > 1) {                                  // per-LP block state (look-ahead launch -> sweep launch)
        t->v.bk_stride = (rows + kLdAlign - 1) / kLdAlign * kLdAlign;
        t->v.zs_bk = (int64_t)kMaxBlock * t->v.bk_stride;
        t->v.zs_bkp = (int64_t)kMaxBlock * t->v.ld;
        t->v.zs_rm = t->v.bk_stride;
        t->v.zs_sm = t->v.ld;
        ALLOC(t->v.bk_col, (size_t)n_lps * t->v.zs_bk * sizeof(double));
        ALLOC(t->v.bk_prow, (size_t)n_lps * t->v.zs_bkp * sizeof(double));
        ALLOC(t->v.bk_rmask, (size_t)n_lps * t->v.zs_rm * sizeof(uint32_t));
        ALLOC(t->v.bk_smask, (size_t)n_lps * t->v.zs_sm * sizeof(uint32_t));
        ALLOC(t->v.blk, (size_t)n_lps * sizeof(BlockCtl));
    }
    if (n_lps == 1) {                                 // blocked pivoting (DESIGN.md 4.8)
        t->v.bk_stride = (rows + kLdAlign - 1) / kLdAlign * kLdAlign;
        ALLOC(t->v.bk_col, (size_t)kWideBlock * t->v.bk_stride * sizeof(double));     // (room for wide blocks)
        ALLOC(t->v.bk_prow, (size_t)kWideBlock * t->v.ld * sizeof(double));
        ALLOC(t->v.blk, sizeof(BlockCtl));
        ALLOC(t->v.bk_rmask, (size_t)t->v.bk_stride * sizeof(uint32_t));
        ALLOC(t->v.bk_smask, (size_t)t->v.ld * sizeof(uint32_t));
        ALLOC(t->v.bk_smask2, (size_t)t->v.ld * sizeof(uint32_t));
        ALLOC(t->v.la_px, kLaRecordBytes);
        ALLOC(t->v.la_rx, kLaRecordBytes);
    }
#undef ALLOC
    // (coherent: the GPU writes both while the host polls h_seq -- k_ctl_publish)
    if ((e = hipHostMalloc((void **)&t->h_ctl, n_lps * sizeof(Ctl), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
        (e = hipHostMalloc((void **)&t->h_seq, 64, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&t->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        free_tab(t);
        return fail(MI_HIP_ERROR, "stream/pinned allocation failed: %s", hipGetErrorString(e));
    }
    t->stream = t->own_stream;
    memset(t->h_ctl, 0, n_lps * sizeof(Ctl));
    memset(t->h_seq, 0, 64);
    poison(t->v.M, t->v.M ? mbytes : 0, t->stream);
    poison(t->v.col, n_lps * rows * sizeof(double), t->stream);
    poison(t->v.prow, n_lps * t->v.ld * sizeof(double), t->stream);
    poison(t->v.rhs, rows * sizeof(double), t->stream);
    poison(t->v.trace_ec, kTraceCap * sizeof(int64_t), t->stream);
    poison(t->v.trace_cr, kTraceCap * sizeof(int64_t), t->stream);
    // pricing / ratio partials are read by launches that may follow a no-op launch: defined contents
    if ((e = hipMemsetAsync(t->v.part_v, 0, n_lps * part_cap * sizeof(double), t->stream)) != hipSuccess ||
        (e = hipMemsetAsync(t->v.part_i, 0xff, n_lps * part_cap * sizeof(int64_t), t->stream)) != hipSuccess ||
        (e = hipMemsetAsync(t->v.part_s, 0, n_lps * part_cap * sizeof(int64_t), t->stream)) != hipSuccess) {
        free_tab(t);
        return fail(MI_HIP_ERROR, "memset failed: %s", hipGetErrorString(e));
    }
    if (n_lps > 1 && ((e = hipMemsetAsync(t->v.bk_col, 0, (size_t)n_lps * t->v.zs_bk * sizeof(double), t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.bk_prow, 0, (size_t)n_lps * t->v.zs_bkp * sizeof(double), t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.bk_rmask, 0, (size_t)n_lps * t->v.zs_rm * sizeof(uint32_t), t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.bk_smask, 0, (size_t)n_lps * t->v.zs_sm * sizeof(uint32_t), t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.blk, 0, (size_t)n_lps * sizeof(BlockCtl), t->stream)) != hipSuccess)) {
        free_tab(t);
        return fail(MI_HIP_ERROR, "memset failed: %s", hipGetErrorString(e));
    }
    if ((n_lps == 1 && ((e = hipMemsetAsync(t->v.blk, 0, sizeof(BlockCtl), t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.bk_rmask, 0, t->v.bk_stride * sizeof(uint32_t), t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.bk_smask, 0, t->v.ld * sizeof(uint32_t), t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.bk_smask2, 0, t->v.ld * sizeof(uint32_t), t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.la_px, 0, kLaRecordBytes, t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.la_rx, 0, kLaRecordBytes, t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.bk_col, 0, (size_t)kWideBlock * t->v.bk_stride * sizeof(double), t->stream)) != hipSuccess ||
                      (e = hipMemsetAsync(t->v.bk_prow, 0, (size_t)kWideBlock * t->v.ld * sizeof(double), t->stream)) != hipSuccess)) ||
        (e = hipMemsetAsync(t->v.ctl, 0, n_lps * sizeof(Ctl), t->stream)) != hipSuccess ||
        (e = hipMemsetAsync(t->v.basis, 0, n_lps * nb * sizeof(int64_t), t->stream)) != hipSuccess) {
        free_tab(t);
        return fail(MI_HIP_ERROR, "memset failed: %s", hipGetErrorString(e));
    }
    *out = t;
    return MI_OK;
}

int upload(mi355x_tab *t, const double *hm, const int64_t *hb)
{
    const TabView &v = t->v;
    t->n_part = 0;
    t->compact = false;                   // the dense logical tableau is (re)defined by the caller
    t->compact_failed = false;
    t->unit_basis = false;
    if (!t->v.M)
        HIP_TRY(hipMalloc((void **)&t->v.M, (size_t)v.n_lps * v.rows * v.ld * sizeof(double)));
    if (hm) {
        const size_t all_rows = (size_t)v.rows * v.n_lps;     // LPs of a batch are stacked
        if (v.ld != v.cols)    // zero the padding columns once per upload
            HIP_TRY(hipMemsetAsync(v.M, 0, all_rows * v.ld * sizeof(double), t->stream));
        HIP_TRY(hipMemcpy2DAsync(v.M, v.ld * sizeof(double), hm, v.cols * sizeof(double),
                                 v.cols * sizeof(double), all_rows, hipMemcpyHostToDevice, t->stream));
    }
    if (hb && v.rows > 1)
        HIP_TRY(hipMemcpyAsync(v.basis, hb, v.n_lps * (v.rows - 1) * sizeof(int64_t),
                               hipMemcpyHostToDevice, t->stream));
    launch_ctl_reset(v, 0, /*reset_trace=*/1, t->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));   // host buffers may be released by the caller
    return MI_OK;
}

// Wait for everything enqueued on `s`.  hipStreamSynchronize lets the thread sleep on the completion
// interrupt; coming back costs 20 .. 50 us on an idle host -- a tenth of a 20-pivot request at config 3
// (one block: 0.3 ms) -- and milliseconds when the host is busy or the runtime takes that path for the
// first time (5 .. 20 ms measured: the whole difference between the 61 k and the 88 k pivots/s of one
// and the same steady-state run, bench.py).  The waits of the solve loops are short (the status
// read-back behind a chunk of blocks: 0.3 .. 20 ms; a whole config-3 solve is 70 ms) and the calling
// thread has nothing else to do, so the stream is POLLED -- what the CUDA runtime does by default when
// there are more cores than devices -- for up to MI355X_SPIN_WAIT_US microseconds (default 200 000;
// 0 = sleep at once), with a yield every few polls; only then does the thread go to sleep.
int64_t spin_wait_us()
{
    static const int64_t v = [] {
        const char *e = getenv("MI355X_SPIN_WAIT_US");
        return e ? std::max<int64_t>(0, atoll(e)) : (int64_t)200000;
    }();
    return v;
}
hipError_t wait_stream(hipStream_t s)
{
    const int64_t limit = spin_wait_us();
    if (limit > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int polls = 1;; ++polls) {
            const hipError_t e = hipStreamQuery(s);
            if (e == hipSuccess) return hipSuccess;
            if (e != hipErrorNotReady) return e;
            (void)hipGetLastError();                      // hipErrorNotReady is sticky in the runtime's last-error slot
            if ((polls & 15) == 0) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(limit)) break;
                if ((polls & 255) == 0) std::this_thread::yield();
            }
        }
    }
    return hipStreamSynchronize(s);
}

// The status read-back behind a request: the first n control blocks in t->h_ctl when this returns.
// Default (g_ctl_wait 2): k_ctl_publish behind the request and a poll of its sequence number in pinned
// memory -- no runtime call between the GPU's last store and the host's next instruction; if the number
// has not arrived after spin_wait_us() (a request longer than that, or a fault: the stream wait then
// reports it) the thread sleeps in hipStreamSynchronize like everybody else.  1: copy + polled stream
// query, 0: copy + hipStreamSynchronize (mi355x_tune_set_ctl_wait: the A/B of tools/steady_gap.py).
// (process-wide knobs read by every solving thread: atomics; the measurement below is per THREAD -- round-5 advisor
// finding: plain globals written from the worker threads of multibatches and column partitions were a data race)
static std::atomic<int> g_ctl_wait{2};
void set_ctl_wait(int mode) { g_ctl_wait.store((mode >= 0 && mode <= 2) ? mode : 2, std::memory_order_relaxed); }
// where the calling thread's last read-back's host time went (mi355x_debug_last_wait): launching k_ctl_publish, polling its number
static thread_local double g_last_wait_us[2] = {0.0, 0.0};
static inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    std::this_thread::yield();
#endif
}

int read_ctls(mi355x_tab *t, int64_t n)
{
    const int ctl_wait = g_ctl_wait.load(std::memory_order_relaxed);
    if (ctl_wait == 2 && t->h_seq && spin_wait_us() > 0) {
        const unsigned long long seq = ++t->seq_next;
        const auto tl = std::chrono::steady_clock::now();
        launch_ctl_publish(t->v, n, t->h_ctl, t->h_seq, seq, t->stream);
        HIP_TRY(hipGetLastError());
        const auto t0 = std::chrono::steady_clock::now();
        g_last_wait_us[0] = std::chrono::duration<double, std::micro>(t0 - tl).count();
        const auto limit = std::chrono::microseconds(spin_wait_us());
        for (int polls = 1;; ++polls) {
            if (__atomic_load_n(t->h_seq, __ATOMIC_ACQUIRE) == seq) {
                g_last_wait_us[1] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
                return MI_OK;
            }
            cpu_relax();
            if ((polls & 63) == 0 && std::chrono::steady_clock::now() - t0 > limit) break;
        }
        HIP_TRY(hipStreamSynchronize(t->stream));
        if (__atomic_load_n(t->h_seq, __ATOMIC_ACQUIRE) != seq)
            return fail(MI_HIP_ERROR, "the control block did not arrive although the stream is idle");
        return MI_OK;
    }
    HIP_TRY(hipMemcpyAsync(t->h_ctl, t->v.ctl, (size_t)n * sizeof(Ctl), hipMemcpyDeviceToHost, t->stream));
    if (ctl_wait == 0) HIP_TRY(hipStreamSynchronize(t->stream));
    else                 HIP_TRY(wait_stream(t->stream));
    return MI_OK;
}
int read_ctl(mi355x_tab *t) { return read_ctls(t, 1); }

// ---- representation changes (DESIGN.md 4.5) -------------------------------------------
TabView &cur(mi355x_tab *t) { return t->compact ? t->c : t->v; }

// Rebuild the dense logical tableau from the compact representation (no-op when dense).
int ensure_dense(mi355x_tab *t)
{
    if (!t->compact) return MI_OK;
    if (!t->v.M) {                                    // handle born compact (mi355x_tab_create_compact)
        HIP_TRY(hipMalloc((void **)&t->v.M, (size_t)t->v.n_lps * t->v.rows * t->v.ld * sizeof(double)));
    }
    launch_expand(t->v, t->c, t->brow, t->stream);
    HIP_TRY(hipGetLastError());
    t->compact = false;
    t->n_part = 0;
    return MI_OK;
}

// Switch to [non-basic columns | RHS] if the basis columns are exactly unit vectors (they are
// for everything build-tableau produces and stay so under pivoting); otherwise stay dense.
int ensure_compact(mi355x_tab *t)
{
    TabView &v = t->v;
    const int64_t m = v.rows - 1, vc = v.cols - 1, n_nb = vc - m, nl = v.n_lps;
    if (t->compact || !t->tn.compact_enabled || t->compact_failed || m < 1 || n_nb < 1) return MI_OK;
    if (v.p2l) return MI_OK;                          // a compact column shard stays as it is
    t->compact_failed = true;                         // until proven otherwise
    std::vector<int64_t> basis((size_t)(nl * m));
    HIP_TRY(hipMemcpyAsync(basis.data(), v.basis, nl * m * sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    std::vector<int64_t> l2p((size_t)(nl * vc), 0), p2l((size_t)(nl * n_nb), 0);
    for (int64_t k = 0; k < nl; ++k) {                // every LP of a batch must qualify
        int64_t *l = l2p.data() + k * vc, *p = p2l.data() + k * n_nb;
        for (int64_t i = 0; i < m; ++i) {
            const int64_t b = basis[(size_t)(k * m + i)];
            if (b < 0 || b >= vc || l[b] == -1) return MI_OK;           // out of range / repeated
            l[b] = -1;
        }
        int64_t slot = 0;
        for (int64_t cidx = 0; cidx < vc; ++cidx)
            if (l[cidx] != -1) { l[cidx] = slot; p[slot++] = cidx; }
    }
    if (!t->flag) HIP_TRY(hipMalloc((void **)&t->flag, sizeof(int)));
    HIP_TRY(hipMemsetAsync(t->flag, 0, sizeof(int), t->stream));
    launch_verify_basis(v, t->flag, t->stream);
    int bad = 1;
    HIP_TRY(hipMemcpyAsync(&bad, t->flag, sizeof(int), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    if (bad) return MI_OK;
    if (t->c.cols != n_nb + 1) {                      // first time: describe the compact view
        t->c = v;                                     // shares every auxiliary buffer
        t->c.M = nullptr; t->c.p2l = nullptr; t->c.l2p = nullptr;
        t->c.cols = n_nb + 1;
        t->c.ld = padded_ld(n_nb + 1);
        if (nl > 1) { t->c.zs_M = v.rows * t->c.ld; t->c.zs_p2l = n_nb; t->c.zs_l2p = vc; }
    }
    // allocate whatever is still missing (a failed attempt must not leave a half-built view)
    if (!t->c.M) {
        HIP_TRY(hipMalloc((void **)&t->c.M, (size_t)nl * v.rows * t->c.ld * sizeof(double)));
        poison(t->c.M, (size_t)nl * v.rows * t->c.ld * sizeof(double), t->stream);
    }
    if (!t->c.p2l) HIP_TRY(hipMalloc((void **)&t->c.p2l, nl * n_nb * sizeof(int64_t)));
    if (!t->c.l2p) HIP_TRY(hipMalloc((void **)&t->c.l2p, nl * vc * sizeof(int64_t)));
    if (!t->brow)  HIP_TRY(hipMalloc((void **)&t->brow, nl * vc * sizeof(int64_t)));
    HIP_TRY(hipMemcpyAsync(t->c.p2l, p2l.data(), nl * n_nb * sizeof(int64_t), hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipMemcpyAsync(t->c.l2p, l2p.data(), nl * vc * sizeof(int64_t), hipMemcpyHostToDevice, t->stream));
    launch_compact(v, t->c, t->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(t->stream));         // p2l / l2p host vectors go out of scope
    t->compact = true;
    t->compact_failed = false;
    t->unit_basis = true;
    t->n_part = 0;
    // the exchange buffer of the resident solve belongs to the representation, not to the first solve
    // (an allocation and a memset of 0.1 .. 4 MB would otherwise sit inside that solve: 20 us of config
    // 2's 1.2 ms)
    if (!t->res_x && t->tn.resident_mode != 1 && resident_plan(t->c, nullptr)) {
        const size_t bytes = resident_xbuf_bytes(t->c);
        HIP_TRY(hipMalloc((void **)&t->res_x, bytes));
        HIP_TRY(hipMemsetAsync(t->res_x, 0, bytes, t->stream));
        HIP_TRY(hipStreamSynchronize(t->stream));
        t->res_epoch = 1;
    }
    return MI_OK;
}

// A select met an inf / NaN in the entering column while on the compact representation
// (status kNeedDense, the pivot was not applied): the reference would turn basic columns into
// NaNs, so go back to the dense logical tableau for good and let the pivot be redone there.
int fall_back_to_dense(mi355x_tab *t)
{
    int rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    t->compact_failed = true;
    t->unit_basis = false;
    launch_ctl_resume(t->v, t->stream, kNeedDense);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// select of one iteration; prices from the partials of the preceding update when they exist
void enqueue_select(mi355x_tab *t, int is_max, double f)
{
    const int np = (t->n_part > 0 && t->part_is_max == (is_max ? 1 : 0)) ? t->n_part : 0;
    // single-workgroup select for small tableaux (fewest launches), split select for large
    // ones (the strided column gather needs many workgroups' memory pipelines)
    const TabView &v = cur(t);
    bool split = (v.rows > 1024 || v.ld > 4096);
    if (t->tn.select_mode == 1) split = false;
    if (t->tn.select_mode == 2) split = true;
    if (split && select_split_supported(v)) { launch_select_split(v, is_max, f, np, t->stream); t->path_counts[kPathSelectSplit]++; }
    else                                    launch_select(v, is_max, f, np, t->stream);
}

// update of one iteration (+ optional event pair around it); prices the new objective row
int enqueue_update(mi355x_tab *t, int is_max)
{
    const bool timed = t->timing_stride > 0 && t->n_timed < kTimingCap &&
                       (t->update_launches++ % t->timing_stride) == 0;
    if (timed) {
        if ((int)t->ev0.size() <= t->n_timed) {
            hipEvent_t a, b;
            HIP_TRY(hipEventCreate(&a));
            HIP_TRY(hipEventCreate(&b));
            t->ev0.push_back(a);
            t->ev1.push_back(b);
        }
        HIP_TRY(hipEventRecord(t->ev0[t->n_timed], t->stream));
    }
    t->n_part = launch_update(cur(t), is_max ? 1.0 : -1.0, 1, t->stream, t->sweeps++);
    t->path_counts[kPathPerPivot]++;
    t->part_is_max = is_max ? 1 : 0;
    if (timed) {
        HIP_TRY(hipEventRecord(t->ev1[t->n_timed], t->stream));
        t->n_timed++;
    }
    return MI_OK;
}

int enqueue_iteration(mi355x_tab *t, int is_max, double f)
{
    enqueue_select(t, is_max, f);
    return enqueue_update(t, is_max);
}

// ---- blocked pivoting (DESIGN.md 4.8): k look-ahead selects, then one sweep applies them all
// pivots per sweep of this handle: the knob as it was when the handle was created, or by size --
// 16 wherever the persistent look-ahead runs (its state lives in LDS), a wide block where the
// sweep dominates (wide_block_default), 16 otherwise
int block_size(const mi355x_tab *t)
{
    if (t->tn.block_k != 0) return t->tn.block_k;
    if (t->tn.la_mode != 1 && !t->la_lost && la_block_supported(t->c)) {
        // the persistent look-ahead holds up to 24 pending pivots: 24 per pass from 28 MiB of stored tableau
        // on, 16 where the stored tableau sits in the L2s and the one-launch k_sweep16 is the faster form.
        // Measured per pivot, 16 / 24 per pass (round 5, one-launch ring pass with one round of workgroups):
        // 24 MB stored 7.11 / 7.29 us, 33 MB 7.93 / 7.73, 40 MB 8.01 / 7.81, 45 MB 8.37 / 7.92,
        // 54 MB 8.61 / 7.96, 78 MB 8.62 / 8.12, 100 MB 9.16 / 8.33, 268 MB (config 3) 12.0 / 11.3
        // (round 4, two-launch pass: the switch was at 100 MB)
        const int64_t stored = t->c.rows * t->c.ld * (int64_t)sizeof(double);
        // More than 32 workgroups (records per workgroup, round 5): the persistent step saves 3 us of a pivot
        // (395 MB stored 16.3 against 19.4 us per pivot, 649 MB 20.3 / 23.3, 1.06 GB 26.4 / 29.2, 2.05 GB
        // 41.4 / 43.4) -- until the pass is so long that 28 pivots per pass behind the two-launch look-ahead win
        // it back: 2.3 GB 48.6 against 48.0, 4.1 GB 77.0 / 73.0 (tools/la_wide_ab.py, DESIGN_experiments.md
        // R5.18).  So where wide_block_default asks for more than the 24 pivots this look-ahead can hold
        // (from 2e9 bytes on), these shapes keep the two-launch form -- unless the persistent one is forced.
        const bool wide_wins = la_block_workgroups(t->c) > kLaWaveRecordsMaxNw && t->tn.la_mode != 2 &&
                               wide_block_default(t->c) > kLaBlockMax;
        if (!wide_wins) return (stored >= (28ll << 20) && t->c.bk_smask2) ? kLaBlockMax : kMaxBlock;
    }
    const int w = wide_block_default(t->c);
    return w ? w : kMaxBlock;
}

bool block_mode(const mi355x_tab *t)
{
    if (t->tn.block_k == 1 || !t->compact || !block_supported(t->c)) return false;
    if (t->tn.select_mode == 1) return false;             // forced: single-workgroup select, per pivot
    if (t->tn.select_mode == 2) return true;
    // the persistent look-ahead pays at every size (a step costs less than the select + update
    // launches of one pivot); the two-launches-per-step form only where the split select is used
    if (t->tn.la_mode != 1 && la_block_supported(t->c)) return true;
    return t->c.rows > 1024 || t->c.ld > 4096;
}

// The FIRST launch of a kernel in a process is not free (the runtime looks the function up in the code
// object and sets its queue up for the kernel's LDS / register needs: measured on config 3, a 20-pivot
// request whose two kernels had not run before took 467 us, the same request afterwards 256 us).  A
// request of n pivots picks its kernels by n (full blocks of 24, a block of 20, one of <= 16 by its
// size), so a caller's warm-up request does not in general touch what the next request runs.  The
// first block a handle enqueues is therefore preceded by one EMPTY block of every form its requests
// can pick: a look-ahead of 0 steps (it only starts a new, empty pending list under its own stamp)
// and the sweep for that list (kk = 0: its workgroups leave before touching the tableau).  Persistent
// look-ahead only: under stamp 0 a sweep would take the previous block's list for its own.
static std::atomic<int> g_prime{1};
void set_prime(int on) { g_prime.store(on ? 1 : 0, std::memory_order_relaxed); }
// What priming warms -- a kernel's first launch: code-object lookup, queue set-up for its LDS / register needs -- is a
// property of the PROCESS and the DEVICE, not of a handle (round-5 advisor finding: every new tableau enqueued up to
// seven empty look-ahead + sweep pairs, and the native route makes a fresh handle per solve).  Which forms have been
// launched once is therefore kept per device; a handle only launches what nobody has yet.
static std::mutex g_primed_mutex;
static std::vector<std::vector<uint64_t>> g_primed_keys;         // [device] -> keys of the (look-ahead, sweep) forms launched once
static bool primed_on_device(int device, uint64_t key, bool mark)
{
    std::lock_guard<std::mutex> lock(g_primed_mutex);
    if ((size_t)device >= g_primed_keys.size()) g_primed_keys.resize((size_t)device + 1);
    auto &v = g_primed_keys[(size_t)device];
    const bool had = std::find(v.begin(), v.end(), key) != v.end();
    if (!had && mark) v.push_back(key);
    return had;
}

int prime_block_kernels(mi355x_tab *t, int is_max, double f)
{
    const TabView &v = t->c;
    const int bk = block_size(t);
    const int la_nw = la_launch_workgroups(v);
    int forms[8], nf = 0;
    if (bk > kMaxBlock) { forms[nf++] = bk; forms[nf++] = 20; }
    forms[nf++] = kMaxBlock; forms[nf++] = kMaxBlock - 1; forms[nf++] = 8; forms[nf++] = 4; forms[nf++] = 2;
    for (int i = 0; i < nf; ++i) {
        if (forms[i] > kMaxBlock && !v.bk_smask2) continue;
        if (t->la_epoch > 0x7fff0000u) break;
        // the kernel instantiations behind this form: the look-ahead by (16 | 24 pending pivots, record per wave |
        // per workgroup), the sweep by the number of links and by the size class that picks its cache policy
        const double bytes = (double)v.rows * (double)v.ld * 8.0;
        const uint64_t key = (uint64_t)forms[i] | ((uint64_t)(la_nw > kLaWaveRecordsMaxNw) << 8) |
                             ((uint64_t)(bytes > 240.0 * 1024 * 1024) << 9) | ((uint64_t)(bytes > 320.0 * 1024 * 1024) << 10) |
                             ((uint64_t)(bytes < (28ll << 20)) << 11);
        if (primed_on_device(t->device, key, true)) continue;
        launch_la_block_form(v, forms[i], 0, is_max, f, t->la_epoch, t->stream);   // (the 16- and the 24-step look-ahead are two kernels)
        (void)launch_sweep(v, forms[i], is_max ? 1.0 : -1.0, t->stream, t->la_epoch, la_nw);
        t->la_epoch += 2 * kLaBlockMax + 2;
    }
    t->la_last_nw = la_nw;
    t->n_part = 0;                                             // (no sweep above priced anything)
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

int enqueue_block(mi355x_tab *t, int is_max, double f, int k)
{
    const TabView &v = t->c;
    if (!t->primed) {
        t->primed = true;
        if (g_prime.load(std::memory_order_relaxed) && t->tn.la_mode != 1 && !t->la_lost && block_size(t) <= kLaBlockMax && la_block_supported(v)) {
            const int rc = prime_block_kernels(t, is_max, f);
            if (rc != MI_OK) return rc;
        }
    }
    int np = (t->n_part > 0 && t->part_is_max == (is_max ? 1 : 0)) ? t->n_part : 0;
    // (a handle that lost an exchange runs the two-launch form, forced mode 2 or not: re-launching the
    // persistent kernel block after block on a GPU that cannot co-schedule its workgroups would cost a
    // time-out per block.  It is re-armed after la_rearm_in clean blocks -- 1024 after the first loss,
    // four times as many after each further one -- so a GPU that was shared for a while does not leave
    // a long-lived handle ~2 x slower for good, and one that stays shared pays a time-out ever more rarely)
    if (t->la_lost && t->la_rearm_in > 0 && --t->la_rearm_in == 0 && t->tn.block_k == 0) {
        t->la_lost = false;
        t->primed = false;                            // (the persistent forms may never have run in this process: look again)
    }
    const bool persistent = t->tn.la_mode != 1 && !t->la_lost && k <= kLaBlockMax && block_size(t) <= kLaBlockMax &&
                            la_block_supported(v) && (k <= kMaxBlock || v.bk_smask2);
    // event pairs around FULL blocks only: the statistics are per (look-ahead of g_block_k
    // pivots, sweep of g_block_k pivots), the partial last block of a run is left out
    const bool timed = t->timing_stride > 0 && t->n_timed < kTimingCap && k == block_size(t) &&
                       (t->update_launches++ % t->timing_stride) == 0;
    auto ensure_events = [](std::vector<hipEvent_t> &a, std::vector<hipEvent_t> &b, int n) -> hipError_t {
        while ((int)a.size() <= n) {
            hipEvent_t x, y;
            hipError_t e = hipEventCreate(&x);
            if (e != hipSuccess) return e;
            if ((e = hipEventCreate(&y)) != hipSuccess) { (void)hipEventDestroy(x); return e; }
            a.push_back(x);
            b.push_back(y);
        }
        return hipSuccess;
    };
    if (timed) {
        HIP_TRY(ensure_events(t->la0, t->la1, t->n_timed_la));
        HIP_TRY(ensure_events(t->ev0, t->ev1, t->n_timed));
        HIP_TRY(hipEventRecord(t->la0[t->n_timed_la], t->stream));
    }
    unsigned stamp = 0;
    int la_nw = 0;
    t->last_was_resident = false;
    if (persistent) {
        if (t->la_epoch > 0x7fff0000u) {              // 32-bit tags: start over on clean records
            HIP_TRY(hipMemsetAsync(v.la_px, 0, kLaRecordBytes, t->stream));
            HIP_TRY(hipMemsetAsync(v.la_rx, 0, kLaRecordBytes, t->stream));
            t->la_epoch = 1;
        }
        stamp = t->la_epoch;
        la_nw = la_launch_workgroups(v);
        launch_la_block(v, k, is_max, f, t->la_epoch, t->stream);
        t->la_last_nw = la_nw;
        t->la_epoch += 2 * kLaBlockMax + 2;
        t->path_counts[kPathLaPersistent]++;
    } else {
        for (int j = 0; j < k; ++j) np = launch_lookahead(v, j, is_max, f, np, t->stream);
        t->path_counts[kPathLaTwoLaunch]++;
    }
    if (timed) {
        HIP_TRY(hipEventRecord(t->la1[t->n_timed_la], t->stream));
        t->n_timed_la++;
        HIP_TRY(hipEventRecord(t->ev0[t->n_timed], t->stream));
    }
    t->n_part = launch_sweep(v, k, is_max ? 1.0 : -1.0, t->stream, stamp, la_nw);
    t->path_counts[sweep_kind(k) == 2 ? kPathSweepWide : (sweep_kind(k) == 1 ? kPathSweep16 : kPathSweepShort)]++;
    t->part_is_max = is_max ? 1 : 0;
    if (timed) {
        HIP_TRY(hipEventRecord(t->ev1[t->n_timed], t->stream));
        t->n_timed++;
    }
    return MI_OK;
}

// The persistent look-ahead gave up waiting for a workgroup's record (status kSyncLost): its
// workgroups were not all resident at the same time -- a GPU shared with other work.  Every
// workgroup times out on its own, so the leader's workgroup may have committed one pivot more than
// some other workgroup completed (that one gave up on the ratio exchange whose records the leader
// still saw arrive).  The sweep that followed applied only the pivots EVERY workgroup completed
// (BlockCtl::done); the bookkeeping of the one beyond is taken back here (k_la_rollback), and
// everything enqueued behind the failed launch was a no-op.  Nothing is lost: continue on the
// two-launch look-ahead, which needs no co-residency, for the rest of this handle's life.
int recover_lost_exchange(mi355x_tab *t)
{
    t->n_part = 0;
    if (t->last_was_resident) {
        // the resident solve's workgroups were not co-resident at their first exchange: nothing was
        // modified (it writes the tableau back only at the end of a launch that got through)
        t->res_lost = true;
    } else {
        t->la_lost = true;
        t->la_rearm_in = (int64_t)1024 << (2 * std::min(t->la_losses, 8));
        t->la_losses++;
        if (t->la_last_nw) launch_la_rollback(t->c, t->la_last_nw, t->stream);
    }
    launch_ctl_resume(t->v, t->stream, kSyncLost);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

int status_to_rc(int32_t st) { return st == kRunning ? MI_RUNNING : (int)st; }

// ---- the resident solve (tableaux that fit the register files; simplex_kernels.hip, k_resident)
bool knobs_at_default(const TuneSnapshot &k)
{
    return k.select_mode == 0 && k.la_mode == 0 && k.block_k == 0 && k.batch_mode == 0 && k.batch_block_k == 0;
}

bool resident_mode(const mi355x_tab *t)
{
    if (!t->compact || t->res_lost || t->tn.resident_mode == 1) return false;
    if (t->tn.resident_mode == 0 && !knobs_at_default(t->tn)) return false;   // an explicit knob asks for another path
    return resident_plan(t->c, nullptr);
}

// one launch of up to `cap` pivots per LP (cap <= 65536)
int enqueue_resident(mi355x_tab *t, int is_max, double f, int cap)
{
    if (!t->res_x) {
        const size_t bytes = resident_xbuf_bytes(t->c);
        HIP_TRY(hipMalloc((void **)&t->res_x, bytes));
        HIP_TRY(hipMemsetAsync(t->res_x, 0, bytes, t->stream));
        t->res_epoch = 1;
    }
    if (t->res_epoch > 0x7ffe0000u) {                 // 32-bit tags: start over on clean buffers
        HIP_TRY(hipMemsetAsync(t->res_x, 0, resident_xbuf_bytes(t->c), t->stream));
        t->res_epoch = 1;
    }
    // (mi355x_tab_timing_*: a resident launch is bracketed like an update launch)
    const bool timed = t->timing_stride > 0 && t->n_timed < kTimingCap &&
                       (t->update_launches++ % t->timing_stride) == 0;
    if (timed) {
        if ((int)t->ev0.size() <= t->n_timed) {
            hipEvent_t a, b;
            HIP_TRY(hipEventCreate(&a));
            HIP_TRY(hipEventCreate(&b));
            t->ev0.push_back(a);
            t->ev1.push_back(b);
        }
        HIP_TRY(hipEventRecord(t->ev0[t->n_timed], t->stream));
    }
    if (!launch_resident(t->c, t->res_x, is_max, f, cap, t->res_epoch, t->stream))
        return fail(MI_BAD_ARG, "resident launch refused");
    if (timed) {
        HIP_TRY(hipEventRecord(t->ev1[t->n_timed], t->stream));
        t->n_timed++;
    }
    t->res_epoch += (unsigned)cap + 2u;
    t->path_counts[kPathResident]++;
    t->last_was_resident = true;
    t->n_part = 0;                                    // no pricing partials are left behind
    return MI_OK;
}

// A way out of a solve (the reference has no pivot cap and no anti-cycling rule, simplex.lisp:453-461;
// in Lisp a cycling LP is interruptible, a blocking foreign call is not).  Every blocking solve loop
// enqueues BOUNDED chunks of launches -- at most 64 blocks, 512 per-pivot iterations, one resident
// launch of 65536 pivots, 4096 pivots of a per-LP batch kernel -- and looks at this flag whenever it
// has read the status back, i.e. when everything enqueued has completed and the tableau is whole.
bool take_cancel(mi355x_tab *t)
{
    const bool own = t->cancel.exchange(0, std::memory_order_acq_rel) != 0;
    const bool peer = t->cancel_peer && t->cancel_peer->exchange(0, std::memory_order_acq_rel) != 0;
    return own || peer;
}
// A request is aimed at the solve in flight (or, with none in flight, at the next one): whichever
// way that solve ends, the request ends with it.  Inside mi355x_solve_two_phase the CALL is the
// solve in flight: a phase that ends leaves the flags alone (TwoPhaseCancelScope clears them).
struct CancelScope {
    mi355x_tab *t;
    explicit CancelScope(mi355x_tab *tab) : t(tab) {}
    ~CancelScope() { if (!t->cancel_scoped_outside) t->cancel.store(0, std::memory_order_release); }
};
struct FlagCancelScope {                  // the same for a handle that owns a flag of its own (column partition)
    std::atomic<int> &f;
    explicit FlagCancelScope(std::atomic<int> &flag) : f(flag) {}
    ~FlagCancelScope() { f.store(0, std::memory_order_release); }
};
struct TwoPhaseCancelScope {
    mi355x_tab *a, *b;
    TwoPhaseCancelScope(mi355x_tab *x, mi355x_tab *y) : a(x), b(y)
    {
        a->cancel_peer = &b->cancel; b->cancel_peer = &a->cancel;
        a->cancel_scoped_outside = b->cancel_scoped_outside = true;
    }
    ~TwoPhaseCancelScope()
    {
        a->cancel_peer = b->cancel_peer = nullptr;
        a->cancel_scoped_outside = b->cancel_scoped_outside = false;
        a->cancel.store(0, std::memory_order_release);
        b->cancel.store(0, std::memory_order_release);
    }
};

// per-LP outcome of a batch as the host mirror of the control blocks holds it (an LP a cancelled
// solve left unfinished reports MI_RUNNING; its tableau is whole, a later solve call carries on)
int batch_report(mi355x_tab *t, int32_t *status, int64_t *n_pivots, int rc)
{
    for (int64_t i = 0; i < t->v.n_lps; ++i) {
        if (status) status[i] = status_to_rc(t->h_ctl[i].status);
        if (n_pivots) n_pivots[i] = t->h_ctl[i].n_pivots;
    }
    return rc;
}

}  // namespace
