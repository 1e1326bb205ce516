// capi_assemble.inc -- what the entries that have the device build tableaux share on the host: the check of members
// given as problem rows, and the (main, artificial) pair of double-precision batches around an assembly, on one
// device and split over several.  Part of simplex_capi.hip (ONE translation unit: included there after
// capi_batch.inc, whose mb_layout and mb_free it uses; alloc_tab and free_tab are capi_tab_impl.inc's).

namespace {

// one member's part of lps_check (and of the ragged create, whose members have shapes of their own): its rows
// (m + 1) x (ncv + 1) and m senses -> its `=` rows and its artificial rows (:243-252)
template <class T>
int lps_member_counts(int64_t q, int64_t m, int64_t ncv, const T *rows, const int32_t *sense, int64_t *n_eq, int64_t *n_art)
{
    const int64_t W = ncv + 1;
    int64_t e = 0, a = 0;
    for (int64_t i = 0; i < m; ++i) {
        const int32_t s = sense[i];
        if (s < 0 || s > 2) return fail(MI_BAD_ARG, "member %lld: sense %d of row %lld", (long long)q, (int)s, (long long)i);
        e += s == 2;
        a += row_word_artificial(row_word(rows[i * W + ncv] < T(0), s));            // :243-252
    }
    *n_eq = e; *n_art = a;
    return MI_OK;
}

// the argument checks of the create-from-rows entries (no device is looked for): the numbers of `=` rows and of
// artificial rows every member has.  O(m) per member: only the signs of the right-hand sides are read (T: double,
// float, or the numerators of reduced fractions).  max_lps_log2: the entry's limit on n_lps (0: none).
template <class T>
int lps_check(int64_t n_lps, int max_lps_log2, int64_t m, int64_t ncv, const T *lps, const int32_t *sense, int64_t *n_eq_out,
              int64_t *n_art_out)
{
    if (!lps) return fail(MI_BAD_ARG, "lps is NULL");
    if (!sense) return fail(MI_BAD_ARG, "sense is NULL");
    if (n_lps < 1 && !max_lps_log2) return fail(MI_BAD_ARG, "n_lps=%lld must be >= 1", (long long)n_lps);
    if (n_lps < 1 || (max_lps_log2 && n_lps > (1LL << max_lps_log2)))
        return fail(MI_BAD_ARG, "n_lps=%lld must be in [1, 2^%d]", (long long)n_lps, max_lps_log2);
    if (m < 1 || ncv < 1) return fail(MI_BAD_ARG, "m=%lld ncv=%lld must be >= 1", (long long)m, (long long)ncv);
    if (m > (1 << 24) || ncv > (1 << 24)) return fail(MI_BAD_ARG, "m=%lld ncv=%lld out of range", (long long)m, (long long)ncv);
    const int64_t per = (m + 1) * (ncv + 1);
    int64_t n_eq = -1, n_art = -1;
    for (int64_t q = 0; q < n_lps; ++q) {
        int64_t e = 0, a = 0;
        const int rc = lps_member_counts(q, m, ncv, lps + q * per, sense + q * m, &e, &a);
        if (rc != MI_OK) return rc;
        if (n_eq >= 0 && (e != n_eq || a != n_art))
            return fail(MI_BAD_ARG, "member %lld has %lld `=` and %lld artificial rows, the members before it %lld and %lld",
                        (long long)q, (long long)e, (long long)a, (long long)n_eq, (long long)n_art);
        n_eq = e; n_art = a;
    }
    *n_eq_out = n_eq; *n_art_out = n_art;
    return MI_OK;
}

mi355x_batch *batch_of(mi355x_tab *t)
{
    mi355x_batch *b = new (std::nothrow) mi355x_batch;
    if (b) b->t = t;
    return b;
}

// n members on one device: t[0] the main batch (rows x cols), t[1] the artificial one (n_art more columns) or NULL,
// filled by fill(stream, main view, artificial view, mem) -> MI_*: uploads and launches on that stream, with
// mem_bytes of device memory of their own (freed here once the stream is idle).  Both end in the state upload() leaves.
template <class Fill>
int tab_pair_build(mi355x_tab *t[2], int64_t n, int64_t rows, int64_t cols, int64_t n_art, int device, size_t mem_bytes, Fill fill)
{
    auto hip = [](hipError_t e) {
        return e == hipSuccess ? MI_OK : fail(e == hipErrorOutOfMemory ? MI_NO_MEMORY : MI_HIP_ERROR, "device assembly failed: %s",
                                              hipGetErrorString(e));
    };
    t[0] = t[1] = nullptr;
    void *mem = nullptr;
    int rc = alloc_tab(&t[0], rows, cols, device, n);
    if (rc == MI_OK && n_art) rc = alloc_tab(&t[1], rows, cols + n_art, device, n);
    if (rc == MI_OK) rc = hip(hipMalloc(&mem, mem_bytes));
    // alloc_tab left memsets of the artificial batch's basis and control blocks on ITS stream; the assembly
    // writes both from the main batch's stream, so those memsets have to be over first
    // (which stream the hardware serves first decided the outcome: no deterministic test can show it; the
    // random searches of tests/test_gpu_branch_and_bound.py failed now and then without this wait)
    if (rc == MI_OK && t[1]) rc = hip(hipStreamSynchronize(t[1]->stream));
    if (rc == MI_OK) {
        hipStream_t st = t[0]->stream;
        rc = fill(st, t[0]->v, t[1] ? t[1]->v : TabView{}, (char *)mem);
        if (rc == MI_OK) {
            launch_ctl_reset(t[0]->v, 0, 1, st);
            if (t[1]) launch_ctl_reset(t[1]->v, 0, 1, st);
            rc = hip(hipGetLastError());
        }
        const hipError_t e = hipStreamSynchronize(st);              // (the caller's arrays and `mem` may go)
        if (rc == MI_OK) rc = hip(e);
    }
    if (mem) (void)hipFree(mem);
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

// the same over several devices, the split of mi355x_multibatch_create: pair(t, k0, count, device) -> MI_* builds the
// pair of the sub-batch that holds members [k0, k0 + count)
template <class Pair>
int multibatch_pair_build(mi355x_multibatch **out_main, mi355x_multibatch **out_art, int64_t n, int64_t rows, int64_t cols,
                          int64_t n_art, int n_devices, const int *device_ids, Pair pair)
{
    mi355x_multibatch *mb[2] = {new (std::nothrow) mi355x_multibatch, n_art ? new (std::nothrow) mi355x_multibatch : nullptr};
    auto cleanup = [&](int code) { mb_free(mb[0]); mb_free(mb[1]); return code; };
    if (!mb[0] || (n_art && !mb[1])) return cleanup(fail(MI_NO_MEMORY, "host allocation failed"));
    std::vector<int> devs;
    int nd = n_devices;
    int rc = mb_layout(mb[0], n, rows, cols, &nd, device_ids, devs);
    if (rc == MI_OK && mb[1]) { int nd2 = n_devices; std::vector<int> dv2; rc = mb_layout(mb[1], n, rows, cols + n_art, &nd2, device_ids, dv2); }
    if (rc != MI_OK) return cleanup(rc);
    std::vector<int64_t> f2;
    for (int s = 0; s < nd; ++s) {
        const int64_t k0 = mb[0]->first[(size_t)s], k1 = mb[0]->first[(size_t)s + 1];
        if (k1 <= k0) continue;                                   // (an empty sub-batch: first[] keeps only the boundaries in use)
        mi355x_tab *t[2];
        rc = pair(t, k0, k1 - k0, devs[(size_t)s]);
        if (rc != MI_OK) return cleanup(rc);
        for (int w = 0; w < 2 && t[w]; ++w) {
            mi355x_batch *bt = batch_of(t[w]);
            if (!bt) { free_tab(t[w]); rc = fail(MI_NO_MEMORY, "host allocation failed"); continue; }
            mb[w]->sub.push_back(bt);
        }
        if (rc != MI_OK) return cleanup(rc);
        f2.push_back(k0);
    }
    f2.push_back(n);
    mb[0]->first = f2;
    if (mb[1]) mb[1]->first = f2;
    *out_main = mb[0];
    if (out_art) *out_art = mb[1];
    return MI_OK;
}

}  // namespace
