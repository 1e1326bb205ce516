// capi_exact_lps.inc -- mi355x_xbatch_create_lps: batches of exact rational LPs whose start states the device
// builds from the members' problem rows (build-tableau, src/simplex.lisp:214-328, followed by x_start_state).
// Part of simplex_capi.hip (ONE translation unit: included there after capi_exact_bb.inc; the handle, xb_alloc /
// xb_fresh / ctl helpers are capi_exact_batch.inc's, x_objective_multipliers and x_check_device capi_exact.inc's).
//
// The rows stay on the device for the life of the handles (XbLps, shared by the main and the artificial batch of
// a group): a member that overflows 64 bits in a solve is assembled again from them at 128 bits
// (xb_restart_128), main and artificial slot alike.  The host keeps nothing per entry: it validates the
// fractions once, derives the hand-over multipliers from the objective rows, and reads the control blocks.

struct XbLps {
    int      device = 0;
    int64_t  m = 0, ncv = 0, n_slack = 0, n_art = 0;
    int64_t *num = nullptr, *den = nullptr;
    int32_t *sense = nullptr;
    const mi355x_xbatch *art = nullptr;       // the artificial batch of a two-phase group (compared, never followed)
    ~XbLps()
    {
        (void)hipSetDevice(device);
        (void)hipFree(num); (void)hipFree(den); (void)hipFree(sense);
    }
};

namespace {

XbLpsView xlp_view(const XbLps &l) { return XbLpsView{l.num, l.den, l.sense, l.m, l.ncv, l.n_slack, l.n_art}; }

// members [q0, q0 + count) of a group at `bits` into mt and / or art (NULL: left out), fresh control blocks first;
// afterwards h[q] holds the member's D, and its status is kXbIdle or kXOverflow.  MI_OK or an error.
int xlp_assemble(mi355x_xbatch *mt, mi355x_xbatch *art, int bits, int64_t q0, int64_t count, hipStream_t s)
{
    const int wi = xb_wi(bits);
    XbView views[2] = {XbView{}, XbView{}};
    mi355x_xbatch *hs[2] = {mt, art};
    for (int k = 0; k < 2; ++k) {
        if (!hs[k]) continue;
        const int rc = xb_alloc(hs[k], wi);
        if (rc != MI_OK) return rc;
        XbWidth &w = hs[k]->w[wi];
        for (int64_t q = q0; q < q0 + count; ++q) w.h[q] = xb_fresh(0);
        HIP_TRY(hipMemcpyAsync(w.v.ctl + q0, &w.h[q0], count * sizeof(XbCtl), hipMemcpyHostToDevice, s));
        views[k] = w.v;
    }
    launch_xb_assemble_lps(views[0], views[1], xlp_view(*(mt ? mt : art)->lps), q0, count, s);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < 2; ++k)
        if (hs[k]) {
            XbWidth &w = hs[k]->w[wi];
            HIP_TRY(hipMemcpyAsync(&w.h[q0], w.v.ctl + q0, count * sizeof(XbCtl), hipMemcpyDeviceToHost, s));
        }
    HIP_TRY(hipStreamSynchronize(s));
    return MI_OK;
}

int xlp_reassemble_128(mi355x_xbatch *b, int64_t q, hipStream_t s, __int128 *D0)
{
    const bool is_art = b->lps->art == b;
    const int rc = xlp_assemble(is_art ? nullptr : b, is_art ? b : nullptr, 128, q, 1, s);
    if (rc != MI_OK) return rc;
    if (b->w[1].h[q].status == kXOverflow) return kXOverflow;
    *D0 = b->w[1].h[q].D;
    return MI_OK;
}

// what the members [q0, q0 + count) of h left in their control blocks at `bits`: the width, or a fresh block
void xlp_settle(mi355x_xbatch *h, int bits, int64_t q0, int64_t count)
{
    XbWidth &w = h->w[xb_wi(bits)];
    for (int64_t q = q0; q < q0 + count; ++q) {
        if (w.h[q].status == kXOverflow) w.h[q] = xb_fresh(0);
        else                             h->width[q] = bits;
    }
}

// an empty batch of n members whose start states come from `lps`
mi355x_xbatch *xlp_new_batch(const std::shared_ptr<XbLps> &lps, int64_t n, int64_t rows, int64_t cols, bool start_ok)
{
    mi355x_xbatch *b = new (std::nothrow) mi355x_xbatch;
    if (!b) return nullptr;
    b->device = lps->device;
    b->n = n; b->rows = rows; b->cols = cols;
    b->lps = lps;
    b->start_ok.assign((size_t)n, start_ok ? 1 : 0);
    b->width.assign((size_t)n, 0);
    b->mult.assign((size_t)(n * (cols + 1)), 0);
    if (hipSetDevice(b->device) != hipSuccess || hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
        mi355x_xbatch_destroy(b);
        return nullptr;
    }
    return b;
}

uint64_t xlp_gcd(uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; }

}  // namespace

int mi355x_xbatch_create_lps(mi355x_xbatch **out_main, mi355x_xbatch **out_art, int64_t n_lps, int64_t m, int64_t ncv,
                             const int64_t *num, const int64_t *den, const int32_t *sense, int device, int min_bits)
{
    if (!out_main || !out_art) return fail(MI_BAD_ARG, "out is NULL");
    *out_main = *out_art = nullptr;
    if (n_lps < 1 || m < 1 || ncv < 1 || !num || !den || !sense) return fail(MI_BAD_ARG, "bad shape or NULL array");
    if (min_bits != 0 && min_bits != 64 && min_bits != 128) return fail(MI_BAD_ARG, "min_bits must be 0, 64 or 128");
    if (m > (1 << 24) || ncv > (1 << 24) || n_lps > (1 << 24)) return fail(MI_BAD_ARG, "shape out of range");
    const int64_t W = ncv + 1, per = (m + 1) * W;
    for (int64_t k = 0; k < n_lps * per; ++k) {
        const uint64_t a = num[k] < 0 ? 0 - (uint64_t)num[k] : (uint64_t)num[k];
        if (den[k] <= 0 || xlp_gcd(a, (uint64_t)den[k]) != 1)
            return fail(MI_BAD_ARG, "member %lld: entry %lld, %lld / %lld, is not a reduced fraction", (long long)(k / per),
                        (long long)(k % per), (long long)num[k], (long long)den[k]);
    }
    int64_t n_eq = 0, n_art = 0;
    int rc = lps_check(n_lps, 24, m, ncv, num, sense, &n_eq, &n_art);
    if (rc != MI_OK) return rc;
    rc = x_check_device(device);
    if (rc != MI_OK) return rc;
    const int64_t rows = m + 1, cols = ncv + (m - n_eq) + 1, nac = cols + n_art;
    if ((size_t)(rows + (n_art ? nac : cols)) * 16 > kXbSnapshotLimit)
        return fail(MI_UNSUPPORTED, "a %lld x %lld member's snapshots do not fit a workgroup's LDS", (long long)rows,
                    (long long)(n_art ? nac : cols));
    static_assert(kXbSnapshotLimit / 16 * 3 * sizeof(int32_t) + 5 * 1024 <= 64 * 1024,
                  "k_xb_assemble_lps keeps three int32 per row in LDS beside its reduction scratch");
    std::shared_ptr<XbLps> lps = std::make_shared<XbLps>();
    lps->device = device;
    lps->m = m; lps->ncv = ncv; lps->n_slack = m - n_eq; lps->n_art = n_art;
    const size_t ne = (size_t)(n_lps * per), ns = (size_t)(n_lps * m);
    HIP_TRY(hipSetDevice(device));
    if (hipMalloc((void **)&lps->num, ne * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void **)&lps->den, ne * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void **)&lps->sense, ns * sizeof(int32_t)) != hipSuccess)
        return fail(MI_NO_MEMORY, "device allocation failed");
    HIP_TRY(hipMemcpy(lps->num, num, ne * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lps->den, den, ne * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lps->sense, sense, ns * sizeof(int32_t), hipMemcpyHostToDevice));
    // the main batch: runnable on its own only without artificial rows (its basis names no column for them)
    mi355x_xbatch *mt = xlp_new_batch(lps, n_lps, rows, cols, n_art == 0);
    mi355x_xbatch *art = n_art ? xlp_new_batch(lps, n_lps, rows, nac, true) : nullptr;
    auto undo = [&](int code) { mi355x_xbatch_destroy(mt); mi355x_xbatch_destroy(art); return code; };
    if (!mt || (n_art && !art)) return undo(fail(MI_NO_MEMORY, "batch creation failed"));
    lps->art = art;
    // cl_j and L_c from the objective row as the main tableau holds it: the slack columns' entries are 0
    std::vector<int64_t> cn((size_t)cols, 0), cd((size_t)cols, 1);
    std::vector<i128_t> cl;
    for (int64_t q = 0; q < n_lps; ++q) {
        const int64_t *on = num + q * per + m * W, *od = den + q * per + m * W;
        std::copy(on, on + ncv, cn.begin());
        std::copy(od, od + ncv, cd.begin());
        cn[cols - 1] = on[ncv]; cd[cols - 1] = od[ncv];
        i128_t lc = 0;
        if (x_objective_multipliers(cols, cn.data(), cd.data(), &lc, cl)) {
            std::copy(cl.begin(), cl.end(), &mt->mult[q * (cols + 1)]);
            mt->mult[q * (cols + 1) + cols] = lc;
        }
    }
    hipStream_t s = mt->stream;
    const int first = min_bits == 128 ? 128 : 64;
    for (int bits = first; bits <= 128; bits += 64) {
        // one launch for the whole group at its first width; at 128 bits after 64 only the tableaux that need it
        mi355x_xbatch *hs[2] = {mt, art};
        if (bits == first) {
            rc = xlp_assemble(mt, art, bits, 0, n_lps, s);
            if (rc != MI_OK) return undo(rc);
            xlp_settle(mt, bits, 0, n_lps);
            if (art) xlp_settle(art, bits, 0, n_lps);
        } else {
            for (int k = 0; k < 2; ++k) {
                if (!hs[k]) continue;
                for (int64_t q = 0; q < n_lps; ++q) {
                    if (hs[k]->width[q] != 0) continue;
                    int64_t cnt = 1;
                    while (q + cnt < n_lps && hs[k]->width[q + cnt] == 0) ++cnt;
                    rc = xlp_assemble(k == 0 ? mt : nullptr, k == 1 ? art : nullptr, bits, q, cnt, s);
                    if (rc != MI_OK) return undo(rc);
                    xlp_settle(hs[k], bits, q, cnt);
                    q += cnt - 1;
                }
            }
        }
        for (int k = 0; k < 2; ++k)
            if (hs[k] && hs[k]->w[xb_wi(bits)].v.T && xb_write_ctl(hs[k], s) != MI_OK)
                return undo(fail(MI_HIP_ERROR, "upload of the control blocks failed"));
        if (hipStreamSynchronize(s) != hipSuccess) return undo(fail(MI_HIP_ERROR, "upload of the control blocks failed"));
    }
    *out_main = mt;
    *out_art = art;
    return MI_OK;
}
