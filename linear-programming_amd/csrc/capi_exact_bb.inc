// capi_exact_bb.inc -- exact branch-and-bound (simplex-solver on rationals, src/simplex.lisp:462-542): node
// batches assembled on the device and the light read-back.  Part of simplex_capi.hip (ONE translation
// unit: included there after capi_exact_batch.inc, whose handle, xb_alloc / xb_fresh / ctl helpers and
// capi_exact.inc's x_lcm / x_mul / x_start_state / x_objective_multipliers / x_put it uses).
//
// The search itself, build-tableau of the base problem and the reading of a solution stay in the host
// language, which has bignums; the library turns (base, node rows) into start states (k_xbb_assemble) and
// gathers what the read-back functions need (k_xbb_readback).
//
// The integer scale Db.  The fraction-free pivots divide exactly only when Db times every minor of the
// rational tableau is an integer, which the plain LCM of all denominators does not give (rows x/2 <= 1 and
// y/2 <= 1: LCM 2, the first pivot already leaves 1/2).  Db is therefore x_start_state's D of the base --
// the product of its rows' LCMs, the one the other exact handles start from -- times the LCM of the offsets'
// denominators: a node row's entries are integers except its right-hand side bound - offset, and a term
// of a minor holds at most one right-hand side.

struct XbbImage {                             // the base at one width
    void *B = nullptr, *voff = nullptr;
    bool  tried = false;
};

struct XbbBase {
    int      device = 0;
    int64_t  rows = 0, cols = 0, ncv = 0, nb = 0, n_vars = 0, n_art = 0;
    bool     start_ok = false;
    i128_t   Db = 0;
    std::vector<i128_t>  B, voff;             // Db * entry, Db * offset
    std::vector<int64_t> basis, vcol, off_num, off_den;
    std::vector<int32_t> kind;
    std::vector<i128_t>  cl;                  // the hand-over multipliers of the objective row (cols values), and
    i128_t   lc = 0;                          // L_c (0: they overflowed 128 bits)
    int64_t *d_basis = nullptr, *d_vcol = nullptr;
    int32_t *d_kind = nullptr;
    XbbImage img[2];
    std::mutex mu;                            // (the 128-bit image is made at its first use, by any thread)
    ~XbbBase()
    {
        (void)hipSetDevice(device);
        for (XbbImage &i : img) { (void)hipFree(i.B); (void)hipFree(i.voff); }
        (void)hipFree(d_basis); (void)hipFree(d_vcol); (void)hipFree(d_kind);
    }
};

struct mi355x_xbb_base { std::shared_ptr<XbbBase> p; };

struct XbbNodes {
    std::shared_ptr<XbbBase> base;
    int64_t  d = 0;
    int64_t *var = nullptr, *bound = nullptr;
    int32_t *sense = nullptr;
    const mi355x_xbatch *art = nullptr;       // the artificial batch of a two-phase group (compared, never followed)
    ~XbbNodes()
    {
        (void)hipSetDevice(base->device);
        (void)hipFree(var); (void)hipFree(bound); (void)hipFree(sense);
    }
};

namespace {

// the base at `bits` on its device: MI_OK, kXOverflow when it does not fit the width, or the device's error
// (a later call tries the upload again)
int xbb_image(XbbBase &b, int bits, XbbBaseView *out)
{
    std::lock_guard<std::mutex> lock(b.mu);
    XbbImage &im = b.img[xb_wi(bits)];
    if (!im.tried) {
        bool fits = x_fits(b.Db, bits);
        for (size_t k = 0; k < b.B.size() && fits; ++k) fits = x_fits(b.B[k], bits);
        for (size_t k = 0; k < b.voff.size() && fits; ++k) fits = x_fits(b.voff[k], bits);
        if (fits) {
            const size_t wb = bits / 8, nB = b.B.size(), nv = b.voff.size();
            std::vector<unsigned char> stage((nB + nv) * wb);
            for (size_t k = 0; k < nB; ++k) x_put(&stage[k * wb], b.B[k], bits);
            for (size_t k = 0; k < nv; ++k) x_put(&stage[(nB + k) * wb], b.voff[k], bits);
            void *dB = nullptr, *dv = nullptr;
            HIP_TRY(hipSetDevice(b.device));
            if (hipMalloc(&dB, nB * wb) != hipSuccess || hipMalloc(&dv, nv * wb) != hipSuccess) {
                (void)hipFree(dB); (void)hipFree(dv);
                return fail(MI_NO_MEMORY, "device allocation failed");
            }
            if (hipMemcpy(dB, stage.data(), nB * wb, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(dv, &stage[nB * wb], nv * wb, hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipFree(dB); (void)hipFree(dv);
                return fail(MI_HIP_ERROR, "upload of the base problem failed");
            }
            im.B = dB; im.voff = dv;
        }
        im.tried = true;                                                    // (it fits or it does not: settled)
    }
    if (!im.B) return kXOverflow;
    *out = XbbBaseView{im.B, im.voff, b.rows, b.cols, b.ncv, b.nb, b.d_basis, b.d_kind, b.d_vcol, b.Db};
    return MI_OK;
}

// does the node row end up artificial?  (the sign test of k_xbb_assemble: bound - offset < 0 flips the sense)
bool xbb_row_artificial(const XbbBase &b, int64_t var, int sense, int64_t bound)
{
    bool neg = bound < 0;
    if (b.kind[var] != 2) neg = (i128_t)bound * b.off_den[var] < (i128_t)b.off_num[var];
    return row_word_artificial(row_word(neg, sense));
}

XbbNodeRows xbb_rows(const XbbNodes &nd) { return XbbNodeRows{nd.var, nd.sense, nd.bound, nd.d}; }

// members [q0, q0 + count) of a group at `bits` into mt and / or art (NULL: left out), control blocks with D = Db
// first; afterwards h[q].status is kXbIdle or kXOverflow.  MI_OK, kXOverflow (the base does not fit), or an error.
int xbb_assemble(mi355x_xbatch *mt, mi355x_xbatch *art, int bits, int64_t q0, int64_t count, hipStream_t s)
{
    mi355x_xbatch *any = mt ? mt : art;
    XbbBaseView bv;
    const int irc = xbb_image(*any->nodes->base, bits, &bv);
    if (irc != MI_OK) return irc;
    const int wi = xb_wi(bits);
    XbView views[2] = {XbView{}, XbView{}};
    mi355x_xbatch *hs[2] = {mt, art};
    for (int k = 0; k < 2; ++k) {
        if (!hs[k]) continue;
        const int rc = xb_alloc(hs[k], wi);
        if (rc != MI_OK) return rc;
        XbWidth &w = hs[k]->w[wi];
        for (int64_t q = q0; q < q0 + count; ++q) w.h[q] = xb_fresh(bv.Db);
        HIP_TRY(hipMemcpyAsync(w.v.ctl + q0, &w.h[q0], count * sizeof(XbCtl), hipMemcpyHostToDevice, s));
        views[k] = w.v;
    }
    launch_xbb_assemble(views[0], views[1], bv, xbb_rows(*any->nodes), q0, count, s);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < 2; ++k)
        if (hs[k]) {
            XbWidth &w = hs[k]->w[wi];
            HIP_TRY(hipMemcpyAsync(&w.h[q0], w.v.ctl + q0, count * sizeof(XbCtl), hipMemcpyDeviceToHost, s));
        }
    HIP_TRY(hipStreamSynchronize(s));
    return MI_OK;
}

int xbb_reassemble_128(mi355x_xbatch *b, int64_t q, hipStream_t s, __int128 *D0)
{
    const bool is_art = b->nodes->art == b;
    const int rc = xbb_assemble(is_art ? nullptr : b, is_art ? b : nullptr, 128, q, 1, s);
    if (rc != MI_OK) return rc;
    if (b->w[1].h[q].status == kXOverflow) return kXOverflow;
    *D0 = b->nodes->base->Db;
    return MI_OK;
}

// an empty batch of n members whose start states come from `nodes`
mi355x_xbatch *xbb_new_batch(const std::shared_ptr<XbbNodes> &nodes, int64_t n, int64_t rows, int64_t cols, bool start_ok)
{
    mi355x_xbatch *b = new (std::nothrow) mi355x_xbatch;
    if (!b) return nullptr;
    const XbbBase &base = *nodes->base;
    b->device = base.device;
    b->n = n; b->rows = rows; b->cols = cols;
    b->nodes = nodes;
    b->start_ok.assign((size_t)n, start_ok ? 1 : 0);
    b->width.assign((size_t)n, 0);
    // cl_j and L_c of the base's objective row with the d node slacks (objective entry 0) inserted: the same for
    // every member.  (Only the main batch of a two-phase group is ever read for them.)
    b->mult.assign((size_t)(n * (cols + 1)), 0);
    if (base.lc != 0 && cols == base.cols + nodes->d) {
        const int64_t at = base.ncv + base.nb, d = nodes->d;
        for (int64_t q = 0; q < n; ++q) {
            i128_t *mq = &b->mult[q * (cols + 1)];
            for (int64_t j = 0; j < base.cols; ++j) mq[j < at ? j : j + d] = base.cl[j];
            mq[cols] = base.lc;
        }
    }
    if (hipSetDevice(b->device) != hipSuccess || hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
        mi355x_xbatch_destroy(b);
        return nullptr;
    }
    return b;
}

}  // namespace

int mi355x_xbb_base_create(mi355x_xbb_base **out, int64_t rows, int64_t cols, const int64_t *num, const int64_t *den,
                           const int64_t *basis, int64_t ncv, int64_t nb, int64_t n_vars, const int32_t *kind,
                           const int64_t *col, const int64_t *off_num, const int64_t *off_den, int device)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (rows < 1 || cols < 1 || !num || !den || (rows > 1 && !basis) || n_vars < 1 || !kind || !col || !off_num || !off_den)
        return fail(MI_BAD_ARG, "bad shape or NULL array");
    if (rows > (1 << 24) || cols > (1 << 24) || n_vars > cols) return fail(MI_BAD_ARG, "shape out of range");
    if (ncv < n_vars || nb < 0 || nb > rows - 1 || ncv + nb > cols - 1) return fail(MI_BAD_ARG, "bad column or row counts");
    for (int64_t k = 0; k < rows * cols; ++k)
        if (den[k] <= 0) return fail(MI_BAD_ARG, "denominator %lld of entry %lld is not positive", (long long)den[k], (long long)k);
    for (int64_t v = 0; v < n_vars; ++v) {
        if (kind[v] < 0 || kind[v] > 2 || col[v] < 0 || col[v] + (kind[v] == 2 ? 1 : 0) >= ncv)
            return fail(MI_BAD_ARG, "bad mapping of variable %lld", (long long)v);
        if (off_den[v] <= 0) return fail(MI_BAD_ARG, "offset denominator of variable %lld is not positive", (long long)v);
    }
    for (int64_t i = 0; i < rows - 1; ++i)
        if (basis[i] < 0 || basis[i] > cols) return fail(MI_BAD_ARG, "basis entry %lld out of range", (long long)i);
    int rc = x_check_device(device);
    if (rc != MI_OK) return rc;
    std::shared_ptr<XbbBase> b = std::make_shared<XbbBase>();
    b->device = device;
    b->rows = rows; b->cols = cols; b->ncv = ncv; b->nb = nb; b->n_vars = n_vars;
    b->basis.assign(basis, basis + (rows - 1));
    b->kind.assign(kind, kind + n_vars);
    b->vcol.assign(col, col + n_vars);
    b->off_num.assign(off_num, off_num + n_vars);
    b->off_den.assign(off_den, off_den + n_vars);
    const int64_t m = rows - 1;
    b->start_ok = true;
    for (int64_t i = 0; i < m; ++i) {
        const int64_t bc = basis[i];
        if (bc == cols) { b->n_art += 1; continue; }
        for (int64_t r = 0; r <= m && b->start_ok; ++r)
            b->start_ok = bc < cols - 1 && num[r * cols + bc] == (r == i ? den[r * cols + bc] : 0);
    }
    i128_t D0 = 0, loff = 1;
    bool ok = x_start_state(rows, cols, num, den, 128, b->B, &D0) == MI_OK;
    for (int64_t v = 0; v < n_vars && ok; ++v) ok = x_lcm(loff, off_den[v], &loff);
    ok = ok && x_mul(D0, loff, &b->Db) && x_fits(b->Db, 128);
    for (size_t k = 0; k < b->B.size() && ok; ++k) ok = x_mul(b->B[k], loff, &b->B[k]) && x_fits(b->B[k], 128);
    b->voff.assign((size_t)n_vars, 0);
    for (int64_t v = 0; v < n_vars && ok; ++v) ok = x_mul(b->Db / off_den[v], off_num[v], &b->voff[v]) && x_fits(b->voff[v], 128);
    if (!ok) return fail(MI_EXACT_OVERFLOW, "the base problem at integer scale needs more than 128 bits");
    if (x_objective_multipliers(cols, num + m * cols, den + m * cols, &b->lc, b->cl)) {
        // (an overflow leaves L_c = 0: the hand-over of every member then reports it)
    } else {
        b->lc = 0;
    }
    HIP_TRY(hipSetDevice(device));
    if (hipMalloc((void **)&b->d_basis, std::max<int64_t>(m, 1) * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void **)&b->d_vcol, n_vars * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void **)&b->d_kind, n_vars * sizeof(int32_t)) != hipSuccess)
        return fail(MI_NO_MEMORY, "device allocation failed");
    if (m > 0) HIP_TRY(hipMemcpy(b->d_basis, basis, m * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_vcol, col, n_vars * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_kind, kind, n_vars * sizeof(int32_t), hipMemcpyHostToDevice));
    XbbBaseView bv;
    rc = xbb_image(*b, 64, &bv);                                            // (kept where it fits; 128 at first need)
    if (rc != MI_OK && rc != kXOverflow) return rc;
    mi355x_xbb_base *h = new (std::nothrow) mi355x_xbb_base;
    if (!h) return fail(MI_NO_MEMORY, "host allocation failed");
    h->p = std::move(b);
    *out = h;
    return MI_OK;
}

void mi355x_xbb_base_destroy(mi355x_xbb_base *base) { delete base; }

int mi355x_xbatch_create_nodes(mi355x_xbatch **out_main, mi355x_xbatch **out_art, const mi355x_xbb_base *base,
                               int64_t n_nodes, int64_t depth, const int64_t *var, const int32_t *sense,
                               const int64_t *bound, int min_bits)
{
    if (!out_main || !out_art) return fail(MI_BAD_ARG, "out is NULL");
    *out_main = *out_art = nullptr;
    if (!base || n_nodes < 1 || depth < 1 || !var || !sense || !bound) return fail(MI_BAD_ARG, "bad counts or NULL array");
    if (min_bits != 0 && min_bits != 64 && min_bits != 128) return fail(MI_BAD_ARG, "min_bits must be 0, 64 or 128");
    if (n_nodes > (1 << 24) || depth > (1 << 24)) return fail(MI_BAD_ARG, "shape out of range");
    const XbbBase &b = *base->p;
    int64_t n_art = -1;
    for (int64_t q = 0; q < n_nodes; ++q) {
        int64_t a = b.n_art;
        for (int64_t k = q * depth; k < (q + 1) * depth; ++k) {
            if (var[k] < 0 || var[k] >= b.n_vars || sense[k] < 0 || sense[k] > 1 || bound[k] == INT64_MIN)
                return fail(MI_BAD_ARG, "bad node row %lld", (long long)k);
            a += xbb_row_artificial(b, var[k], sense[k], bound[k]);
        }
        if (n_art >= 0 && a != n_art) return fail(MI_BAD_ARG, "the nodes have different numbers of artificial rows");
        n_art = a;
    }
    int rc = x_check_device(b.device);
    if (rc != MI_OK) return rc;
    const int64_t rows = b.rows + depth, cols = b.cols + depth, nac = cols + n_art;
    if ((size_t)(rows + (n_art ? nac : cols)) * 16 > kXbSnapshotLimit)
        return fail(MI_UNSUPPORTED, "a %lld x %lld member's snapshots do not fit a workgroup's LDS", (long long)rows,
                    (long long)(n_art ? nac : cols));
    std::shared_ptr<XbbNodes> nodes = std::make_shared<XbbNodes>();
    nodes->base = base->p;
    nodes->d = depth;
    const size_t nk = (size_t)(n_nodes * depth);
    HIP_TRY(hipSetDevice(b.device));
    if (hipMalloc((void **)&nodes->var, nk * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void **)&nodes->bound, nk * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void **)&nodes->sense, nk * sizeof(int32_t)) != hipSuccess)
        return fail(MI_NO_MEMORY, "device allocation failed");
    HIP_TRY(hipMemcpy(nodes->var, var, nk * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(nodes->bound, bound, nk * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(nodes->sense, sense, nk * sizeof(int32_t), hipMemcpyHostToDevice));
    // the main batch: runnable on its own only without artificial rows (its basis names no column for them)
    mi355x_xbatch *mt = xbb_new_batch(nodes, n_nodes, rows, cols, b.start_ok && n_art == 0);
    mi355x_xbatch *art = n_art ? xbb_new_batch(nodes, n_nodes, rows, nac, b.start_ok) : nullptr;
    auto undo = [&](int code) { mi355x_xbatch_destroy(mt); mi355x_xbatch_destroy(art); return code; };
    if (!mt || (n_art && !art)) return undo(fail(MI_NO_MEMORY, "batch creation failed"));
    nodes->art = art;
    hipStream_t s = mt->stream;
    for (int bits = min_bits == 128 ? 128 : 64; bits <= 128; bits += 64) {
        // one launch for the whole group at its first width; at 128 bits after 64 only the members that need it
        const int wi = xb_wi(bits);
        for (int64_t q = 0; q < n_nodes; ++q) {
            if (mt->width[q] != 0) continue;
            int64_t cnt = 1;
            while (q + cnt < n_nodes && mt->width[q + cnt] == 0) ++cnt;
            rc = xbb_assemble(mt, art, bits, q, cnt, s);
            if (rc == kXOverflow) break;                                    // (the base itself does not fit this width)
            if (rc != MI_OK) return undo(rc);
            for (int64_t k = q; k < q + cnt; ++k) {
                const bool ovf = mt->w[wi].h[k].status == kXOverflow || (art && art->w[wi].h[k].status == kXOverflow);
                if (ovf) {
                    mt->w[wi].h[k] = xb_fresh(0);
                    if (art) art->w[wi].h[k] = xb_fresh(0);
                } else {
                    mt->width[k] = bits;
                    if (art) art->width[k] = bits;
                }
            }
            q += cnt - 1;
        }
        if (mt->w[wi].v.T && (xb_write_ctl(mt, s) != MI_OK || (art && xb_write_ctl(art, s) != MI_OK) ||
                              hipStreamSynchronize(s) != hipSuccess))
            return undo(fail(MI_HIP_ERROR, "upload of the control blocks failed"));
    }
    *out_main = mt;
    *out_art = art;
    return MI_OK;
}

int mi355x_xbatch_readback(mi355x_xbatch *b, int64_t *values_lo_hi, int64_t *basis, int32_t *status)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (!values_lo_hi) return fail(MI_BAD_ARG, "values_lo_hi is NULL");
    int rc = use_device_id(b->device);
    if (rc != MI_OK) return rc;
    const size_t n = (size_t)b->n, m = (size_t)b->rows - 1, per = 2 * (size_t)(1 + b->rows + b->cols);
    if (!b->rb_width) {                                                     // (both buffers or neither)
        if (!b->rb) HIP_TRY(hipMalloc((void **)&b->rb, n * (per + m) * sizeof(int64_t)));
        HIP_TRY(hipMalloc((void **)&b->rb_width, n * sizeof(int32_t)));
    }
    static_assert(sizeof(int) == sizeof(int32_t), "the widths go to the device as they are");
    HIP_TRY(hipMemcpyAsync(b->rb_width, b->width.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
    for (int wi = 0; wi < 2; ++wi)
        if (b->w[wi].v.T) launch_xbb_readback(b->w[wi].v, b->rb_width, b->rb, b->rb + n * per, b->stream);
    HIP_TRY(hipGetLastError());
    std::vector<int64_t> host(n * (per + m));
    HIP_TRY(hipMemcpyAsync(host.data(), b->rb, host.size() * sizeof(int64_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (size_t q = 0; q < n; ++q) {
        const bool lost = b->width[q] == 0;                                 // (its slots hold nothing of use)
        if (status) status[q] = lost ? MI_EXACT_OVERFLOW : MI_OK;
        if (lost) std::fill(values_lo_hi + q * per, values_lo_hi + (q + 1) * per, 0);
        else      std::copy(&host[q * per], &host[(q + 1) * per], values_lo_hi + q * per);
        if (basis && m > 0) {
            if (lost) std::fill(basis + q * m, basis + (q + 1) * m, 0);
            else      std::copy(&host[n * per + q * m], &host[n * per + (q + 1) * m], basis + q * m);
        }
    }
    return MI_OK;
}
