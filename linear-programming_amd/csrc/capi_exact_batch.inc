// capi_exact_batch.inc -- mi355x_xbatch_*: many exact rational LPs of one shape side by side, one
// workgroup per member (kernels_exact_batch.inc).  Part of simplex_capi.hip (ONE translation unit:
// included there after capi_exact.inc, whose host helpers -- x_start_state, x_start_ok,
// x_objective_multipliers, x_put, x_download_lo_hi, x_exact_status -- it shares).
//
// A handle keeps the callers' rationals of every member on the host and up to two sub-batches on the
// device, one per width.  Every member has a slot in each: it runs in the slot of its current width,
// the other one stays idle.  A member that overflows 64 bits is loaded again from its own start state
// into its 128-bit slot and replays, with the other restarted members, up to the same cumulative pivot
// count.  The host reads the control blocks once per round of launches; nothing between the phases
// comes back to the host per member.
//
// A member's start state has one of two sources: the caller's rationals (mi355x_xbatch_create), or a node
// spec -- a base problem and the member's node rows -- from which k_xbb_assemble writes it on the device
// (mi355x_xbatch_create_nodes, capi_exact_bb.inc).  A third source is the members' problem rows in column
// space, from which k_xb_assemble_lps writes it on the device (mi355x_xbatch_create_lps, capi_exact_lps.inc).
// Everything after the start is the same for all three.

struct XbbNodes;                         // capi_exact_bb.inc: the node spec of a handle made by create_nodes
struct XbLps;                            // capi_exact_lps.inc: the problem rows of a handle made by create_lps

struct XbWidth {
    XbView             v{};              // v.T == nullptr: this width is not allocated
    void              *aux = nullptr;    // per member: cl_j (cols values), then L_c; L_c = 0: they do not fit the width
    std::vector<XbCtl> h;                // host mirror of v.ctl, current whenever no call is running
};

struct mi355x_xbatch {
    int         device = 0;
    hipStream_t stream = nullptr;
    int64_t     n = 0, rows = 0, cols = 0;
    std::vector<int64_t> num, den, basis0;      // the callers' tableaux, member after member (none: see nodes)
    std::shared_ptr<XbbNodes> nodes;            // the other source of the start states: the members' node rows
    std::shared_ptr<XbLps> lps;                 // or the third: the members' problem rows, resident on the device
    int64_t    *rb = nullptr;                   // mi355x_xbatch_readback's device buffer, made at its first call
    int32_t    *rb_width = nullptr;
    std::vector<char>    start_ok;              // per member: unit basis columns over a zero objective entry
    std::vector<int>     width;                 // per member: 64, 128, or 0 once it needs more than 128 bits
    std::vector<i128_t>  mult;                  // per member: cl_j (cols values), then L_c (0: overflowed 128 bits)
    XbWidth     w[2];                           // the 64-bit and the 128-bit sub-batch
    int         rule = MI_RULE_DANTZIG;         // mi355x_xbatch_set_pivot_rule; each width's v.rule carries it to k_xb_solve
    bool        derived = false;                // the main batch of a two-phase job
    mi355x_xbatch *tp_main = nullptr;           // on the artificial batch: its main batch
    std::atomic<int> cancel{0};
};

namespace {

constexpr int64_t kXbTraceCap = MI355X_XBATCH_TRACE_CAP;
static_assert(MI355X_XBATCH_WORKGROUP == kXThreads, "the header states k_xb_solve's workgroup size");

// member q of a handle made from node specs assembled again at 128 bits (capi_exact_bb.inc): MI_OK and its
// D, kXOverflow, or an error
int xbb_reassemble_128(mi355x_xbatch *b, int64_t q, hipStream_t s, __int128 *D0);
// the same for a handle made from problem rows (capi_exact_lps.inc)
int xlp_reassemble_128(mi355x_xbatch *b, int64_t q, hipStream_t s, __int128 *D0);

int xb_wi(int bits) { return bits == 128 ? 1 : 0; }
XbCtl &xb_ctl(mi355x_xbatch *b, int64_t q) { return b->w[xb_wi(b->width[q])].h[q]; }
bool xb_live(const mi355x_xbatch *b, int64_t q) { return b->start_ok[q] && b->width[q] != 0; }

// pivots per member and launch: a launch stays short at every shape (a cancel is honoured between two)
int64_t xb_launch_cap(const mi355x_xbatch *b)
{
    return std::max<int64_t>(8, std::min<int64_t>(4096, ((int64_t)1 << 22) / (b->rows * b->cols)));
}

// member q's start state at `bits` into dst (rows * cols values of the width): MI_OK or kXOverflow
int xb_stage_member(const mi355x_xbatch *b, int64_t q, int bits, unsigned char *dst, i128_t *D0)
{
    const int64_t RC = b->rows * b->cols;
    std::vector<i128_t> T0;
    if (x_start_state(b->rows, b->cols, &b->num[q * RC], &b->den[q * RC], bits, T0, D0) != MI_OK) return kXOverflow;
    for (int64_t k = 0; k < RC; ++k) x_put(dst + k * (bits / 8), T0[k], bits);
    return MI_OK;
}

XbCtl xb_fresh(i128_t D0)
{
    XbCtl c{};
    c.status = kXbIdle;
    c.D = D0;
    return c;
}

void xb_free(mi355x_xbatch *b, int wi)
{
    XbWidth &s = b->w[wi];
    (void)hipFree(s.v.T); (void)hipFree(s.v.basis); (void)hipFree(s.v.ctl);
    (void)hipFree(s.v.trace_ec); (void)hipFree(s.v.trace_cr); (void)hipFree(s.aux);
    s.v = XbView{};
    s.aux = nullptr;
}

// the sub-batch of one width: buffers for every member, the start bases, the hand-over multipliers,
// every control block idle
int xb_alloc(mi355x_xbatch *b, int wi)
{
    XbWidth &s = b->w[wi];
    if (s.v.T) return MI_OK;
    const int bits = wi ? 128 : 64;
    const size_t wb = bits / 8, n = (size_t)b->n, R = (size_t)b->rows, C = (size_t)b->cols, m = R - 1;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMalloc(&s.v.T, n * R * C * wb));
    HIP_TRY(hipMalloc((void **)&s.v.basis, std::max<size_t>(n * m, 1) * sizeof(int64_t)));
    HIP_TRY(hipMalloc((void **)&s.v.ctl, n * sizeof(XbCtl)));
    HIP_TRY(hipMalloc((void **)&s.v.trace_ec, n * kXbTraceCap * sizeof(int64_t)));
    HIP_TRY(hipMalloc((void **)&s.v.trace_cr, n * kXbTraceCap * sizeof(int64_t)));
    HIP_TRY(hipMalloc(&s.aux, n * (C + 1) * wb));
    s.v.aux = s.aux;
    s.v.n = b->n; s.v.rows = b->rows; s.v.cols = b->cols; s.v.trace_cap = kXbTraceCap; s.v.bits = bits;
    s.v.rule = b->rule;
    std::vector<unsigned char> stage(n * (C + 1) * wb, 0);
    for (size_t q = 0; q < n; ++q) {
        const i128_t *mq = &b->mult[q * (C + 1)];
        bool ok = mq[C] != 0;
        for (size_t j = 0; j <= C && ok; ++j) ok = x_fits(mq[j], bits);
        if (!ok) continue;                                                  // (L_c stays 0)
        for (size_t j = 0; j <= C; ++j) x_put(&stage[(q * (C + 1) + j) * wb], mq[j], bits);
    }
    HIP_TRY(hipMemcpyAsync(s.aux, stage.data(), stage.size(), hipMemcpyHostToDevice, b->stream));
    if (n * m > 0 && !b->nodes && !b->lps)                                  // (specs: the assembling kernel writes the bases)
        HIP_TRY(hipMemcpyAsync(s.v.basis, b->basis0.data(), n * m * sizeof(int64_t), hipMemcpyHostToDevice, b->stream));
    s.h.assign(n, xb_fresh(0));
    HIP_TRY(hipMemcpyAsync(s.v.ctl, s.h.data(), n * sizeof(XbCtl), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));                               // (`stage` may go)
    return MI_OK;
}

int xb_write_ctl(mi355x_xbatch *b, hipStream_t s)
{
    for (int wi = 0; wi < 2; ++wi)
        if (b->w[wi].v.T)
            HIP_TRY(hipMemcpyAsync(b->w[wi].v.ctl, b->w[wi].h.data(), b->n * sizeof(XbCtl), hipMemcpyHostToDevice, s));
    return MI_OK;
}
int xb_read_ctl(mi355x_xbatch *b, hipStream_t s)
{
    for (int wi = 0; wi < 2; ++wi)
        if (b->w[wi].v.T)
            HIP_TRY(hipMemcpyAsync(b->w[wi].h.data(), b->w[wi].v.ctl, b->n * sizeof(XbCtl), hipMemcpyDeviceToHost, s));
    return MI_OK;
}

// Member q again from its own start state at 128 bits, running up to cap_at (status: kRunning or
// kXbIdle): MI_OK, kXOverflow (it needs more than 128 bits: width 0 from now on), or an error.
int xb_restart_128(mi355x_xbatch *b, int64_t q, int32_t status, int64_t cap_at, hipStream_t s)
{
    int rc = xb_alloc(b, 1);
    if (rc != MI_OK) return rc;
    const size_t RC = (size_t)(b->rows * b->cols), m = (size_t)b->rows - 1;
    std::vector<unsigned char> stage;
    i128_t D0 = 0;
    XbWidth &w = b->w[1];
    if (b->nodes || b->lps) {
        rc = b->nodes ? xbb_reassemble_128(b, q, s, &D0) : xlp_reassemble_128(b, q, s, &D0);
        if (rc == kXOverflow) { b->width[q] = 0; return kXOverflow; }
        if (rc != MI_OK) return rc;
    } else {
        stage.resize(RC * 16);
        if (xb_stage_member(b, q, 128, stage.data(), &D0) != MI_OK) { b->width[q] = 0; return kXOverflow; }
        HIP_TRY(hipMemcpyAsync((unsigned char *)w.v.T + (size_t)q * RC * 16, stage.data(), stage.size(), hipMemcpyHostToDevice, s));
        if (m > 0)
            HIP_TRY(hipMemcpyAsync(w.v.basis + q * m, &b->basis0[q * m], m * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    w.h[q] = xb_fresh(D0);
    w.h[q].status = status;
    w.h[q].cap_at = cap_at;
    HIP_TRY(hipMemcpyAsync(w.v.ctl + q, &w.h[q], sizeof(XbCtl), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                                       // (`stage` may go)
    b->width[q] = 128;
    return MI_OK;
}

// the widths in which some member of b (single phase) or of the job (art, mt) still runs: only those are launched
void xb_active_widths(mi355x_xbatch *b, mi355x_xbatch *mt, bool active[2])
{
    active[0] = active[1] = false;
    for (int64_t q = 0; q < b->n; ++q) {
        if (!xb_live(b, q)) continue;
        const XbCtl &c = xb_ctl(b, q);
        if (c.status == kRunning || (mt && c.tp == 1 && xb_ctl(mt, q).status == kRunning)) active[xb_wi(b->width[q])] = true;
    }
}

int32_t xb_member_status(int32_t st)
{
    return st == kRunning ? MI_RUNNING : st;
}

}  // namespace

int mi355x_xbatch_create(mi355x_xbatch **out, int64_t n_lps, int64_t rows, int64_t cols, const int64_t *num,
                         const int64_t *den, const int64_t *basis, int device, int min_bits)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (n_lps < 1 || rows < 1 || cols < 1 || !num || !den || (rows > 1 && !basis))
        return fail(MI_BAD_ARG, "bad shape or NULL array");
    if (min_bits != 0 && min_bits != 64 && min_bits != 128) return fail(MI_BAD_ARG, "min_bits must be 0, 64 or 128");
    if (rows > (1 << 24) || cols > (1 << 24) || n_lps > (1 << 24)) return fail(MI_BAD_ARG, "shape out of range");
    const int64_t RC = rows * cols, m = rows - 1;
    for (int64_t k = 0; k < n_lps * RC; ++k)
        if (den[k] <= 0) return fail(MI_BAD_ARG, "denominator %lld of entry %lld is not positive", (long long)den[k], (long long)k);
    int rc = x_check_device(device);
    if (rc != MI_OK) return rc;
    if ((size_t)(rows + cols) * 16 > kXbSnapshotLimit)
        return fail(MI_UNSUPPORTED, "a %lld x %lld member's snapshots do not fit a workgroup's LDS", (long long)rows, (long long)cols);
    mi355x_xbatch *b = new (std::nothrow) mi355x_xbatch;
    if (!b) return fail(MI_NO_MEMORY, "host allocation failed");
    b->device = device;
    b->n = n_lps; b->rows = rows; b->cols = cols;
    b->num.assign(num, num + n_lps * RC);
    b->den.assign(den, den + n_lps * RC);
    if (m > 0) b->basis0.assign(basis, basis + n_lps * m);
    b->start_ok.assign((size_t)n_lps, 0);
    b->width.assign((size_t)n_lps, 0);
    b->mult.assign((size_t)(n_lps * (cols + 1)), 0);
    std::vector<unsigned char> stage[2];
    std::vector<i128_t> D0((size_t)n_lps, 0), cl;
    for (int64_t q = 0; q < n_lps; ++q) {
        b->start_ok[q] = x_start_ok(rows, cols, &b->num[q * RC], &b->den[q * RC], m > 0 ? &b->basis0[q * m] : nullptr);
        i128_t lc = 0;
        if (x_objective_multipliers(cols, &b->num[q * RC + m * cols], &b->den[q * RC + m * cols], &lc, cl)) {
            std::copy(cl.begin(), cl.end(), &b->mult[q * (cols + 1)]);
            b->mult[q * (cols + 1) + cols] = lc;
        }
        for (int bits = min_bits == 128 ? 128 : 64; bits <= 128 && b->width[q] == 0; bits += 64) {
            std::vector<unsigned char> &st = stage[xb_wi(bits)];
            if (st.empty()) st.assign((size_t)(n_lps * RC) * (bits / 8), 0);
            if (xb_stage_member(b, q, bits, &st[(size_t)(q * RC) * (bits / 8)], &D0[q]) == MI_OK) b->width[q] = bits;
        }
    }
    auto undo = [&](int code) { mi355x_xbatch_destroy(b); return code; };
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess)
        return undo(fail(MI_HIP_ERROR, "stream creation failed"));
    for (int wi = 0; wi < 2; ++wi) {
        bool any = false;
        for (int64_t q = 0; q < n_lps; ++q) any = any || b->width[q] == (wi ? 128 : 64);
        if (!any) continue;
        rc = xb_alloc(b, wi);
        if (rc != MI_OK) return undo(rc);
        XbWidth &w = b->w[wi];
        for (int64_t q = 0; q < n_lps; ++q)
            if (b->width[q] == (wi ? 128 : 64)) w.h[q] = xb_fresh(D0[q]);
        if (hipMemcpyAsync(w.v.T, stage[wi].data(), stage[wi].size(), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
            xb_write_ctl(b, b->stream) != MI_OK || hipStreamSynchronize(b->stream) != hipSuccess)
            return undo(fail(MI_HIP_ERROR, "upload of the start states failed"));
    }
    *out = b;
    return MI_OK;
}

int mi355x_xbatch_solve(mi355x_xbatch *b, int is_max, int64_t max_pivots, int32_t *status, int64_t *n_pivots)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    if (b->derived || b->tp_main) return fail(MI_BAD_ARG, "a batch of a two-phase job: use mi355x_xbatch_solve_two_phase");
    int rc = use_device_id(b->device);
    if (rc != MI_OK) return rc;
    const int64_t n = b->n, launch_cap = xb_launch_cap(b);
    std::vector<int64_t> k0((size_t)n, 0), cap((size_t)n, 0);
    for (int64_t q = 0; q < n; ++q) {
        if (!xb_live(b, q)) continue;
        XbCtl &c = xb_ctl(b, q);
        k0[q] = c.n_pivots;
        cap[q] = max_pivots > 0 ? c.n_pivots + max_pivots : 0;
        c.status = kRunning;
        c.cap_at = cap[q];
    }
    rc = xb_write_ctl(b, b->stream);
    if (rc != MI_OK) return rc;
    bool cancelled = false, active[2];
    for (;;) {
        xb_active_widths(b, nullptr, active);
        for (int wi = 0; wi < 2; ++wi)
            if (active[wi]) launch_xb_solve(b->w[wi].v, is_max, launch_cap, b->stream);
        HIP_TRY(hipGetLastError());
        rc = xb_read_ctl(b, b->stream);
        if (rc != MI_OK) return rc;
        HIP_TRY(hipStreamSynchronize(b->stream));
        bool running = false;
        for (int64_t q = 0; q < n; ++q) {
            if (!xb_live(b, q)) continue;
            const int32_t st = xb_ctl(b, q).status;
            if (st == kXInexact) return x_exact_status(kXInexact);
            if (st == kXOverflow) {
                // the member again from its start at 128 bits: the same pivots, up to the same count
                if (b->width[q] == 128) { b->width[q] = 0; continue; }
                rc = xb_restart_128(b, q, kRunning, cap[q], b->stream);
                if (rc == kXOverflow) continue;
                if (rc != MI_OK) return rc;
                running = true;
            } else if (st == kRunning) running = true;
        }
        // (a cancel that arrives while the last round finishes goes with the call: it never reaches the next one)
        const int c = b->cancel.exchange(0, std::memory_order_acq_rel);
        if (!running) break;
        if (c) { cancelled = true; break; }                                  // (whole pivots only)
    }
    for (int64_t q = 0; q < n; ++q) {
        const bool live = xb_live(b, q);
        if (status) status[q] = !b->start_ok[q] ? MI_UNSUPPORTED : !live ? MI_EXACT_OVERFLOW : xb_member_status(xb_ctl(b, q).status);
        if (n_pivots) n_pivots[q] = live ? std::max<int64_t>(0, xb_ctl(b, q).n_pivots - k0[q]) : 0;
    }
    return cancelled ? MI_CANCELLED : MI_OK;
}

int mi355x_xbatch_solve_two_phase(mi355x_xbatch *art, mi355x_xbatch *mt, int main_is_max, int64_t max_pivots,
                                  int32_t *status, int64_t *n_pivots)
{
    if (!art || !mt || art == mt) return fail(MI_BAD_ARG, "two distinct handles are needed");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    if (art->n != mt->n || art->rows != mt->rows || mt->cols > art->cols || art->device != mt->device)
        return fail(MI_BAD_ARG, "the batches do not belong to one list of problems");
    if (art->derived || mt->tp_main) return fail(MI_BAD_ARG, "handles used in another role");
    if (art->tp_main && art->tp_main != mt) return fail(MI_BAD_ARG, "the artificial batch belongs to another job");
    if (!art->tp_main && mt->derived) return fail(MI_BAD_ARG, "the main batch belongs to another job");
    int rc = use_device_id(art->device);
    if (rc != MI_OK) return rc;
    hipStream_t s = art->stream;
    const int64_t n = art->n, launch_cap = xb_launch_cap(art);
    if (!art->tp_main) {
        // one width per member for the job (both still at their start)
        for (int64_t q = 0; q < n; ++q) {
            if (art->width[q] == 0 || mt->width[q] == 0) { art->width[q] = mt->width[q] = 0; continue; }
            if (art->width[q] == 64 && mt->width[q] == 128) {
                rc = xb_restart_128(art, q, kXbIdle, 0, s);
                if (rc == kXOverflow) { mt->width[q] = 0; continue; }
                if (rc != MI_OK) return rc;
            }
            mt->width[q] = art->width[q];
        }
        art->tp_main = mt;
        mt->derived = true;
    }
    for (int wi = 0; wi < 2; ++wi)
        if (art->w[wi].v.T) {
            rc = xb_alloc(mt, wi);
            if (rc != MI_OK) return rc;
        }
    HIP_TRY(hipStreamSynchronize(mt->stream));
    // per member: the pivots of both phases and the drive-outs so far, and the call's target
    std::vector<int64_t> n1((size_t)n, 0), n2((size_t)n, 0), target((size_t)n, 0);
    for (int64_t q = 0; q < n; ++q) {
        if (!xb_live(art, q)) continue;
        XbCtl &ca = xb_ctl(art, q), &cm = xb_ctl(mt, q);
        n1[q] = ca.n_pivots + ca.driveouts;
        n2[q] = ca.tp == 1 ? cm.n_pivots : 0;
        target[q] = max_pivots > 0 ? n1[q] + n2[q] + max_pivots : 0;
        if (ca.tp == 0) {
            ca.status = kRunning;
            ca.cap_at = target[q];
            cm = xb_fresh(0);
        } else if (ca.tp == 1) {
            cm.status = kRunning;
            cm.cap_at = max_pivots > 0 ? n2[q] + max_pivots : 0;
        }
    }
    rc = xb_write_ctl(art, s);
    if (rc == MI_OK) rc = xb_write_ctl(mt, s);
    if (rc != MI_OK) return rc;
    bool cancelled = false, active[2];
    for (;;) {
        xb_active_widths(art, mt, active);
        for (int wi = 0; wi < 2; ++wi)
            if (active[wi]) {
                launch_xb_solve(art->w[wi].v, 0, launch_cap, s);
                launch_xb_between(art->w[wi].v, mt->w[wi].v, s);
                launch_xb_solve(mt->w[wi].v, main_is_max, launch_cap, s);
            }
        HIP_TRY(hipGetLastError());
        rc = xb_read_ctl(art, s);
        if (rc == MI_OK) rc = xb_read_ctl(mt, s);
        if (rc != MI_OK) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        bool running = false;
        for (int64_t q = 0; q < n; ++q) {
            if (!xb_live(art, q)) continue;
            const XbCtl &ca = xb_ctl(art, q), &cm = xb_ctl(mt, q);
            const int32_t sa = ca.status, sm = ca.tp == 1 ? cm.status : kXbIdle;
            if (sa == kXInexact || sm == kXInexact) return x_exact_status(kXInexact);
            if (sa == kXOverflow || sm == kXOverflow) {
                // both phases again from the start at 128 bits, up to the same pivot count
                if (art->width[q] == 128) { art->width[q] = mt->width[q] = 0; continue; }
                rc = xb_restart_128(art, q, kRunning, target[q], s);
                if (rc == kXOverflow) { mt->width[q] = 0; continue; }
                if (rc != MI_OK) return rc;
                rc = xb_alloc(mt, 1);
                if (rc != MI_OK) return rc;
                mt->width[q] = 128;
                mt->w[1].h[q] = xb_fresh(0);
                HIP_TRY(hipMemcpyAsync(mt->w[1].v.ctl + q, &mt->w[1].h[q], sizeof(XbCtl), hipMemcpyHostToDevice, s));
                HIP_TRY(hipStreamSynchronize(s));
                running = true;
            } else if (sa == kRunning || sm == kRunning) running = true;
        }
        int c = art->cancel.exchange(0, std::memory_order_acq_rel);         // (as in mi355x_xbatch_solve)
        c |= mt->cancel.exchange(0, std::memory_order_acq_rel);
        if (!running) break;
        if (c) { cancelled = true; break; }                                  // (whole pivots only)
    }
    for (int64_t q = 0; q < n; ++q) {
        const bool live = xb_live(art, q);
        if (status) status[q] = !art->start_ok[q] ? MI_UNSUPPORTED : MI_EXACT_OVERFLOW;
        if (n_pivots) n_pivots[2 * q] = n_pivots[2 * q + 1] = 0;
        if (!live) continue;
        const XbCtl &ca = xb_ctl(art, q), &cm = xb_ctl(mt, q);
        if (status) status[q] = ca.tp == 2 ? ca.tp_status : xb_member_status(ca.tp == 1 ? cm.status : ca.status);
        if (n_pivots) {
            n_pivots[2 * q] = std::max<int64_t>(0, ca.n_pivots + ca.driveouts - n1[q]);
            n_pivots[2 * q + 1] = ca.tp == 1 ? std::max<int64_t>(0, cm.n_pivots - n2[q]) : 0;
        }
    }
    return cancelled ? MI_CANCELLED : MI_OK;
}

int mi355x_xbatch_download(mi355x_xbatch *b, int64_t q, int64_t *num_lo_hi, int64_t *den_lo_hi, int64_t *basis)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (q < 0 || q >= b->n) return fail(MI_BAD_ARG, "member %lld out of range", (long long)q);
    if (b->width[q] == 0) return fail(MI_EXACT_OVERFLOW, "the member overflowed 128 bits");
    int rc = use_device_id(b->device);
    if (rc != MI_OK) return rc;
    const XbWidth &w = b->w[xb_wi(b->width[q])];
    const int64_t RC = b->rows * b->cols, m = b->rows - 1;
    rc = x_download_lo_hi(w.v.T, b->width[q], b->stream, q * RC, RC, w.h[q].D, num_lo_hi, den_lo_hi);
    if (rc != MI_OK) return rc;
    if (basis && m > 0) {
        HIP_TRY(hipMemcpyAsync(basis, w.v.basis + q * m, m * sizeof(int64_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    return MI_OK;
}

int mi355x_xbatch_trace(mi355x_xbatch *b, int64_t q, int64_t *ecs, int64_t *crs, int64_t cap, int64_t *n)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (q < 0 || q >= b->n) return fail(MI_BAD_ARG, "member %lld out of range", (long long)q);
    if (n) *n = 0;
    if (b->width[q] == 0) return MI_OK;
    int rc = use_device_id(b->device);
    if (rc != MI_OK) return rc;
    const XbWidth &w = b->w[xb_wi(b->width[q])];
    return download_trace(w.v.trace_ec + q * kXbTraceCap, w.v.trace_cr + q * kXbTraceCap, w.h[q].trace_n, kXbTraceCap,
                          b->stream, ecs, crs, cap, n);
}

int mi355x_xbatch_bits(const mi355x_xbatch *b, int64_t q, int *bits)
{
    if (!b || !bits) return fail(MI_BAD_ARG, "NULL argument");
    if (q < 0 || q >= b->n) return fail(MI_BAD_ARG, "member %lld out of range", (long long)q);
    *bits = b->width[q] ? b->width[q] : 128;
    return MI_OK;
}

int mi355x_xbatch_set_pivot_rule(mi355x_xbatch *b, int rule)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (rule != MI_RULE_DANTZIG && rule != MI_RULE_BLAND && rule != MI_RULE_DANTZIG_BLAND)
        return fail(MI_BAD_ARG, "unknown pivot rule %d", rule);
    // (a member at its start has no pivot, no drive-out and no stall flag, in either width's slot)
    for (int wi = 0; wi < 2; ++wi)
        for (const XbCtl &c : b->w[wi].h)
            if (c.n_pivots > 0 || c.driveouts > 0 || c.tp != 0)
                return fail(MI_BAD_ARG, "the pivot rule is set before the batch's first pivot");
    b->rule = rule;
    for (int wi = 0; wi < 2; ++wi) {
        if (b->w[wi].v.T) b->w[wi].v.rule = rule;
        for (XbCtl &c : b->w[wi].h) c.stall = 0;     // (the solve calls write the mirrors to the device first)
    }
    return MI_OK;
}

int mi355x_xbatch_cancel(mi355x_xbatch *b)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    b->cancel.store(1, std::memory_order_release);
    return MI_OK;
}

void mi355x_xbatch_destroy(mi355x_xbatch *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    xb_free(b, 0);
    xb_free(b, 1);
    (void)hipFree(b->rb);
    (void)hipFree(b->rb_width);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}
