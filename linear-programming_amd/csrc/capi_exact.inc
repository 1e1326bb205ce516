// capi_exact.inc -- mi355x_xtab_*: exact rational solves on fraction-free integer tableaux
// (kernels_exact.inc).  Part of simplex_capi.hip (ONE translation unit: included there, in this order).
//
// The handle keeps the caller's rationals on the host: a solve that overflows 64 bits starts again,
// both phases, from them at 128 bits, and one that overflows 128 bits at 256 where the handle allows it
// (mi355x_xtab_create_wide).  The host's own arithmetic is one copy on either value type: __int128 up to
// 128 bits, X256 (xwide.h, the type the kernels store) at 256.  What stays on the host: the start state (row LCMs, one pass
// over the input), the phase-1 feasibility test and the drive-out decisions (one element, the basis and
// the row of each artificial variable still basic: a sequential scan over a handful of rows, once per
// solve), and the hand-over's multipliers (the LCM of the objective row's denominators and c[b_i]).

struct mi355x_xtab {
    int         device = 0;
    hipStream_t stream = nullptr;
    int64_t     rows = 0, cols = 0;
    std::vector<int64_t> num, den, basis0;   // the caller's tableau, t0 = num / den
    bool        start_ok = false;            // basis columns exact unit columns, objective row zero on them
    int         bits = 0;                    // width of the device buffers (0: none yet)
    int         max_bits = 128;              // the widest the solves may escalate to: 128 or 256
    XView       v{};
    XCtl        h{};                         // host mirror of v.ctl, current whenever no call is running
    void       *aux = nullptr;               // hand-over multipliers: rows + cols values of the width
    bool        dead = false;                // overflowed max_bits: only destroy is left
    bool        derived = false;             // the main tableau of a two-phase job
    // two-phase job, kept on the artificial tableau
    mi355x_xtab *tp_main = nullptr;
    int         tp_phase = 0;                // 0 phase 1, 1 phase 2, 2 the hand-over ended the job (tp_status)
    int         tp_status = MI_OK;
    int64_t     tp_driveouts = 0;
    std::atomic<int> cancel{0};
};

namespace {

constexpr int64_t kXTraceCap = 1 << 18;

typedef unsigned __int128 u128_t;
typedef __int128 i128_t;
const i128_t INT128_MIN_ = (i128_t)((u128_t)1 << 127);

int use_device_id(int device)
{
    HIP_TRY(hipSetDevice(device));
    return MI_OK;
}

// ---- the value type V of a width: i128_t (64 and 128 bits) or X256 (256 bits) ---------------------------
// What crosses the boundary is int64_t, so a wide value is only ever multiplied by a wide value and divided
// or reduced by a 64-bit one.
bool x_mul(i128_t a, i128_t b, i128_t *r) { return !__builtin_mul_overflow(a, b, r); }
bool x_mul(const X256 &a, const X256 &b, X256 *r) { return xw_mul_ovf(a, b, r); }
i128_t x_div64(i128_t a, int64_t d) { return a / d; }
X256 x_div64(const X256 &a, int64_t d) { return xw_divmod_small(a, d, nullptr); }
int64_t x_mod64(i128_t a, int64_t d) { return (int64_t)(a % d); }
int64_t x_mod64(const X256 &a, int64_t d) { int64_t r = 0; (void)xw_divmod_small(a, d, &r); return r; }
bool x_sym(i128_t x) { return x != INT128_MIN_; }
bool x_sym(const X256 &x) { return !xw_is_min(x); }
bool x_zero(i128_t x) { return x == 0; }
bool x_zero(const X256 &x) { return x == 0; }
int64_t x_gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }
// lcm of positive values, false on overflow of V's symmetric range
template <class V> bool x_lcm(V a, int64_t b, V *r) { return x_mul(x_div64(a, x_gcd64(x_mod64(a, b), b)), (V)b, r) && x_sym(*r); }
bool x_lcm(const X256 &a, int64_t b, X256 *r) { return xw_lcm_small(a, b, r); }
bool x_fits(i128_t x, int bits)
{
    if (bits == 64) return x > (i128_t)INT64_MIN && x <= (i128_t)INT64_MAX;
    return x != INT128_MIN_;
}
bool x_fits(const X256 &x, int) { return x_sym(x); }                    // (X256 is the value type of 256 bits alone)

// a value of the device's width (64: the low half) at dst / src, and the ABI's low and high 64-bit limbs
void x_put(unsigned char *dst, i128_t x, int bits)
{
    if (bits == 64) { const int64_t y = (int64_t)x; memcpy(dst, &y, 8); }
    else            memcpy(dst, &x, 16);
}
void x_put(unsigned char *dst, const X256 &x, int) { memcpy(dst, x.l, 32); }
void x_get(const unsigned char *src, int bits, i128_t *out)
{
    int64_t y;
    if (bits == 64) { memcpy(&y, src, 8); *out = y; }
    else            memcpy(out, src, 16);
}
void x_get(const unsigned char *src, int, X256 *out) { memcpy(out->l, src, 32); }
void x_lo_hi(i128_t x, int64_t out[2])
{
    out[0] = (int64_t)(uint64_t)(u128_t)x;
    out[1] = (int64_t)(x >> 64);
}
// a value as `limbs` little-endian 64-bit limbs, sign-extended (limbs: 2 or 4 for i128_t, 4 for X256)
void x_limbs(i128_t x, int limbs, int64_t *out)
{
    x_lo_hi(x, out);
    for (int k = 2; k < limbs; ++k) out[k] = x < 0 ? -1 : 0;
}
void x_limbs(const X256 &x, int, int64_t *out) { memcpy(out, x.l, 32); }
// the common denominator in the control block's field of the width
void x_ctl_set_D(XCtl &h, i128_t D) { h.D = D; }
void x_ctl_set_D(XCtl &h, const X256 &D) { h.Dw = D; }
void x_ctl_get_D(const XCtl &h, i128_t *D) { *D = h.D; }
void x_ctl_get_D(const XCtl &h, X256 *D) { *D = h.Dw; }

int x_take_cancel(mi355x_xtab *a, mi355x_xtab *b = nullptr)
{
    int c = a->cancel.exchange(0, std::memory_order_acq_rel);
    if (b) c |= b->cancel.exchange(0, std::memory_order_acq_rel);
    return c;
}

int x_read_ctl(mi355x_xtab *t)
{
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&t->h, t->v.ctl, sizeof(XCtl), hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return MI_OK;
}
int x_write_ctl(mi355x_xtab *t)
{
    HIP_TRY(hipMemcpyAsync(t->v.ctl, &t->h, sizeof(XCtl), hipMemcpyHostToDevice, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return MI_OK;
}

void x_free_width(mi355x_xtab *t)
{
    (void)hipFree(t->v.T); (void)hipFree(t->v.col); (void)hipFree(t->v.prow); (void)hipFree(t->aux);
    t->v.T = t->v.col = t->v.prow = t->aux = nullptr;
}

// The start state at `bits`: D0 = prod L_i (the objective row's LCM folded into the first constraint
// row's), T0 = D0 * t0.  MI_OK, or kXOverflow when it does not fit the width.
template <class V> int x_start_state(int64_t R, int64_t C, const int64_t *num, const int64_t *den, int bits, std::vector<V> &T0,
                                     V *D0)
{
    const int64_t m = R - 1;
    std::vector<V> L(R, (V)1);
    for (int64_t i = 0; i < R; ++i)
        for (int64_t j = 0; j < C; ++j)
            if (!x_lcm(L[i], den[i * C + j], &L[i])) return kXOverflow;
    V D = 1;
    if (m > 0 && !x_mul(L[0], L[m], &L[0])) return kXOverflow;
    if (m == 0) D = L[0];
    for (int64_t i = 0; i < m; ++i)
        if (!x_mul(D, L[i], &D)) return kXOverflow;
    if (!x_fits(D, bits)) return kXOverflow;
    T0.assign((size_t)(R * C), (V)0);
    for (int64_t k = 0; k < R * C; ++k) {
        V x;
        if (!x_mul(x_div64(D, den[k]), (V)num[k], &x) || !x_fits(x, bits)) return kXOverflow;
        T0[k] = x;
    }
    *D0 = D;
    return MI_OK;
}

// the start the fraction-free state assumes: every basis column is an exact unit column, the
// objective row zero on it
bool x_start_ok(int64_t rows, int64_t cols, const int64_t *num, const int64_t *den, const int64_t *basis)
{
    const int64_t m = rows - 1;
    for (int64_t i = 0; i < m; ++i) {
        const int64_t b = basis[i];
        if (b < 0 || b >= cols - 1) return false;
        for (int64_t r = 0; r <= m; ++r)
            if (num[r * cols + b] != (r == i ? den[r * cols + b] : 0)) return false;
    }
    return true;
}

// multipliers of the hand-over's re-elimination from the main tableau's original objective row cn / cd
// (Cm entries): L_c (the LCM of its denominators) and cl_j = L_c * c_j; w_i of basic column b is cl[b].
// false on overflow of V.
template <class V> bool x_objective_multipliers(int64_t Cm, const int64_t *cn, const int64_t *cd, V *lc, std::vector<V> &cl)
{
    V l = 1;
    for (int64_t j = 0; j < Cm; ++j)
        if (!x_lcm(l, cd[j], &l)) return false;
    cl.assign((size_t)Cm, (V)0);
    for (int64_t j = 0; j < Cm; ++j)
        if (!x_mul(x_div64(l, cd[j]), (V)cn[j], &cl[j])) return false;
    *lc = l;
    return true;
}

// (re)load the start state at `bits`: device buffers of that width, T0, basis, a fresh control block
template <class V> int x_reset_v(mi355x_xtab *t, int bits)
{
    std::vector<V> T0;
    V D0 = 0;
    if (x_start_state(t->rows, t->cols, t->num.data(), t->den.data(), bits, T0, &D0) != MI_OK) return kXOverflow;
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipStreamSynchronize(t->stream));
    const size_t w = bits / 8, R = (size_t)t->rows, C = (size_t)t->cols;
    if (t->bits != bits) {
        x_free_width(t);
        HIP_TRY(hipMalloc(&t->v.T, R * C * w));
        HIP_TRY(hipMalloc(&t->v.col, R * w));
        HIP_TRY(hipMalloc(&t->v.prow, C * w));
        HIP_TRY(hipMalloc(&t->aux, (R + C) * w));
        t->bits = t->v.bits = bits;
    }
    std::vector<unsigned char> stage(R * C * w);
    for (size_t k = 0; k < R * C; ++k) x_put(&stage[k * w], T0[k], bits);
    HIP_TRY(hipMemcpyAsync(t->v.T, stage.data(), stage.size(), hipMemcpyHostToDevice, t->stream));
    if (R > 1) HIP_TRY(hipMemcpyAsync(t->v.basis, t->basis0.data(), (R - 1) * sizeof(int64_t), hipMemcpyHostToDevice, t->stream));
    t->h = XCtl{};
    t->h.status = MI_OPTIMAL;
    x_ctl_set_D(t->h, D0);
    return x_write_ctl(t);                    // (synchronises: `stage` may go)
}
int x_reset(mi355x_xtab *t, int bits) { return bits == 256 ? x_reset_v<X256>(t, bits) : x_reset_v<i128_t>(t, bits); }
// the start state at the first width above `from` that holds it, up to the handle's limit: MI_OK, kXOverflow
// (none does), or an error
int x_reset_wider(mi355x_xtab *t, int from)
{
    for (int bits = from * 2; bits <= t->max_bits; bits *= 2) {
        const int rc = x_reset(t, bits);
        if (rc != kXOverflow) return rc;
    }
    return kXOverflow;
}
// both tableaux of a two-phase job at one such width
int x_reset_wider(mi355x_xtab *a, mi355x_xtab *mt, int from)
{
    for (int bits = from * 2; bits <= a->max_bits; bits *= 2) {
        int rc = x_reset(a, bits);
        if (rc == MI_OK) rc = x_reset(mt, bits);
        if (rc != kXOverflow) return rc;
    }
    return kXOverflow;
}

// one solve of the handle's tableau, blind enqueue of (select, update) pairs in growing chunks with one
// control-block read per chunk: the status, MI_CANCELLED, kXOverflow or kXInexact
int x_run(mi355x_xtab *t, int is_max, int64_t cap_at, mi355x_xtab *peer)
{
    t->h.status = kRunning;
    t->h.err = 0;
    t->h.apply = 0;
    t->h.cap_at = cap_at;
    int rc = x_write_ctl(t);
    if (rc != MI_OK) return rc;
    for (int64_t chunk = 8;; chunk = std::min<int64_t>(chunk * 2, 512)) {
        for (int64_t k = 0; k < chunk; ++k) {
            launch_x_select(t->v, is_max, t->stream);
            launch_x_update(t->v, t->stream);
        }
        rc = x_read_ctl(t);
        if (rc != MI_OK) return rc;
        if (t->h.err) return t->h.err;
        if (t->h.status != kRunning) return t->h.status;
        if (x_take_cancel(t, peer)) return MI_CANCELLED;    // (the chunk ended on an update: whole pivots)
    }
}

// n values of the width from k0 on of the device array T (stream s, synchronised)
template <class V> int x_download_values(const void *T, int bits, hipStream_t s, int64_t k0, int64_t n, std::vector<V> &out)
{
    const size_t w = bits / 8;
    std::vector<unsigned char> buf((size_t)n * w);
    if (n > 0)
        HIP_TRY(hipMemcpyAsync(buf.data(), (const unsigned char *)T + (size_t)k0 * w, buf.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out.resize((size_t)n);
    for (int64_t k = 0; k < n; ++k) x_get(&buf[k * w], bits, &out[k]);
    return MI_OK;
}

// what both download entry points return: the entries (n of them) and D as limb pairs
int x_download_lo_hi(const void *T, int bits, hipStream_t s, int64_t k0, int64_t n, i128_t D, int64_t *num_lo_hi, int64_t *den_lo_hi)
{
    if (num_lo_hi) {
        std::vector<i128_t> vals;
        const int rc = x_download_values(T, bits, s, k0, n, vals);
        if (rc != MI_OK) return rc;
        for (int64_t k = 0; k < n; ++k) x_lo_hi(vals[k], num_lo_hi + 2 * k);
    }
    if (den_lo_hi) x_lo_hi(D, den_lo_hi);
    return MI_OK;
}
// the same as `limbs` limbs per value, from a tableau of value type V
template <class V> int x_download_limbs(mi355x_xtab *t, int limbs, int64_t *num_limbs, int64_t *den_limbs)
{
    if (num_limbs) {
        std::vector<V> vals;
        const int rc = x_download_values(t->v.T, t->bits, t->stream, 0, t->rows * t->cols, vals);
        if (rc != MI_OK) return rc;
        for (size_t k = 0; k < vals.size(); ++k) x_limbs(vals[k], limbs, num_limbs + (size_t)limbs * k);
    }
    if (den_limbs) {
        V D;
        x_ctl_get_D(t->h, &D);
        x_limbs(D, limbs, den_limbs);
    }
    return MI_OK;
}

// between the phases (src/simplex.lisp:405-451): MI_OK (main ready for phase 2), MI_INFEASIBLE,
// MI_ART_NONZERO, MI_ART_STUCK, kXOverflow, kXInexact, or an error
template <class V> int x_handover_v(mi355x_xtab *a, mi355x_xtab *mt)
{
    const int64_t m = a->rows - 1, C = a->cols, nav = C - 1, nv = mt->cols - 1;
    std::vector<V> row;
    int rc = x_download_values(a->v.T, a->bits, a->stream, m * C + nav, 1, row);    // the artificial objective value
    if (rc != MI_OK) return rc;
    if (!x_zero(row[0])) return MI_INFEASIBLE;
    std::vector<int64_t> basis((size_t)m);
    if (m > 0) HIP_TRY(hipMemcpy(basis.data(), a->v.basis, m * sizeof(int64_t), hipMemcpyDeviceToHost));
    rc = tp_drive_out<V>(
        m, nv, nav, basis.data(), [](const V &x) { return x_zero(x); },
        [&](int64_t i, std::vector<V> &r) { return x_download_values(a->v.T, a->bits, a->stream, i * C, C, r); },
        [&](int64_t col, int64_t i) {
            launch_x_force(a->v, col, i, a->stream);
            launch_x_update(a->v, a->stream);
            const int rc2 = x_read_ctl(a);
            return rc2 != MI_OK ? rc2 : (int)a->h.err;
        },
        [&] { a->tp_driveouts += 1; });
    if (rc != MI_OK) return rc;
    // multipliers of the re-elimination: L_c (LCM of the original objective row's denominators),
    // w_i = L_c * c[b_i], cl_j = L_c * c_j
    const int64_t Cm = mt->cols;
    V lc = 1;
    std::vector<V> cl;
    if (!x_objective_multipliers(Cm, &mt->num[m * Cm], &mt->den[m * Cm], &lc, cl)) return kXOverflow;
    std::vector<V> mult((size_t)(m + Cm));
    for (int64_t i = 0; i < m; ++i) mult[i] = cl[basis[i]];
    for (int64_t j = 0; j < Cm; ++j) mult[m + j] = cl[j];
    if (!x_fits(lc, mt->bits)) return kXOverflow;
    for (const V &x : mult)
        if (!x_fits(x, mt->bits)) return kXOverflow;
    const size_t w = mt->bits / 8;
    std::vector<unsigned char> stage(mult.size() * w);
    for (size_t k = 0; k < mult.size(); ++k) x_put(&stage[k * w], mult[k], mt->bits);
    HIP_TRY(hipMemcpyAsync(mt->aux, stage.data(), stage.size(), hipMemcpyHostToDevice, mt->stream));
    if (m > 0) HIP_TRY(hipMemcpyAsync(mt->v.basis, basis.data(), m * sizeof(int64_t), hipMemcpyHostToDevice, mt->stream));
    mt->h = XCtl{};
    mt->h.status = MI_OPTIMAL;
    rc = x_write_ctl(mt);                      // (synchronises: `stage` may go)
    if (rc != MI_OK) return rc;
    unsigned char lcw[sizeof(X256)];
    x_put(lcw, lc, mt->bits);
    launch_x_handover(a->v, mt->v, mt->aux, (const unsigned char *)mt->aux + m * w, lcw, mt->stream);
    rc = x_read_ctl(mt);
    if (rc != MI_OK) return rc;
    return mt->h.err ? mt->h.err : MI_OK;
}
int x_handover(mi355x_xtab *a, mi355x_xtab *mt) { return a->bits == 256 ? x_handover_v<X256>(a, mt) : x_handover_v<i128_t>(a, mt); }

// the two-phase job from where it stands up to `target` pivots of both phases together (0: no cap)
int x_two_phase(mi355x_xtab *a, mi355x_xtab *mt, int is_max, int64_t target)
{
    if (a->tp_phase == 2) return a->tp_status;
    if (a->tp_phase == 0) {
        const int st = x_run(a, 0, target, mt);
        if (st != MI_OPTIMAL) return st;
        const int rc = x_handover(a, mt);
        if (rc == kXOverflow || rc == kXInexact || rc < 0) return rc;
        if (rc != MI_OK) { a->tp_phase = 2; a->tp_status = rc; return rc; }
        a->tp_phase = 1;
    }
    const int64_t n1 = a->h.n_pivots + a->tp_driveouts;
    if (target > 0 && target - n1 <= mt->h.n_pivots) return MI_MAX_PIVOTS;
    return x_run(mt, is_max, target > 0 ? target - n1 : 0, a);
}

int x_check_device(int device)
{
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(MI_BAD_ARG, "device %d out of range (%d visible)", device, ndev);
    return MI_OK;
}

// a kernel's kXInexact / kXOverflow as the ABI's error, any other status as it is
int x_exact_status(int st, int max_bits = 128)
{
    if (st == kXInexact) return fail(MI_EXACT_INEXACT, "a fraction-free division left a remainder (internal error)");
    if (st == kXOverflow) return fail(MI_EXACT_OVERFLOW, "an entry of the exact tableau needs more than %d bits", max_bits);
    return st;
}
int x_status(mi355x_xtab *t, int st)
{
    if (st == kXOverflow) t->dead = true;
    return x_exact_status(st, t->max_bits);
}

int x_create(mi355x_xtab **out, int64_t rows, int64_t cols, const int64_t *num, const int64_t *den, const int64_t *basis,
             int device, int min_bits, int max_bits);

}  // namespace

int mi355x_xtab_create(mi355x_xtab **out, int64_t rows, int64_t cols, const int64_t *num, const int64_t *den,
                       const int64_t *basis, int device, int min_bits)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (rows < 1 || cols < 1 || !num || !den || (rows > 1 && !basis))
        return fail(MI_BAD_ARG, "bad shape or NULL array");
    if (min_bits != 0 && min_bits != 64 && min_bits != 128) return fail(MI_BAD_ARG, "min_bits must be 0, 64 or 128");
    return x_create(out, rows, cols, num, den, basis, device, min_bits, 128);
}

int mi355x_xtab_create_wide(mi355x_xtab **out, int64_t rows, int64_t cols, const int64_t *num, const int64_t *den,
                            const int64_t *basis, int device, int min_bits, int max_bits)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (max_bits != 128 && max_bits != 256) return fail(MI_BAD_ARG, "max_bits must be 128 or 256");
    if ((min_bits != 0 && min_bits != 64 && min_bits != 128 && min_bits != 256) || min_bits > max_bits)
        return fail(MI_BAD_ARG, "min_bits must be 0, 64, 128 or 256 and at most max_bits");
    if (rows < 1 || cols < 1 || !num || !den || (rows > 1 && !basis))
        return fail(MI_BAD_ARG, "bad shape or NULL array");
    return x_create(out, rows, cols, num, den, basis, device, min_bits, max_bits);
}

namespace {
// what both create entry points do once their arguments' ranges are checked
int x_create(mi355x_xtab **out, int64_t rows, int64_t cols, const int64_t *num, const int64_t *den, const int64_t *basis,
             int device, int min_bits, int max_bits)
{
    for (int64_t k = 0; k < rows * cols; ++k)
        if (den[k] <= 0) return fail(MI_BAD_ARG, "denominator %lld of entry %lld is not positive", (long long)den[k], (long long)k);
    int rc = x_check_device(device);
    if (rc != MI_OK) return rc;
    mi355x_xtab *t = new (std::nothrow) mi355x_xtab;
    if (!t) return fail(MI_NO_MEMORY, "host allocation failed");
    t->device = device;
    t->max_bits = max_bits;
    t->rows = rows;
    t->cols = cols;
    t->num.assign(num, num + rows * cols);
    t->den.assign(den, den + rows * cols);
    t->basis0.assign(basis ? basis : num, basis ? basis + (rows - 1) : num);
    const int64_t m = rows - 1;
    t->start_ok = x_start_ok(rows, cols, t->num.data(), t->den.data(), t->basis0.data());
    auto undo = [&](int code) { mi355x_xtab_destroy(t); return code; };
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) != hipSuccess)
        return undo(fail(MI_HIP_ERROR, "stream creation failed"));
    if (hipMalloc(&t->v.ctl, sizeof(XCtl)) != hipSuccess ||
        (m > 0 && hipMalloc(&t->v.basis, m * sizeof(int64_t)) != hipSuccess) ||
        hipMalloc(&t->v.trace_ec, kXTraceCap * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&t->v.trace_cr, kXTraceCap * sizeof(int64_t)) != hipSuccess)
        return undo(fail(MI_NO_MEMORY, "device allocation failed"));
    t->v.rows = rows;
    t->v.cols = cols;
    t->v.trace_cap = kXTraceCap;
    rc = x_reset_wider(t, min_bits > 64 ? min_bits / 2 : 32);
    if (rc == kXOverflow) return undo(fail(MI_EXACT_OVERFLOW, "the start state needs more than %d bits", max_bits));
    if (rc != MI_OK) return undo(rc);
    *out = t;
    return MI_OK;
}
}  // namespace

int mi355x_xtab_solve(mi355x_xtab *t, int is_max, int64_t max_pivots, int64_t *n_pivots)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    if (n_pivots) *n_pivots = 0;
    if (t->dead) return fail(MI_EXACT_OVERFLOW, "the tableau overflowed %d bits", t->max_bits);
    if (t->derived || t->tp_main) return fail(MI_BAD_ARG, "a tableau of a two-phase job: use mi355x_xtab_solve_two_phase");
    if (!t->start_ok) return fail(MI_UNSUPPORTED, "the basis columns are not exact unit columns with a zero objective entry");
    int rc = use_device_id(t->device);
    if (rc != MI_OK) return rc;
    const int64_t k0 = t->h.n_pivots, cap = max_pivots > 0 ? k0 + max_pivots : 0;
    int st;
    for (;;) {
        st = x_run(t, is_max, cap, nullptr);
        if (st == kXOverflow && t->bits < t->max_bits) {
            // the whole solve again from the start at the next width: the same pivots, up to the same count
            rc = x_reset_wider(t, t->bits);
            if (rc == kXOverflow) { st = rc; break; }
            if (rc != MI_OK) return rc;
            continue;
        }
        break;
    }
    if (n_pivots) *n_pivots = std::max<int64_t>(0, t->h.n_pivots - k0);
    return x_status(t, st);
}

int mi355x_xtab_solve_two_phase(mi355x_xtab *art, mi355x_xtab *mt, int main_is_max, int64_t max_pivots,
                                int64_t *n_pivots)
{
    if (!art || !mt || art == mt) return fail(MI_BAD_ARG, "two distinct handles are needed");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    if (n_pivots) n_pivots[0] = n_pivots[1] = 0;
    if (art->rows != mt->rows || mt->cols > art->cols || art->device != mt->device)
        return fail(MI_BAD_ARG, "the tableaux do not belong to one problem");
    if (art->derived || mt->tp_main) return fail(MI_BAD_ARG, "handles used in another role");
    if (art->tp_main && art->tp_main != mt) return fail(MI_BAD_ARG, "the artificial tableau belongs to another job");
    if (art->max_bits != mt->max_bits) return fail(MI_BAD_ARG, "the two tableaux allow different widths (max_bits)");
    if (art->dead || mt->dead) return fail(MI_EXACT_OVERFLOW, "the tableaux overflowed %d bits", art->max_bits);
    if (!art->start_ok) return fail(MI_UNSUPPORTED, "the basis columns are not exact unit columns with a zero objective entry");
    int rc = use_device_id(art->device);
    if (rc != MI_OK) return rc;
    if (!art->tp_main) {
        art->tp_main = mt;
        mt->derived = true;
        if (art->bits != mt->bits) {                 // one width for the job (both still at their start)
            const int wide = std::max(art->bits, mt->bits);
            rc = x_reset(art->bits < mt->bits ? art : mt, wide);
            if (rc == kXOverflow) rc = x_reset_wider(art, mt, wide);
            if (rc == kXOverflow) { art->dead = mt->dead = true; return x_status(art, rc); }
            if (rc != MI_OK) return rc;
        }
    }
    const int64_t n1 = art->h.n_pivots + art->tp_driveouts, n2 = art->tp_phase == 1 ? mt->h.n_pivots : 0;
    const int64_t target = max_pivots > 0 ? n1 + n2 + max_pivots : 0;
    int st;
    for (;;) {
        st = x_two_phase(art, mt, main_is_max, target);
        if (st == kXOverflow && art->bits < art->max_bits) {
            // both phases again from the start at the next width, up to the same pivot count
            rc = x_reset_wider(art, mt, art->bits);
            if (rc == kXOverflow) { st = rc; break; }
            if (rc != MI_OK) return rc;
            art->tp_phase = 0;
            art->tp_driveouts = 0;
            continue;
        }
        if (st < 0 && st != kXOverflow && st != kXInexact) return st;
        break;
    }
    if (st == kXOverflow) mt->dead = true;
    if (n_pivots) {
        n_pivots[0] = std::max<int64_t>(0, art->h.n_pivots + art->tp_driveouts - n1);
        n_pivots[1] = art->tp_phase == 1 ? std::max<int64_t>(0, mt->h.n_pivots - n2) : 0;
    }
    return x_status(art, st);
}

int mi355x_xtab_download(mi355x_xtab *t, int64_t *num_lo_hi, int64_t *den_lo_hi, int64_t *basis)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (t->dead) return fail(MI_EXACT_OVERFLOW, "the tableau overflowed %d bits", t->max_bits);
    if (t->bits > 128)
        return fail(MI_BAD_ARG, "a tableau at %d bits has no (low, high) form: use mi355x_xtab_download_limbs with 4 limbs", t->bits);
    int rc = use_device_id(t->device);
    if (rc != MI_OK) return rc;
    rc = x_download_lo_hi(t->v.T, t->bits, t->stream, 0, t->rows * t->cols, t->h.D, num_lo_hi, den_lo_hi);
    if (rc != MI_OK) return rc;
    if (basis && t->rows > 1)
        HIP_TRY(hipMemcpy(basis, t->v.basis, (t->rows - 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi355x_xtab_download_limbs(mi355x_xtab *t, int limbs, int64_t *num_limbs, int64_t *den_limbs, int64_t *basis)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (limbs != 2 && limbs != 4) return fail(MI_BAD_ARG, "limbs must be 2 or 4");
    if (t->dead) return fail(MI_EXACT_OVERFLOW, "the tableau overflowed %d bits", t->max_bits);
    if (t->bits > 64 * limbs) return fail(MI_BAD_ARG, "a tableau at %d bits does not fit %d limbs", t->bits, limbs);
    int rc = use_device_id(t->device);
    if (rc != MI_OK) return rc;
    rc = t->bits == 256 ? x_download_limbs<X256>(t, limbs, num_limbs, den_limbs)
                        : x_download_limbs<i128_t>(t, limbs, num_limbs, den_limbs);
    if (rc != MI_OK) return rc;
    if (basis && t->rows > 1)
        HIP_TRY(hipMemcpy(basis, t->v.basis, (t->rows - 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi355x_xtab_trace(mi355x_xtab *t, int64_t *ecs, int64_t *crs, int64_t cap, int64_t *n)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = use_device_id(t->device);
    if (rc != MI_OK) return rc;
    return download_trace(t->v.trace_ec, t->v.trace_cr, t->h.trace_n, kXTraceCap, t->stream, ecs, crs, cap, n);
}

int mi355x_xtab_bits(const mi355x_xtab *t, int *bits)
{
    if (!t || !bits) return fail(MI_BAD_ARG, "NULL argument");
    *bits = t->bits;
    return MI_OK;
}

int mi355x_xtab_set_pivot_rule(mi355x_xtab *t, int rule)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    if (rule != MI_RULE_DANTZIG && rule != MI_RULE_BLAND && rule != MI_RULE_DANTZIG_BLAND)
        return fail(MI_BAD_ARG, "unknown pivot rule %d", rule);
    if (t->h.n_pivots > 0 || t->tp_phase != 0 || t->tp_driveouts > 0)
        return fail(MI_BAD_ARG, "the pivot rule is set before the handle's first pivot");
    t->v.rule = rule;                            // (k_x_select reads it there; no reset touches it)
    t->h.stall = 0;                              // (x_run writes the mirror to the device before its first launch)
    return MI_OK;
}

int mi355x_xtab_cancel(mi355x_xtab *t)
{
    if (!t) return fail(MI_BAD_ARG, "handle is NULL");
    t->cancel.store(1, std::memory_order_release);
    return MI_OK;
}

void mi355x_xtab_destroy(mi355x_xtab *t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    x_free_width(t);
    (void)hipFree(t->v.ctl);
    (void)hipFree(t->v.basis);
    (void)hipFree(t->v.trace_ec);
    (void)hipFree(t->v.trace_cr);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}
