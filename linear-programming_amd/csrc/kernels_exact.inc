// kernels_exact.inc -- exact rational solves on fraction-free (Bareiss) integer tableaux.
// Part of simplex_kernels.hip (ONE translation unit: included there, in this order, inside namespace mi355x).
//
// The reference's `rational` dispatch of fp=, fp<, fp> is plain =, <, > (src/utils.lisp:84-124), and
// its tableau then holds ratios.  Here the tableau is one integer matrix T and one integer D > 0 with
// t_ij = T_ij / D for every row (simplex_kernels.h, XCtl / XView):
//   pricing     compares T directly (D > 0): lowest-index strict arg-min (max) / arg-max (min) of the
//               objective row over [0, var_count); the column enters iff its value is < 0 (> 0)
//   ratio test  rows with T_ie > 0; rhs_a / a_a < rhs_b / a_b as rhs_a * a_b < rhs_b * a_a at double
//               width; strict, the lowest row wins a tie
//   pivot       (r, e), p = T_re:  T'_rj = sgn(p) T_rj,
//                                   T'_ij = (T_ij |p| - sgn(p) T_ie T_rj) / D   (i != r),   D' = |p|
// (Both choices are the reference's, MI_RULE_DANTZIG.  The opt-in rules replace them in x_price and x_ratio:
// Bland's lowest eligible column and lowest basis column among tied rows, always or after a degenerate pivot.)
// Every division is exact (Sylvester's identity).  It is done as: shift out the 2^k factor of D,
// multiply by the inverse of its odd part modulo 2^W, and verify q * D == N at double width.  A
// failed check tells overflow (the quotient does not fit the width) from a remainder (a bug) by a
// slow bitwise remainder, which only ever runs on that path.
//
// W = 64: int64_t storage, __int128 products.  W = 128: __int128 storage, 256-bit products as two
// 128-bit limbs (S256 below).  W = 256 (the single tableau only): X256 storage, X512 products, both from
// xwide.h -- the overloads below hand the rules its functions.  Plain C++ throughout.
//
//   k_x_select<T, kRules>  one workgroup: pricing, ratio test, pivot record, snapshots col / prow (kRules: the
//                    handle's pivot rule is not the reference's -- MI_RULE_BLAND, MI_RULE_DANTZIG_BLAND)
//   k_x_force<T>     one workgroup: the same record and snapshots for a given pivot (drive-out)
//   k_x_update<T>    the rank-1 update with the exact division (every element once)
//   k_x_handover<T>  main tableau of the two-phase hand-over: constraint rows scaled by L_c and the
//                    objective row re-eliminated, D_main = L_c * D_art
// The rules themselves -- x_price, x_ratio, x_record, x_snapshot, x_update_elem, x_handover_column -- stand
// here once; the kernels above and the batch kernels (kernels_exact_batch.inc) are loops around them.

typedef unsigned __int128 xu128;

// ---- 256-bit two's complement: value = hi * 2^128 + lo -------------------------------------
struct S256 { xu128 lo; __int128 hi; };

__device__ inline S256 s256_of(__int128 x) { S256 r; r.lo = (xu128)x; r.hi = x < 0 ? -1 : 0; return r; }
__device__ inline S256 s256_neg(S256 x)
{
    S256 r;
    r.lo = ~x.lo + 1;
    r.hi = (__int128)(~(xu128)x.hi + (r.lo == 0 ? 1 : 0));
    return r;
}
__device__ inline S256 s256_add(S256 a, S256 b)
{
    S256 r;
    r.lo = a.lo + b.lo;
    r.hi = (__int128)((xu128)a.hi + (xu128)b.hi + (r.lo < a.lo ? 1 : 0));
    return r;
}
__device__ inline S256 s256_sub(S256 a, S256 b)
{
    S256 r;
    r.lo = a.lo - b.lo;
    r.hi = (__int128)((xu128)a.hi - (xu128)b.hi - (a.lo < b.lo ? 1 : 0));
    return r;
}
__device__ inline bool s256_lt(S256 a, S256 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ inline bool s256_eq(S256 a, S256 b) { return a.hi == b.hi && a.lo == b.lo; }
// |a| * |b| for magnitudes below 2^127
__device__ inline S256 u128_mul(xu128 a, xu128 b)
{
    const uint64_t a0 = (uint64_t)a, a1 = (uint64_t)(a >> 64), b0 = (uint64_t)b, b1 = (uint64_t)(b >> 64);
    const xu128 p00 = (xu128)a0 * b0, p01 = (xu128)a0 * b1, p10 = (xu128)a1 * b0, p11 = (xu128)a1 * b1;
    const xu128 mid = (p00 >> 64) + (uint64_t)p01 + (uint64_t)p10;
    S256 r;
    r.lo = (mid << 64) | (uint64_t)p00;
    r.hi = (__int128)(p11 + (p01 >> 64) + (p10 >> 64) + (mid >> 64));
    return r;
}

// ---- width-generic operations: int64_t -> __int128 products, __int128 -> S256 products ----------
__device__ inline __int128 xmul(int64_t a, int64_t b) { return (__int128)a * b; }
__device__ inline S256 xmul(__int128 a, __int128 b)
{
    const bool neg = (a < 0) != (b < 0);
    const S256 p = u128_mul(a < 0 ? -(xu128)a : (xu128)a, b < 0 ? -(xu128)b : (xu128)b);
    return neg ? s256_neg(p) : p;
}
__device__ inline __int128 xsub(__int128 a, __int128 b) { return a - b; }   // operands below 2^126 in magnitude
__device__ inline S256 xsub(S256 a, S256 b) { return s256_sub(a, b); }       // operands below 2^254 in magnitude
__device__ inline bool xlt(__int128 a, __int128 b) { return a < b; }
__device__ inline bool xlt(S256 a, S256 b) { return s256_lt(a, b); }
__device__ inline bool xeq(__int128 a, __int128 b) { return a == b; }
__device__ inline bool xeq(S256 a, S256 b) { return s256_eq(a, b); }
// accumulation that may overflow the double width (the hand-over's sums): false on overflow
__device__ inline bool xsub_ovf(__int128 &acc, __int128 b) { return !__builtin_sub_overflow(acc, b, &acc); }
__device__ inline bool xsub_ovf(S256 &acc, S256 b)
{
    const S256 r = s256_sub(acc, b);
    const bool ovf = ((acc.hi < 0) != (b.hi < 0)) && ((r.hi < 0) != (acc.hi < 0));
    acc = r;
    return !ovf;
}
// a double-width value -> the storage width, inside the symmetric range
__device__ inline bool xfit(__int128 x, int64_t *out)
{
    if (x <= -(__int128)INT64_MAX - 1 || x > (__int128)INT64_MAX) return false;
    *out = (int64_t)x;
    return true;
}
__device__ inline bool xfit(S256 x, __int128 *out)
{
    const __int128 lo = (__int128)x.lo;
    if (x.hi != (lo < 0 ? -1 : 0)) return false;
    if (x.lo == ((xu128)1 << 127)) return false;                 // -2^127: outside the symmetric range
    *out = lo;
    return true;
}
__device__ inline bool xsym(int64_t x) { return x != INT64_MIN; }
__device__ inline bool xsym(__int128 x) { return (xu128)x != ((xu128)1 << 127); }

// |N| mod d by shift and subtract (the failure path only): N below 2^255 in magnitude, 0 < d < 2^127
__device__ inline xu128 xrem(S256 N, xu128 d)
{
    if (N.hi < 0) N = s256_neg(N);
    xu128 r = 0;
    for (int b = 255; b >= 0; --b) {
        const xu128 bit = b >= 128 ? (((xu128)N.hi >> (b - 128)) & 1) : ((N.lo >> b) & 1);
        r = (r << 1) | bit;
        if (r >= d) r -= d;
    }
    return r;
}

// q = N / D exactly, D = 2^shift * odd, inv = odd^-1 mod 2^W.  0, kXOverflow or kXInexact.
__device__ inline int xdiv(__int128 N, int64_t D, int shift, uint64_t inv, int64_t *q)
{
    if (shift && ((uint64_t)N & ((1ull << shift) - 1))) return kXInexact;
    const int64_t qs = (int64_t)((uint64_t)(N >> shift) * inv);
    if (xsym(qs) && (__int128)qs * D == N) { *q = qs; return 0; }
    return xrem(s256_of(N), (xu128)D) == 0 ? kXOverflow : kXInexact;
}
__device__ inline int xdiv(S256 N, __int128 D, int shift, xu128 inv, __int128 *q)
{
    if (shift && (N.lo & ((((xu128)1) << shift) - 1))) return kXInexact;
    xu128 lo = N.lo;
    if (shift) lo = (N.lo >> shift) | ((xu128)N.hi << (128 - shift));
    const __int128 qs = (__int128)(lo * inv);
    if (xsym(qs) && s256_eq(xmul(qs, D), N)) { *q = qs; return 0; }
    return xrem(N, (xu128)D) == 0 ? kXOverflow : kXInexact;
}

template <class U> __device__ inline U xinv_odd(U d)
{
    U x = d;                                  // correct to 3 bits; each Newton step doubles them
    for (int i = 0; i < 7; ++i) x *= (U)2 - d * x;
    return x;
}
__device__ inline int xctz(xu128 d)
{
    const uint64_t lo = (uint64_t)d;
    return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll((uint64_t)(d >> 64));
}

// ---- the same overload set at W = 256: X256 -> X512 products (xwide.h) ---------------------------------
__device__ inline X512 xmul(const X256 &a, const X256 &b) { return xw_mul(a, b); }
__device__ inline X512 xsub(const X512 &a, const X512 &b) { return a - b; }   // operands below 2^510 in magnitude
__device__ inline bool xlt(const X512 &a, const X512 &b) { return xw_lt(a, b); }
__device__ inline bool xeq(const X512 &a, const X512 &b) { return xw_eq(a, b); }
__device__ inline bool xsub_ovf(X512 &acc, const X512 &b) { return xw_sub_ovf(acc, b); }
__device__ inline bool xfit(const X512 &x, X256 *out) { return xw_fit<4>(x, out); }
__device__ inline bool xsym(const X256 &x) { return !xw_is_min(x); }
__device__ inline XU256 xrem(const X512 &N, const XU256 &d) { return xw_rem<4>(N, d); }   // N below 2^511 in magnitude, 0 < d < 2^255
__device__ inline int xctz(const XU256 &d) { return xw_ctz(d); }
// xinv_odd<XU256> is the template above: 3 * 2^7 = 384 correct bits after its seven steps, 256 needed (128 bits
// need six of them, 64 five)
__device__ inline int xdiv(const X512 &N, const X256 &D, int shift, const XU256 &inv, X256 *q)
{
    if (shift && xw_ctz_limbs<8>(N.l) < shift) return kXInexact;
    const X256 qs = (XUWide<4>(X256(xw_sar(N, shift))) * inv).as_signed();
    if (xsym(qs) && xeq(xmul(qs, D), N)) { *q = qs; return 0; }
    const XU256 r = xrem(N, XU256(D));
    return xw_ctz(r) == 256 ? kXOverflow : kXInexact;
}

template <class T> struct XUnsigned;
template <> struct XUnsigned<int64_t>  { typedef uint64_t type; };
template <> struct XUnsigned<__int128> { typedef xu128 type; };
template <> struct XUnsigned<X256>     { typedef XU256 type; };

// the pivot record and the denominator of a width: XPivot and __int128 up to 128 bits, their twins at 256
// (XCtl, simplex_kernels.h)
template <class T> struct XRec {
    typedef XPivot Pivot;
    typedef __int128 Wide;
    __device__ static Wide  &D(XCtl *c) { return c->D; }
    __device__ static Pivot &piv(XCtl *c) { return c->piv; }
};
template <> struct XRec<X256> {
    typedef XPivotW Pivot;
    typedef X256 Wide;
    __device__ static Wide  &D(XCtl *c) { return c->Dw; }
    __device__ static Pivot &piv(XCtl *c) { return c->pivw; }
};

// what xdiv takes besides D = 2^shift * odd, D > 0: the shift and the inverse of the odd part modulo 2^W
template <class T> __device__ inline void x_div_setup(__int128 D, int32_t *shift, __int128 *inv)
{
    typedef typename XUnsigned<T>::type U;
    const int sh = xctz((xu128)D);
    *shift = sh;
    *inv = (__int128)xinv_odd<U>((U)(D >> sh));
}
template <class T> __device__ inline void x_div_setup(const X256 &D, int32_t *shift, X256 *inv)
{
    const int sh = xctz(XU256(D));
    *shift = sh;
    *inv = xinv_odd<XU256>(xw_shr(XU256(D), sh)).as_signed();
}

// ---- what the single tableau and the batches (kernels_exact_batch.inc) share: one copy of each rule ----
// the power of two the reduction trees start from: slots at and above it hold no candidate and are never read
__device__ inline int x_tree_top(int64_t n)
{
    int top = 1;
    while (top < kXThreads && top < n) top <<= 1;
    return top;
}

// x_price and x_ratio: every thread of the workgroup calls them, with the same arguments.  sv, sa, si:
// kXThreads slots of LDS each, free again on return (both end on a barrier, after the read of slot 0).
//
// find-entering-column (src/simplex.lisp:362-379), rational dispatch: the lowest index of the strict
// minimum (max) / maximum (min) of obj[0, nv) if that value is < 0 (> 0), -1 otherwise (optimal).
// bland (the same in every thread): Bland's choice instead, the lowest j < nv with obj[j] < 0 (> 0); no values
// go through LDS then, every thread stops at the first such j of its stride and the tree takes the minimum.
template <class T> __device__ __forceinline__ int64_t x_price(const T *obj, int64_t nv, int is_max, bool bland, T *sv, int64_t *si)
{
    const int tid = threadIdx.x;
    int64_t bi = -1;
    if (bland) {
        for (int64_t j = tid; j < nv; j += kXThreads) {
            const T x = obj[j];
            if (is_max ? x < 0 : x > 0) { bi = j; break; }
        }
        si[tid] = bi;
        __syncthreads();
        for (int s = x_tree_top(nv) / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const int64_t o = si[tid + s];
                if (o >= 0 && (si[tid] < 0 || o < si[tid])) si[tid] = o;
            }
            __syncthreads();
        }
        const int64_t ec = si[0];
        __syncthreads();
        return ec;
    }
    T bv = 0;
    for (int64_t j = tid; j < nv; j += kXThreads) {
        const T x = obj[j];
        if (bi < 0 || (is_max ? x < bv : x > bv)) { bv = x; bi = j; }
    }
    sv[tid] = bv; si[tid] = bi;
    __syncthreads();
    for (int s = x_tree_top(nv) / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int o = tid + s;
            if (si[o] >= 0 && (si[tid] < 0 || (is_max ? sv[o] < sv[tid] : sv[o] > sv[tid]) ||
                               (sv[o] == sv[tid] && si[o] < si[tid]))) { sv[tid] = sv[o]; si[tid] = si[o]; }
        }
        __syncthreads();
    }
    const int64_t ec = si[0];
    const T best = sv[0];
    __syncthreads();
    return ec >= 0 && (is_max ? best < 0 : best > 0) ? ec : -1;
}

// find-pivoting-row (src/simplex.lisp:382-389), cross-multiplied: the lowest row of the strict minimum of
// M[i][nv] / M[i][ec] over the rows i < m with M[i][ec] > 0, -1 if there is none (unbounded).  C: M's columns.
// bland (the same in every thread): among the rows of the minimum the one whose basis column basis[i] is lowest
// instead; the key of each kept row then goes through sk (kXThreads slots of LDS, untouched otherwise) beside it.
template <class T> __device__ __forceinline__ int64_t x_ratio(const T *M, int64_t m, int64_t C, int64_t nv, int64_t ec,
                                                              const int64_t *basis, bool bland, T *sv, T *sa, int64_t *si,
                                                              int64_t *sk)
{
    const int tid = threadIdx.x;
    int64_t bi = -1, bk = 0;
    T br = 0, ba = 0;
    for (int64_t i = tid; i < m; i += kXThreads) {
        const T a = M[i * C + ec];
        if (a > 0) {
            const T r = M[i * C + nv];
            bool better = bi < 0;
            if (!better) {
                const auto lhs = xmul(r, ba), rhs = xmul(br, a);
                better = xlt(lhs, rhs) || (bland && xeq(lhs, rhs) && basis[i] < bk);
            }
            if (better) { br = r; ba = a; bi = i; if (bland) bk = basis[i]; }
        }
    }
    sv[tid] = br; sa[tid] = ba; si[tid] = bi;
    if (bland) sk[tid] = bk;
    __syncthreads();
    for (int s = x_tree_top(m) / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int o = tid + s;
            if (si[o] >= 0) {
                bool better = si[tid] < 0;
                if (!better) {
                    const auto lhs = xmul(sv[o], sa[tid]), rhs = xmul(sv[tid], sa[o]);
                    better = xlt(lhs, rhs) || (xeq(lhs, rhs) && (bland ? sk[o] < sk[tid] : si[o] < si[tid]));
                }
                if (better) { sv[tid] = sv[o]; sa[tid] = sa[o]; si[tid] = si[o]; if (bland) sk[tid] = sk[o]; }
            }
        }
        __syncthreads();
    }
    const int64_t cr = si[0];
    __syncthreads();
    return cr;
}

// the rule in force at one selection (MI_RULE_*): Bland's under rule 1, and under rule 2 while the member's
// stall flag stands (its last selected pivot was degenerate)
__device__ inline bool x_bland(int rule, int stall) { return rule == 1 || (rule == 2 && stall != 0); }

// the pivot record of (ec, cr) on a tableau with denominator D -- one thread; D' is r->pa
template <class T> __device__ inline void x_record(typename XRec<T>::Pivot *r, const T *M, int64_t C, int64_t ec, int64_t cr,
                                                   typename XRec<T>::Wide D)
{
    const T p = M[cr * C + ec];
    r->ec = ec;
    r->cr = cr;
    r->sgn = p < 0 ? -1 : 1;
    r->pa = (typename XRec<T>::Wide)(p < 0 ? -p : p);
    r->dold = D;
    x_div_setup<T>(D, &r->shift, &r->inv);
}

// the record at the width, in registers: what the snapshots and the update of one pivot take
template <class T> struct XPivotT {
    typedef typename XUnsigned<T>::type U;
    int64_t ec, cr;
    int     sgn, shift;
    T       pa, dold;
    U       inv;
    __device__ explicit XPivotT(const typename XRec<T>::Pivot &r)
        : ec(r.ec), cr(r.cr), sgn(r.sgn), shift(r.shift), pa((T)r.pa), dold((T)r.dold), inv((U)r.inv) {}
};

// the entering column times sgn into col (R values) and the pivot row into prow (C values), global or LDS:
// every thread of the workgroup calls this
template <class T> __device__ __forceinline__ void x_snapshot(const T *M, int64_t R, int64_t C, const XPivotT<T> &p, T *col, T *prow)
{
    for (int64_t i = threadIdx.x; i < R; i += kXThreads) {
        const T a = M[i * C + p.ec];
        col[i] = p.sgn < 0 ? -a : a;
    }
    for (int64_t j = threadIdx.x; j < C; j += kXThreads) prow[j] = M[p.cr * C + j];
}

// the update of *x = T[r][j] from the snapshots' cv = col[r] and pv = prow[j].  0, kXOverflow or kXInexact
// (*x is left as it was then)
template <class T> __device__ __forceinline__ int x_update_elem(T *x, int64_t r, T cv, T pv, const XPivotT<T> &p)
{
    if (r == p.cr) { *x = p.sgn < 0 ? -pv : pv; return 0; }
    T q;
    const int e = xdiv(xsub(xmul(*x, p.pa), xmul(cv, pv)), p.dold, p.shift, p.inv, &q);
    if (!e) *x = q;
    return e;
}

// Column j of the hand-over's main tableau M (Cm columns) from the artificial one A (Ca columns, denominator
// D), m constraint rows: M[r][j] = lc * A[r][src] and M[m][j] = D * cl[j] - sum_r w[r] * A[r][src], src = j but
// the artificial right-hand side for the last column.  false: a value left the width (0 is stored for it).
template <class T> __device__ __forceinline__ bool x_handover_column(const T *A, int64_t Ca, T *M, int64_t Cm, int64_t m,
                                                                     int64_t j, T D, const T *w, const T *cl, T lc)
{
    const int64_t src = j < Cm - 1 ? j : Ca - 1;
    auto acc = xmul(D, cl[j]);
    bool ok = true;
    for (int64_t r = 0; r < m; ++r) {
        const T x = A[r * Ca + src];
        T y = 0;
        if (!xfit(xmul(lc, x), &y)) ok = false;
        M[r * Cm + j] = y;
        if (!xsub_ovf(acc, xmul(w[r], x))) ok = false;
    }
    T o = 0;
    if (!xfit(acc, &o)) ok = false;
    M[m * Cm + j] = o;
    return ok;
}

// kRules false: the reference's rule alone, compiled without the other two (v.rule == MI_RULE_DANTZIG is launched
// so: its code and its LDS are what they were before the rules came); true: v.rule decides at run time
template <class T, bool kRules> __global__ __launch_bounds__(kXThreads) void k_x_select(XView v, int is_max)
{
    XCtl *c = v.ctl;
    const T *M = (const T *)v.T;
    const int tid = threadIdx.x;
    const int64_t m = v.rows - 1, nv = v.cols - 1, C = v.cols;
    __shared__ int go, s_bland;
    __shared__ T sv[kXThreads], sa[kXThreads];
    __shared__ int64_t si[kXThreads], sk[kRules ? kXThreads : 1];
    if (tid == 0) {
        int g = 0;
        c->apply = 0;
        if (c->status == kRunning) {
            if (c->err) c->status = c->err;
            else if (c->cap_at > 0 && c->n_pivots >= c->cap_at) c->status = 3;           // MI_MAX_PIVOTS
            else g = 1;
        }
        go = g;
        if (kRules) s_bland = x_bland(v.rule, c->stall);
    }
    __syncthreads();
    if (!go) return;
    const bool bland = kRules && s_bland != 0;
    const int64_t ec = x_price<T>(M + m * C, nv, is_max, bland, sv, si);
    if (ec < 0) {
        if (tid == 0) c->status = 0;                                                        // MI_OPTIMAL
        return;
    }
    const int64_t cr = x_ratio<T>(M, m, C, nv, ec, v.basis, bland, sv, sa, si, sk);
    if (cr < 0) {
        if (tid == 0) c->status = 1;                                                        // MI_UNBOUNDED
        return;
    }
    if (tid == 0) {
        x_record<T>(&XRec<T>::piv(c), M, C, ec, cr, XRec<T>::D(c));
        XRec<T>::D(c) = XRec<T>::piv(c).pa;
        c->apply = 1;
        if (kRules && v.rule == 2) c->stall = M[cr * C + nv] == 0;    // a degenerate pivot: rule 2 selects by Bland's rule next
        v.basis[cr] = ec;
        if (c->trace_n < v.trace_cap) { v.trace_ec[c->trace_n] = ec; v.trace_cr[c->trace_n] = cr; }
        c->trace_n += 1;
        c->n_pivots += 1;
    }
    __syncthreads();
    x_snapshot<T>(M, v.rows, C, XPivotT<T>(XRec<T>::piv(c)), (T *)v.col, (T *)v.prow);
}

// a pivot given by the host (the drive-out of src/simplex.lisp:418-436): not counted, not traced
template <class T> __global__ __launch_bounds__(kXThreads) void k_x_force(XView v, int64_t ec, int64_t cr)
{
    XCtl *c = v.ctl;
    const T *M = (const T *)v.T;
    if (threadIdx.x == 0) {
        x_record<T>(&XRec<T>::piv(c), M, v.cols, ec, cr, XRec<T>::D(c));
        XRec<T>::D(c) = XRec<T>::piv(c).pa;
        c->apply = 1;
        v.basis[cr] = ec;
    }
    __syncthreads();
    x_snapshot<T>(M, v.rows, v.cols, XPivotT<T>(XRec<T>::piv(c)), (T *)v.col, (T *)v.prow);
}

template <class T> __global__ __launch_bounds__(256) void k_x_update(XView v)
{
    XCtl *c = v.ctl;
    if (!c->apply) return;
    T *M = (T *)v.T;
    const T *col = (const T *)v.col, *prow = (const T *)v.prow;
    const int64_t C = v.cols;
    const XPivotT<T> p(XRec<T>::piv(c));
    int err = 0;
    for (int64_t r = blockIdx.y; r < v.rows; r += gridDim.y) {
        const T cv = col[r];
        for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < C; j += (int64_t)gridDim.x * blockDim.x)
            err = max(err, x_update_elem<T>(M + r * C + j, r, cv, prow[j], p));
    }
    if (err) atomicMax(&c->err, err);
}

template <class T> __global__ __launch_bounds__(256) void k_x_handover(XView a, XView mt, const T *w, const T *cl, T lc)
{
    const T D = (T)XRec<T>::D(a.ctl);
    int err = 0;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < mt.cols; j += (int64_t)gridDim.x * blockDim.x)
        if (!x_handover_column<T>((const T *)a.T, a.cols, (T *)mt.T, mt.cols, a.rows - 1, j, D, w, cl, lc)) err = kXOverflow;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        T d = 0;
        if (!xfit(xmul(lc, D), &d)) err = kXOverflow;
        XRec<T>::D(mt.ctl) = (typename XRec<T>::Wide)d;
    }
    if (err) atomicMax(&mt.ctl->err, err);
}

static unsigned x_grid_x(int64_t cols) { const int64_t g = (cols + 255) / 256; return (unsigned)(g < 64 ? g : 64); }
static unsigned x_grid_y(int64_t rows) { return (unsigned)(rows < 4096 ? rows : 4096); }

// f(T()) with T the storage type of `bits`: the int64_t / __int128 pair of every exact launcher (the batches'
// and branch-and-bound's too, which stop at 128 bits) ...
template <class F> static void x_with_width(int bits, F f)
{
    if (bits == 64) f((int64_t)0);
    else            f((__int128)0);
}
// ... and its third case, for the launchers of the single tableau alone
template <class F> static void x_with_tab_width(int bits, F f)
{
    if (bits == 256) f(X256());
    else             x_with_width(bits, f);
}

void launch_x_select(const XView &v, int is_max, hipStream_t s)
{
    x_with_tab_width(v.bits, [&](auto t) {
        typedef decltype(t) T;
        if (v.rule) hipLaunchKernelGGL((k_x_select<T, true>), dim3(1), dim3(kXThreads), 0, s, v, is_max);
        else        hipLaunchKernelGGL((k_x_select<T, false>), dim3(1), dim3(kXThreads), 0, s, v, is_max);
    });
}
void launch_x_force(const XView &v, int64_t ec, int64_t cr, hipStream_t s)
{
    x_with_tab_width(v.bits, [&](auto t) { hipLaunchKernelGGL(k_x_force<decltype(t)>, dim3(1), dim3(kXThreads), 0, s, v, ec, cr); });
}
void launch_x_update(const XView &v, hipStream_t s)
{
    const dim3 grid(x_grid_x(v.cols), x_grid_y(v.rows));
    x_with_tab_width(v.bits, [&](auto t) { hipLaunchKernelGGL(k_x_update<decltype(t)>, grid, dim3(256), 0, s, v); });
}
void launch_x_handover(const XView &art, const XView &mt, const void *w, const void *cl, const void *lc, hipStream_t s)
{
    const dim3 grid((unsigned)((mt.cols + 255) / 256));
    x_with_tab_width(mt.bits, [&](auto t) {
        typedef decltype(t) T;
        T lcv;
        __builtin_memcpy(&lcv, lc, sizeof(T));
        hipLaunchKernelGGL(k_x_handover<T>, grid, dim3(256), 0, s, art, mt, (const T *)w, (const T *)cl, lcv);
    });
}

#ifdef MI355X_TEST_HOOKS
// ---- the arithmetic above, one primitive per launch, element-wise (test build only) -------------
// Element i of a, b and out is four little-endian 64-bit limbs at [4 i, 4 i + 4); a narrower value
// takes the low limbs (out: the rest is zero).  rc[i]: the primitive's own status or flag, -1 for an
// operand outside the primitive's precondition (a divisor <= 0, xctz of 0), which is then not called.
__device__ inline __int128 xp_i128(const int64_t *p) { return (__int128)(((xu128)(uint64_t)p[1] << 64) | (uint64_t)p[0]); }
__device__ inline S256 xp_s256(const int64_t *p) { S256 r; r.lo = (xu128)xp_i128(p); r.hi = xp_i128(p + 2); return r; }
__device__ inline void xp_put(int64_t *o, __int128 x) { o[0] = (int64_t)(uint64_t)(xu128)x; o[1] = (int64_t)(x >> 64); }
__device__ inline void xp_put(int64_t *o, S256 x) { xp_put(o, (__int128)x.lo); xp_put(o + 2, x.hi); }

template <int N> __device__ inline XWide<N> xp_wide(const int64_t *p)
{
    XWide<N> r;
    for (int i = 0; i < N; ++i) r.l[i] = (uint64_t)p[i];
    return r;
}
template <int N> __device__ inline void xp_put(int64_t *o, const XWide<N> &x) { for (int i = 0; i < N; ++i) o[i] = (int64_t)x.l[i]; }

__global__ __launch_bounds__(256) void k_x_arith_probe(int op, int64_t n, const int64_t *a, const int64_t *b,
                                                       int64_t *out, int32_t *rc)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t *pa = a + 4 * i, *pb = b + 4 * i;
        int64_t *o = out + 4 * i;
        int32_t st = 0;
        o[0] = o[1] = o[2] = o[3] = 0;
        switch (op) {
        case kXProbeMul64:  xp_put(o, xmul(pa[0], pb[0])); break;
        case kXProbeMul128: xp_put(o, xmul(xp_i128(pa), xp_i128(pb))); break;
        case kXProbeAdd256: xp_put(o, s256_add(xp_s256(pa), xp_s256(pb))); break;
        case kXProbeSub256: xp_put(o, s256_sub(xp_s256(pa), xp_s256(pb))); break;
        case kXProbeNeg256: xp_put(o, s256_neg(xp_s256(pa))); break;
        case kXProbeLt256:  o[0] = s256_lt(xp_s256(pa), xp_s256(pb)) ? 1 : 0; break;
        case kXProbeSubOvf64:  { __int128 acc = xp_i128(pa); st = xsub_ovf(acc, xp_i128(pb)) ? 0 : 1; xp_put(o, acc); break; }
        case kXProbeSubOvf128: { S256 acc = xp_s256(pa); st = xsub_ovf(acc, xp_s256(pb)) ? 0 : 1; xp_put(o, acc); break; }
        case kXProbeFit64:  { int64_t y = 0; st = xfit(xp_i128(pa), &y) ? 0 : 1; o[0] = y; break; }
        case kXProbeFit128: { __int128 y = 0; st = xfit(xp_s256(pa), &y) ? 0 : 1; xp_put(o, y); break; }
        case kXProbeDiv64: {
            int32_t sh; __int128 inv; int64_t q = 0;
            if (pb[0] <= 0) { st = -1; break; }
            x_div_setup<int64_t>((__int128)pb[0], &sh, &inv);
            st = xdiv(xp_i128(pa), pb[0], sh, (uint64_t)inv, &q);
            o[0] = q;
            break;
        }
        case kXProbeDiv128: {
            int32_t sh; __int128 inv, q = 0;
            if (xp_i128(pb) <= 0) { st = -1; break; }
            x_div_setup<__int128>(xp_i128(pb), &sh, &inv);
            st = xdiv(xp_s256(pa), xp_i128(pb), sh, (xu128)inv, &q);
            xp_put(o, q);
            break;
        }
        case kXProbeRem:
            if (xp_i128(pb) <= 0) { st = -1; break; }
            xp_put(o, (__int128)xrem(xp_s256(pa), (xu128)xp_i128(pb)));
            break;
        case kXProbeInv64:  o[0] = (int64_t)xinv_odd<uint64_t>((uint64_t)pa[0]); break;
        case kXProbeInv128: xp_put(o, (__int128)xinv_odd<xu128>((xu128)xp_i128(pa))); break;
        case kXProbeCtz:
            if (xp_i128(pa) == 0) { st = -1; break; }
            o[0] = xctz((xu128)xp_i128(pa));
            break;
        case kXProbeInv256: xp_put(o, xinv_odd<XU256>(XU256(xp_wide<4>(pa))).as_signed()); break;
        case kXProbeCtz256:
            if (xp_wide<4>(pa) == 0) { st = -1; break; }
            o[0] = xctz(XU256(xp_wide<4>(pa)));
            break;
        default: st = -1;
        }
        rc[i] = st;
    }
}

void launch_x_arith_probe(int op, int64_t n, const int64_t *a, const int64_t *b, int64_t *out, int32_t *rc, hipStream_t s)
{
    const int64_t g = (n + 255) / 256;
    hipLaunchKernelGGL(k_x_arith_probe, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, s, op, n, a, b, out, rc);
}

// Element i of a, b and out is eight limbs at [8 i, 8 i + 8): a 512-bit value takes all of them, a 256-bit one
// the low four (out: the rest is zero).  rc as above.
__global__ __launch_bounds__(256) void k_x_arith_probe8(int op, int64_t n, const int64_t *a, const int64_t *b,
                                                        int64_t *out, int32_t *rc)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t *pa = a + 8 * i, *pb = b + 8 * i;
        int64_t *o = out + 8 * i;
        int32_t st = 0;
        for (int k = 0; k < 8; ++k) o[k] = 0;
        switch (op) {
        case kXProbe8Mul256: xp_put(o, xmul(xp_wide<4>(pa), xp_wide<4>(pb))); break;
        case kXProbe8Add512: xp_put(o, xp_wide<8>(pa) + xp_wide<8>(pb)); break;
        case kXProbe8Sub512: xp_put(o, xsub(xp_wide<8>(pa), xp_wide<8>(pb))); break;
        case kXProbe8Neg512: xp_put(o, -xp_wide<8>(pa)); break;
        case kXProbe8Lt512:  o[0] = xlt(xp_wide<8>(pa), xp_wide<8>(pb)) ? 1 : 0; break;
        case kXProbe8Eq512:  o[0] = xeq(xp_wide<8>(pa), xp_wide<8>(pb)) ? 1 : 0; break;
        case kXProbe8SubOvf256: { X512 acc = xp_wide<8>(pa); st = xsub_ovf(acc, xp_wide<8>(pb)) ? 0 : 1; xp_put(o, acc); break; }
        case kXProbe8Fit256: { X256 y = 0; st = xfit(xp_wide<8>(pa), &y) ? 0 : 1; xp_put(o, y); break; }
        case kXProbe8Div256: {
            int32_t sh; X256 inv, q = 0;
            const X256 d = xp_wide<4>(pb);
            if (!(d > 0)) { st = -1; break; }
            x_div_setup<X256>(d, &sh, &inv);
            st = xdiv(xp_wide<8>(pa), d, sh, XU256(inv), &q);
            xp_put(o, q);
            break;
        }
        case kXProbe8Rem256: {
            const X256 d = xp_wide<4>(pb);
            if (!(d > 0)) { st = -1; break; }
            xp_put(o, xrem(xp_wide<8>(pa), XU256(d)).as_signed());
            break;
        }
        default: st = -1;
        }
        rc[i] = st;
    }
}

void launch_x_arith_probe8(int op, int64_t n, const int64_t *a, const int64_t *b, int64_t *out, int32_t *rc, hipStream_t s)
{
    const int64_t g = (n + 255) / 256;
    hipLaunchKernelGGL(k_x_arith_probe8, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, s, op, n, a, b, out, rc);
}
#endif
