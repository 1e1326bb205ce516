// xwide.h -- fixed-width two's complement integers of N 64-bit limbs, one copy for host and device.
// Included by simplex_kernels.h (so by both translation units, simplex_kernels.hip and simplex_capi.hip)
// and by plain host programs: nothing here needs HIP.  Plain C++ throughout.
//
//   XWide<N>    signed, little-endian limbs; XWide<4> is the storage type of the 256-bit exact tableaux,
//               XWide<8> carries their products (kernels_exact.inc).  A later width is another N.
//   XUWide<N>   the same limbs as an unsigned value modulo 2^(64 N): what the inverse of an odd divisor and
//               the remainder are computed in.
//
// Every loop over limbs has a compile-time trip count and is unrolled, and no limb is ever addressed by a
// run-time index (a variable shift goes by limb counts of 1, 2, 4, ... under a test of the shift's bits):
// on the device the limbs live in registers.  The functions marked host-only divide by a 64-bit value, which
// is all the host's start state and hand-over multipliers need (capi_exact.inc).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XW_HD __host__ __device__
#else
#define XW_HD
#endif
#if defined(__clang__)
#define XW_UNROLL _Pragma("unroll")
#define XW_NOUNROLL _Pragma("nounroll")
#else
#define XW_UNROLL _Pragma("GCC unroll 16")
#define XW_NOUNROLL _Pragma("GCC unroll 1")
#endif

namespace mi355x {

typedef unsigned __int128 xw_u128;

template <int N> struct XWide {
    uint64_t l[N];
    XWide() = default;
    XW_HD XWide(int64_t x)                                    // (implicit: `T x = 0`, `x < 0` in the rules)
    {
        l[0] = (uint64_t)x;
        XW_UNROLL for (int i = 1; i < N; ++i) l[i] = x < 0 ? ~0ull : 0ull;
    }
    // sign extension (M < N) or the low limbs (M > N)
    template <int M> XW_HD explicit XWide(const XWide<M> &o)
    {
        const uint64_t fill = (int64_t)o.l[M - 1] < 0 ? ~0ull : 0ull;
        XW_UNROLL for (int i = 0; i < N; ++i) l[i] = i < M ? o.l[i < M ? i : 0] : fill;
    }
    XW_HD bool neg() const { return (int64_t)l[N - 1] < 0; }
};

template <int N> struct XUWide {
    uint64_t l[N];
    XUWide() = default;
    XW_HD XUWide(int64_t x)
    {
        l[0] = (uint64_t)x;
        XW_UNROLL for (int i = 1; i < N; ++i) l[i] = x < 0 ? ~0ull : 0ull;
    }
    XW_HD explicit XUWide(const XWide<N> &o) { XW_UNROLL for (int i = 0; i < N; ++i) l[i] = o.l[i]; }
    XW_HD XWide<N> as_signed() const
    {
        XWide<N> r;
        XW_UNROLL for (int i = 0; i < N; ++i) r.l[i] = l[i];
        return r;
    }
};

// ---- limb loops, on plain arrays so that both types share them --------------------------------------
template <int N> XW_HD inline void xw_add_limbs(const uint64_t *a, const uint64_t *b, uint64_t *r)
{
    uint64_t c = 0;
    XW_UNROLL for (int i = 0; i < N; ++i) {
        const xw_u128 t = (xw_u128)a[i] + b[i] + c;
        r[i] = (uint64_t)t;
        c = (uint64_t)(t >> 64);
    }
}
// r = a - b; the borrow out of the top limb
template <int N> XW_HD inline uint64_t xw_sub_limbs(const uint64_t *a, const uint64_t *b, uint64_t *r)
{
    uint64_t c = 0;
    XW_UNROLL for (int i = 0; i < N; ++i) {
        const xw_u128 t = (xw_u128)a[i] - b[i] - c;
        r[i] = (uint64_t)t;
        c = (uint64_t)(t >> 64) & 1;
    }
    return c;
}
template <int N> XW_HD inline void xw_neg_limbs(const uint64_t *a, uint64_t *r)
{
    uint64_t c = 1;
    XW_UNROLL for (int i = 0; i < N; ++i) {
        const xw_u128 t = (xw_u128)(~a[i]) + c;
        r[i] = (uint64_t)t;
        c = (uint64_t)(t >> 64);
    }
}
template <int N> XW_HD inline bool xw_eq_limbs(const uint64_t *a, const uint64_t *b)
{
    uint64_t d = 0;
    XW_UNROLL for (int i = 0; i < N; ++i) d |= a[i] ^ b[i];
    return d == 0;
}
// unsigned a < b
template <int N> XW_HD inline bool xw_ult_limbs(const uint64_t *a, const uint64_t *b)
{
    uint64_t t[N];
    return xw_sub_limbs<N>(a, b, t) != 0;
}
// the low R limbs of the unsigned product a (N limbs) * b (N limbs), R <= 2 N: operand scanning; one step's
// a_i * b_j + r_(i+j) + carry is at most 2^128 - 1
template <int N, int R> XW_HD inline void xw_mul_limbs(const uint64_t *a, const uint64_t *b, uint64_t *r)
{
    XW_UNROLL for (int i = 0; i < R; ++i) r[i] = 0;
    XW_UNROLL for (int i = 0; i < N; ++i) {
        uint64_t c = 0;
        XW_UNROLL for (int j = 0; j < N; ++j) {
            if (i + j < R) {
                const xw_u128 t = (xw_u128)a[i] * b[j] + r[i + j] + c;
                r[i + j] = (uint64_t)t;
                c = (uint64_t)(t >> 64);
            }
        }
        if (i + N < R) r[i + N] = c;
    }
}
// x >> s (0 <= s < 64 N), `fill` shifted in: by limbs under the bits 64, 128, ... of s, then by bits
template <int N> XW_HD inline void xw_shr_limbs(uint64_t *x, int s, uint64_t fill)
{
    XW_UNROLL for (int k = 1; k < N; k <<= 1) {
        if (s & (64 * k)) {
            XW_UNROLL for (int i = 0; i < N; ++i) x[i] = i + k < N ? x[i + k < N ? i + k : 0] : fill;
        }
    }
    const int b = s & 63;
    if (b) {
        XW_UNROLL for (int i = 0; i < N; ++i) x[i] = (x[i] >> b) | ((i + 1 < N ? x[i + 1 < N ? i + 1 : 0] : fill) << (64 - b));
    }
}
// trailing zero bits; 64 N for zero
template <int N> XW_HD inline int xw_ctz_limbs(const uint64_t *x)
{
    int n = 64 * N;
    XW_UNROLL for (int i = N - 1; i >= 0; --i)
        if (x[i]) n = 64 * i + __builtin_ctzll(x[i]);
    return n;
}

// ---- XWide ------------------------------------------------------------------------------------------------
template <int N> XW_HD inline XWide<N> operator-(const XWide<N> &a) { XWide<N> r; xw_neg_limbs<N>(a.l, r.l); return r; }
template <int N> XW_HD inline XWide<N> operator+(const XWide<N> &a, const XWide<N> &b) { XWide<N> r; xw_add_limbs<N>(a.l, b.l, r.l); return r; }
template <int N> XW_HD inline XWide<N> operator-(const XWide<N> &a, const XWide<N> &b) { XWide<N> r; (void)xw_sub_limbs<N>(a.l, b.l, r.l); return r; }
template <int N> XW_HD inline bool xw_eq(const XWide<N> &a, const XWide<N> &b) { return xw_eq_limbs<N>(a.l, b.l); }
// signed a < b: on bit patterns with the sign bit flipped the order is the unsigned one
template <int N> XW_HD inline bool xw_lt(const XWide<N> &a, const XWide<N> &b)
{
    XWide<N> x = a, y = b;
    x.l[N - 1] ^= 1ull << 63;
    y.l[N - 1] ^= 1ull << 63;
    return xw_ult_limbs<N>(x.l, y.l);
}
// the comparisons the rules of kernels_exact.inc make on the storage type (an int operand converts)
template <int N> XW_HD inline bool operator<(const XWide<N> &a, const XWide<N> &b) { return xw_lt(a, b); }
template <int N> XW_HD inline bool operator>(const XWide<N> &a, const XWide<N> &b) { return xw_lt(b, a); }
template <int N> XW_HD inline bool operator==(const XWide<N> &a, const XWide<N> &b) { return xw_eq(a, b); }
template <int N> XW_HD inline bool operator!=(const XWide<N> &a, const XWide<N> &b) { return !xw_eq(a, b); }
template <int N> XW_HD inline bool operator<(const XWide<N> &a, int b) { return b == 0 ? a.neg() : xw_lt(a, XWide<N>((int64_t)b)); }
template <int N> XW_HD inline bool operator>(const XWide<N> &a, int b) { return xw_lt(XWide<N>((int64_t)b), a); }
template <int N> XW_HD inline bool operator==(const XWide<N> &a, int b) { return xw_eq(a, XWide<N>((int64_t)b)); }
template <int N> XW_HD inline bool operator!=(const XWide<N> &a, int b) { return !xw_eq(a, XWide<N>((int64_t)b)); }

// -2^(64 N - 1): the one value outside the symmetric range
template <int N> XW_HD inline bool xw_is_min(const XWide<N> &x)
{
    uint64_t d = x.l[N - 1] ^ (1ull << 63);
    XW_UNROLL for (int i = 0; i < N - 1; ++i) d |= x.l[i];
    return d == 0;
}
// the signed product at double width: the unsigned product of the bit patterns, then
// a_s b_s = a_u b_u - 2^(64 N) ([a < 0] b_u + [b < 0] a_u) modulo 2^(128 N)
template <int N> XW_HD inline XWide<2 * N> xw_mul(const XWide<N> &a, const XWide<N> &b)
{
    XWide<2 * N> r;
    xw_mul_limbs<N, 2 * N>(a.l, b.l, r.l);
    uint64_t z[N];
    XW_UNROLL for (int i = 0; i < N; ++i) z[i] = (a.neg() ? b.l[i] : 0) ;
    (void)xw_sub_limbs<N>(r.l + N, z, r.l + N);
    XW_UNROLL for (int i = 0; i < N; ++i) z[i] = (b.neg() ? a.l[i] : 0);
    (void)xw_sub_limbs<N>(r.l + N, z, r.l + N);
    return r;
}
// acc -= b; false when the difference left the width (acc then holds it modulo 2^(64 N))
template <int N> XW_HD inline bool xw_sub_ovf(XWide<N> &acc, const XWide<N> &b)
{
    const XWide<N> r = acc - b;
    const bool ovf = (acc.neg() != b.neg()) && (r.neg() != acc.neg());
    acc = r;
    return !ovf;
}
// x as a value of half the limbs: false when it does not fit two's complement there
template <int N> XW_HD inline bool xw_narrow(const XWide<2 * N> &x, XWide<N> *out)
{
    const uint64_t fill = (int64_t)x.l[N - 1] < 0 ? ~0ull : 0ull;
    uint64_t d = 0;
    XW_UNROLL for (int i = N; i < 2 * N; ++i) d |= x.l[i] ^ fill;
    if (d) return false;
    XW_UNROLL for (int i = 0; i < N; ++i) out->l[i] = x.l[i];
    return true;
}
// ... inside the symmetric range (-2^(64 N - 1) is refused; *out is written only on success)
template <int N> XW_HD inline bool xw_fit(const XWide<2 * N> &x, XWide<N> *out)
{
    XWide<N> y;
    if (!xw_narrow<N>(x, &y) || xw_is_min(y)) return false;
    *out = y;
    return true;
}
// arithmetic x >> s, 0 <= s < 64 N
template <int N> XW_HD inline XWide<N> xw_sar(XWide<N> x, int s)
{
    xw_shr_limbs<N>(x.l, s, x.neg() ? ~0ull : 0ull);
    return x;
}

// ---- XUWide: modulo 2^(64 N) --------------------------------------------------------------------------
template <int N> XW_HD inline XUWide<N> operator*(const XUWide<N> &a, const XUWide<N> &b) { XUWide<N> r; xw_mul_limbs<N, N>(a.l, b.l, r.l); return r; }
template <int N> XW_HD inline XUWide<N> operator-(const XUWide<N> &a, const XUWide<N> &b) { XUWide<N> r; (void)xw_sub_limbs<N>(a.l, b.l, r.l); return r; }
template <int N> XW_HD inline XUWide<N> &operator*=(XUWide<N> &a, const XUWide<N> &b) { a = a * b; return a; }
template <int N> XW_HD inline int xw_ctz(const XUWide<N> &x) { return xw_ctz_limbs<N>(x.l); }
template <int N> XW_HD inline XUWide<N> xw_shr(XUWide<N> x, int s) { xw_shr_limbs<N>(x.l, s, 0); return x; }

// |n| mod d by shift and subtract, one bit of n per step from the top (the dividend moves left by one bit, so
// no bit is picked by a run-time index): |n| < 2^(128 N - 1), 0 < d < 2^(64 N - 1)
template <int N> XW_HD inline XUWide<N> xw_rem(XWide<2 * N> n, const XUWide<N> &d)
{
    if (n.neg()) n = -n;
    XUWide<N> r(0);
    XW_NOUNROLL for (int b = 0; b < 128 * N; ++b) {
        const uint64_t top = n.l[2 * N - 1] >> 63;
        XW_UNROLL for (int i = 2 * N - 1; i > 0; --i) n.l[i] = (n.l[i] << 1) | (n.l[i - 1] >> 63);
        n.l[0] <<= 1;
        XW_UNROLL for (int i = N - 1; i > 0; --i) r.l[i] = (r.l[i] << 1) | (r.l[i - 1] >> 63);
        r.l[0] = (r.l[0] << 1) | top;
        if (!xw_ult_limbs<N>(r.l, d.l)) (void)xw_sub_limbs<N>(r.l, d.l, r.l);
    }
    return r;
}

// ---- host only: what crosses the boundary is int64_t, so the host divides by 64-bit values only -------------
// a * b; false when the product does not fit N limbs (-2^(64 N - 1) does fit: the caller's range test refuses it)
template <int N> inline bool xw_mul_ovf(const XWide<N> &a, const XWide<N> &b, XWide<N> *r)
{
    return xw_narrow<N>(xw_mul(a, b), r);
}
// the quotient of a / d truncated towards zero and its remainder (the sign of a), d > 0: C's / and %
template <int N> inline XWide<N> xw_divmod_small(const XWide<N> &a, int64_t d, int64_t *rem)
{
    const bool neg = a.neg();
    const XWide<N> m = neg ? -a : a;                         // (-2^(64 N - 1) keeps its pattern: 2^(64 N - 1) unsigned)
    XWide<N> q;
    uint64_t r = 0;
    for (int i = N - 1; i >= 0; --i) {
        const xw_u128 cur = ((xw_u128)r << 64) | m.l[i];
        q.l[i] = (uint64_t)(cur / (uint64_t)d);
        r = (uint64_t)(cur % (uint64_t)d);
    }
    if (rem) *rem = neg ? -(int64_t)r : (int64_t)r;
    return neg ? -q : q;
}
// lcm(a, b) of positive values: a / gcd(a mod b, b) * b; false when it leaves the symmetric range
template <int N> inline bool xw_lcm_small(const XWide<N> &a, int64_t b, XWide<N> *r)
{
    int64_t x = 0, y = b;
    (void)xw_divmod_small(a, b, &x);
    while (x) { const int64_t t = y % x; y = x; x = t; }     // y = gcd(a mod b, b)
    return xw_mul_ovf(xw_divmod_small(a, y, nullptr), XWide<N>(b), r) && !xw_is_min(*r);
}

}  // namespace mi355x
