// kernels_exact_lps.inc -- build-tableau on the device for batches of exact rational LPs: the members'
// start states assembled as integers from their problem rows, straight into their slots of a batch of
// exact tableaux.  Part of simplex_kernels.hip (ONE translation unit: included there after
// kernels_exact_bb.inc; the arithmetic -- xmul, xsub_ovf, xfit, xinv_odd, xctz -- is kernels_exact.inc's,
// nothing of it is repeated here).
//
//   k_xb_assemble_lps<T>  one workgroup per member of a group (same m, ncv, number of `=` rows and number of
//                      artificial rows).  The member comes in column space, as build-tableau holds it after
//                      src/simplex.lisp:189-241 and before :243: m rows of ncv structural coefficients and the
//                      right-hand side, then the objective row as :270-283 stores it, every entry a reduced
//                      fraction num / den.  What is written is what build-tableau (:243-328) followed by
//                      x_start_state (capi_exact.inc) gives, entry for entry:
//                        a row whose right-hand side is < 0 is negated whole, its sense flipped (:243-252);
//                        slack columns go in row order to the rows that are not `=`: +1 and basic under `<=`,
//                        -1 under `>=` (:254-265); artificial columns go in decreasing row order to the `>=`
//                        and `=` rows (:257, :261, :296-300); the artificial objective row is the sum of the
//                        artificial rows over the structural and slack columns and the right-hand side
//                        (:302-316).
//                      The integer scale: L_i = LCM of row i's denominators, P = prod_{i<m} L_i.  The main
//                      tableau has D = P * L_m with L_m the LCM of the given objective row.  The artificial
//                      objective row at scale P is integral -- the column sums S_c -- so the LCM of the
//                      denominators of its reduced entries is P / g, g = gcd(P, S_0, S_1, ...), and the
//                      artificial tableau has D = P * (P / g).  A slack column's sum is 0 or -P and changes
//                      nothing in g.  Every entry is (D / den) * num; den | L_i | D, so the division is exact
//                      and is a multiplication by the inverse of den's odd part modulo 2^W.
//                      Overflow.  Every intermediate divides or is bounded by a value that is stored: a
//                      partial LCM or product divides D, |S_c| <= |S_c * (P / g)|, and the sums are
//                      accumulated at double width.  So a tableau's status becomes kXOverflow exactly when
//                      its D or one of its entries leaves the symmetric range of the width -- where
//                      x_start_state reports it -- and nothing of that tableau is to be used then.  The two
//                      tableaux of a member are judged each on its own, as two handles made from the host's
//                      rationals are.  The control block receives D; its status is left as the host wrote it
//                      otherwise.

// a / d for d > 0 that divides a >= 0
template <class T> __device__ __forceinline__ T xl_quot(T a, T d)
{
    typedef typename XUnsigned<T>::type U;
    if (d == 1) return a;
    const int sh = xctz((xu128)d);
    return (T)((U)(a >> sh) * xinv_odd<U>((U)(d >> sh)));
}

// binary gcd; gcd(0, b) = b
template <class U> __device__ inline U xl_gcd(U a, U b)
{
    if (a == 0) return b;
    if (b == 0) return a;
    const int sa = xctz((xu128)a), sb = xctz((xu128)b);
    a >>= sa; b >>= sb;
    while (a != b) {
        if (a > b) { a -= b; a >>= xctz((xu128)a); }
        else       { b -= a; b >>= xctz((xu128)b); }
    }
    return a << (sa < sb ? sa : sb);
}

// l = lcm(l, d) for l > 0, d > 0: false when it leaves the width
template <class T> __device__ inline bool xl_lcm(T &l, int64_t d)
{
    typedef typename XUnsigned<T>::type U;
    if (d == 1) return true;
    const T g = (T)xl_gcd<U>((U)l, (U)(uint64_t)d);
    return xfit(xmul(xl_quot<T>(l, g), (T)d), &l);
}

// input entry i at scale D, negated for a flipped row: false when it leaves the width (0 is stored then)
template <class T> __device__ __forceinline__ bool xl_entry(const XbLpsView &sp, int64_t i, T D, bool neg, T *out)
{
    const int64_t n = sp.num[i];
    *out = 0;
    if (n == 0) return true;
    const T cq = xl_quot<T>(D, (T)sp.den[i]);
    return xfit(xmul(neg ? -cq : cq, (T)n), out);
}

// Members q0 + blockIdx.x.  mt.T / at.T == nullptr: that tableau is not written.  Dynamic LDS: three int32 per
// constraint row -- fl (bit 0: the row is negated; bits 1-2: its sense after that), sc (its slack column, -1
// for `=`) and ab (its artificial-basis entry: row_word, deal_artificial_columns and ab_artificial of simplex_kernels.h).
template <class T> __global__ __launch_bounds__(kXThreads) void k_xb_assemble_lps(XbView mt, XbView at, XbLpsView sp, int64_t q0)
{
    typedef typename XUnsigned<T>::type U;
    extern __shared__ __int128 xb_lds[];
    __shared__ T red[kXThreads];
    __shared__ T s_lm;
    __shared__ int s_err_p, s_err_m, s_err_a;
    const int tid = threadIdx.x;
    const int64_t q = q0 + blockIdx.x;
    const int m = (int)sp.m, ncv = (int)sp.ncv, W = ncv + 1;
    const int num_cols = ncv + (int)sp.n_slack + 1, nac = num_cols + (int)sp.n_art;
    const int64_t in0 = q * (int64_t)(m + 1) * W;                            // the member's first input entry
    int32_t *fl = (int32_t *)xb_lds, *sc = fl + m, *ab = sc + m;
    if (tid == 0) { s_err_p = s_err_m = s_err_a = 0; s_lm = 1; }
    __syncthreads();

    // the rows' LCMs (the product of this thread's in part), flips and senses
    T part = 1;
    bool ok_p = true;
    for (int R = tid; R <= m; R += kXThreads) {
        const int64_t i0 = in0 + (int64_t)R * W;
        T l = 1;
        bool ok = true;
        for (int c = 0; c < W && ok; ++c) ok = xl_lcm<T>(l, sp.den[i0 + c]);
        if (R == m) {
            if (ok) s_lm = l; else s_err_m = kXOverflow;
            continue;
        }
        ok_p = ok_p && ok && xfit(xmul(part, l), &part);
        fl[R] = row_word(sp.num[i0 + ncv] < 0, sp.sense[q * m + R]);
    }
    red[tid] = ok_p ? part : (T)1;
    if (!ok_p) s_err_p = kXOverflow;
    __syncthreads();
    if (tid == 0) {
        int32_t ns = 0;
        for (int R = 0; R < m; ++R) {                                        // slack columns in row order, :254-265
            const int op = fl[R] >> 1;
            sc[R] = op == 2 ? -1 : ncv + ns++;
            ab[R] = op == 0 ? sc[R] : num_cols;
        }
        deal_artificial_columns(ab, m, num_cols);
    }
    for (int s = kXThreads / 2; s > 0; s >>= 1) {                            // P = prod L_i
        if (tid < s && !xfit(xmul(red[tid], red[tid + s]), &red[tid])) { red[tid] = 1; s_err_p = kXOverflow; }
        __syncthreads();
    }
    const T P = red[0], Lm = s_lm;
    const bool p_ok = s_err_p == 0, lm_ok = s_err_m == 0;
    __syncthreads();                                                        // (red is free again)
    if (!p_ok) {
        if (tid == 0) {
            if (mt.T) mt.ctl[q].status = kXOverflow;
            if (at.T) at.ctl[q].status = kXOverflow;
        }
        return;
    }

    if (mt.T) {
        T D = 0;
        const bool d_ok = lm_ok && xfit(xmul(P, Lm), &D);
        int err = d_ok ? 0 : kXOverflow;
        if (d_ok) {
            T *M = (T *)mt.T + q * (int64_t)(m + 1) * num_cols;
            int64_t *mb = mt.basis + q * m;
            for (int R = tid; R < m; R += kXThreads) mb[R] = ab_main_basis(ab[R], num_cols);
            for (int k = tid; k < (m + 1) * num_cols; k += kXThreads) {
                const int R = k / num_cols, C = k - R * num_cols;
                const bool neg = R < m && (fl[R] & 1);
                T x = 0;
                if (C < ncv || C == num_cols - 1) {
                    if (!xl_entry<T>(sp, in0 + (int64_t)R * W + (C < ncv ? C : ncv), D, neg, &x)) err = kXOverflow;
                } else if (R < m && C == sc[R]) {
                    x = (fl[R] >> 1) == 0 ? D : -D;
                }
                M[k] = x;
            }
        }
        if (err) atomicMax(&s_err_m, err);
        else if (tid == 0) mt.ctl[q].D = D;
    }

    if (at.T) {
        T *A = (T *)at.T + q * (int64_t)(m + 1) * nac;
        T *last = A + (int64_t)m * nac;
        int err = 0;
        // S_c at scale P into the objective row's slots, and the gcd of this thread's
        U g = 0;
        for (int C = tid; C < nac; C += kXThreads) {
            if (C >= ncv && C != nac - 1) continue;
            const int c = C < ncv ? C : ncv;
            auto acc = xmul((T)0, (T)0);
            bool ok = true;
            for (int R = 0; R < m; ++R) {
                if (!ab_artificial(ab[R], num_cols)) continue;
                const int64_t i = in0 + (int64_t)R * W + c;
                const int64_t n = sp.num[i];
                if (n == 0) continue;
                const T cq = xl_quot<T>(P, (T)sp.den[i]);
                ok = xsub_ovf(acc, xmul((fl[R] & 1) ? cq : -cq, (T)n)) && ok;
            }
            T S = 0;
            if (!ok || !xfit(acc, &S)) { err = kXOverflow; S = 0; }
            last[C] = S;
            g = xl_gcd<U>(g, (U)(S < 0 ? -S : S));
        }
        red[tid] = (T)g;
        if (err) atomicMax(&s_err_a, err);
        __syncthreads();
        for (int s = kXThreads / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] = (T)xl_gcd<U>((U)red[tid], (U)red[tid + s]);
            __syncthreads();
        }
        const T gs = red[0];
        const bool s_ok = s_err_a == 0;
        __syncthreads();                                                    // (every thread has read both)
        const T La = xl_quot<T>(P, (T)xl_gcd<U>((U)P, (U)gs));               // P / gcd(P, S_0, S_1, ...)
        T D = 0;
        const bool d_ok = s_ok && xfit(xmul(P, La), &D);
        err = d_ok ? 0 : kXOverflow;
        if (d_ok) {
            int64_t *abasis = at.basis + q * m;
            for (int R = tid; R < m; R += kXThreads) abasis[R] = ab[R];
            for (int k = tid; k < m * nac; k += kXThreads) {
                const int R = k / nac, C = k - R * nac;
                T x = 0;
                if (C < ncv || C == nac - 1) {
                    if (!xl_entry<T>(sp, in0 + (int64_t)R * W + (C < ncv ? C : ncv), D, (fl[R] & 1) != 0, &x)) err = kXOverflow;
                } else if (C < num_cols - 1) {
                    if (C == sc[R]) x = (fl[R] >> 1) == 0 ? D : -D;
                } else if (C == ab[R]) {
                    x = D;
                }
                A[k] = x;
            }
            // the artificial objective row (:302-316): S_c * (P / g); a `>=` row's slack column sums to -D
            for (int C = tid; C < nac; C += kXThreads) {
                T x = 0;
                if ((C < ncv || C == nac - 1) && !xfit(xmul(last[C], La), &x)) { err = kXOverflow; x = 0; }
                last[C] = x;
            }
            __syncthreads();
            for (int R = tid; R < m; R += kXThreads)
                if ((fl[R] >> 1) == 1 && sc[R] >= ncv && sc[R] < num_cols - 1) last[sc[R]] = -D;
        }
        if (err) atomicMax(&s_err_a, err);
        else if (tid == 0) at.ctl[q].D = D;
    }
    __syncthreads();
    if (tid == 0) {
        if (mt.T && s_err_m) mt.ctl[q].status = kXOverflow;
        if (at.T && s_err_a) at.ctl[q].status = kXOverflow;
    }
}

size_t xb_assemble_lps_lds(int64_t m) { return ((size_t)m * 3 * sizeof(int32_t) + 15) & ~(size_t)15; }

void launch_xb_assemble_lps(const XbView &mt, const XbView &at, const XbLpsView &sp, int64_t q0, int64_t count, hipStream_t s)
{
    const int bits = mt.T ? mt.bits : at.bits;
    x_with_width(bits, [&](auto t) {
        hipLaunchKernelGGL(k_xb_assemble_lps<decltype(t)>, dim3((unsigned)count), dim3(kXThreads), xb_assemble_lps_lds(sp.m), s,
                           mt, at, sp, q0);
    });
}
