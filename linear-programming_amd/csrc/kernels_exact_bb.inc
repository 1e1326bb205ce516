// kernels_exact_bb.inc -- exact branch-and-bound: node tableaux assembled as integers straight into the
// members' slots of a batch of exact tableaux, and the light read-back of a solved batch.
// Part of simplex_kernels.hip (ONE translation unit: included there after kernels_exact_batch.inc; the
// arithmetic -- xmul, xsub, xsub_ovf, xfit -- is kernels_exact.inc's, nothing of it is repeated here).
//
//   k_xbb_assemble<T>  one workgroup per node of a group (same depth d, same number of artificial rows):
//                      the exact counterpart of k_bb_rows + k_assemble + k_art_objective.  Rows,
//                      columns, bases and the order in which artificial columns are dealt are those of the
//                      header of kernels_bb.inc (src/simplex.lisp:146, 198-202, 243-265, 292-325).  The base
//                      problem's general-form tableau comes as integers B = Db * b with ONE denominator Db,
//                      offsets as off_v = Db * offset_v; a node row `var <= / >= bound` at that scale is
//                        rhs = bound * Db - off_v  (no offset for a free variable),
//                      negated whole, sense flipped, when rhs < 0; slack and structural entries +-Db.
//                      Integers have no -0, so the inserted columns of base rows are plain 0.  The member's
//                      control block holds D = Db already (the host writes it); a value that leaves the
//                      symmetric range of the width sets its status to kXOverflow, nothing else.
//   k_xbb_readback<T>  per member: D, the right-hand-side column, the objective row (as (lo, hi) limbs)
//                      and the basis, gathered into one buffer -- all that tableau-objective-value,
//                      tableau-variable and tableau-reduced-cost read (src/simplex.lisp:74-120).

// node row k of member q: false when its right-hand side leaves the width (rhs is 0 then)
template <class T> __device__ __forceinline__ bool xbb_node_row(const XbbBaseView &b, const XbbNodeRows &nr, int64_t q, int64_t k,
                                                                int &kind, int64_t &col, T &rhs, bool &flip, int &op)
{
    const int64_t i = q * nr.d + k;
    const int64_t v = nr.var[i];
    kind = b.kind[v]; col = b.vcol[v];
    auto wide = xmul((T)nr.bound[i], (T)b.Db);
    if (kind != 2) wide = xsub(wide, xmul(((const T *)b.voff)[v], (T)1));      // coef 1, :230-237
    rhs = 0;
    const bool fits = xfit(wide, &rhs);
    flip = rhs < 0;
    op = row_word(flip, nr.sense[i]) >> 1;
    return fits;
}

// entry (R, C) of member q's main tableau
template <class T> __device__ __forceinline__ T xbb_main_elem(const XbbBaseView &b, const XbbNodeRows &nr, int64_t q, int64_t R, int64_t C)
{
    const int64_t d = nr.d, nb = b.nb, ncv = b.ncv, last = b.cols + d - 1;
    const T Db = (T)b.Db;
    if (R >= nb && R < nb + d) {
        const int64_t k = R - nb;
        int kind, op; int64_t col; T rhs; bool flip;
        xbb_node_row<T>(b, nr, q, k, kind, col, rhs, flip, op);
        T x = 0;
        if (C == last) x = rhs;
        else if (C == col) x = kind == 1 ? -Db : Db;
        else if (kind == 2 && C == col + 1) x = -Db;
        if (flip) x = -x;
        if (C == ncv + nb + k) x = op == 0 ? Db : -Db;
        return x;
    }
    const int64_t r = R < nb ? R : R - d;                                  // base row (rows_b - 1: objective)
    const T *row = (const T *)b.B + r * b.cols;
    if (C == last) return row[b.cols - 1];
    if (C < ncv + nb) return row[C];
    if (C < ncv + nb + d) return 0;
    return row[C - d];
}

// Members q0 + blockIdx.x.  mt.T / at.T == nullptr: that tableau is not written.  Dynamic LDS: one int32 per
// constraint row (its artificial-basis entry: deal_artificial_columns and ab_artificial of simplex_kernels.h).
template <class T> __global__ __launch_bounds__(kXThreads) void k_xbb_assemble(XbView mt, XbView at, XbbBaseView b, XbbNodeRows nr, int64_t q0)
{
    extern __shared__ __int128 xb_lds[];
    __shared__ int s_err;
    const int tid = threadIdx.x;
    const int64_t q = q0 + blockIdx.x;
    const int64_t d = nr.d, nb = b.nb, ncv = b.ncv;
    const int m = (int)(b.rows - 1 + d), num_cols = (int)(b.cols + d);
    int32_t *ab = (int32_t *)xb_lds;
    if (tid == 0) s_err = 0;
    int err = 0;
    for (int R = tid; R < m; R += kXThreads) {
        int64_t bas;
        if (R >= nb && R < nb + d) {
            int kind, op; int64_t col; T rhs; bool flip;
            if (!xbb_node_row<T>(b, nr, q, R - nb, kind, col, rhs, flip, op)) err = kXOverflow;
            bas = op == 0 ? ncv + R : num_cols;
        } else {
            const int64_t bb = b.basis[R < nb ? R : R - d];
            bas = bb == b.cols ? num_cols : (bb >= ncv + nb ? bb + d : bb);
        }
        ab[R] = (int32_t)bas;
    }
    __syncthreads();
    if (tid == 0) deal_artificial_columns(ab, m, num_cols);
    __syncthreads();
    if (mt.T) {
        T *M = (T *)mt.T + q * (int64_t)(m + 1) * num_cols;
        int64_t *mb = mt.basis + q * m;
        for (int R = tid; R < m; R += kXThreads) mb[R] = ab_main_basis(ab[R], num_cols);
        for (int k = tid; k < (m + 1) * num_cols; k += kXThreads) {
            const int R = k / num_cols;
            M[k] = xbb_main_elem<T>(b, nr, q, R, k - R * num_cols);
        }
    }
    if (at.T) {
        const int nac = (int)at.cols;
        const T Db = (T)b.Db;
        T *A = (T *)at.T + q * (int64_t)(m + 1) * nac;
        int64_t *abasis = at.basis + q * m;
        for (int R = tid; R < m; R += kXThreads) abasis[R] = ab[R];
        for (int k = tid; k < m * nac; k += kXThreads) {
            const int R = k / nac, C = k - R * nac;
            T x = 0;
            if (C < num_cols - 1) x = xbb_main_elem<T>(b, nr, q, R, C);
            else if (C == nac - 1) x = xbb_main_elem<T>(b, nr, q, R, num_cols - 1);
            else if (ab[R] == C) x = Db;
            A[k] = x;
        }
        __syncthreads();
        // the artificial objective row (:302-316): the sum of the artificial rows, every addition checked
        for (int C = tid; C < nac; C += kXThreads) {
            auto acc = xmul((T)0, (T)0);
            bool ok = true;
            if (C < num_cols - 1 || C == nac - 1)
                for (int R = 0; R < m; ++R)
                    if (ab_artificial(ab[R], num_cols)) ok = xsub_ovf(acc, xmul(A[(int64_t)R * nac + C], (T)-1)) && ok;
            T s = 0;
            if (!ok || !xfit(acc, &s)) { err = kXOverflow; s = 0; }
            A[(int64_t)m * nac + C] = s;
        }
    }
    if (err) atomicMax(&s_err, err);
    __syncthreads();
    if (tid == 0 && s_err) {
        if (mt.T) mt.ctl[q].status = s_err;
        if (at.T) at.ctl[q].status = s_err;
    }
}

// Member blockIdx.x, when it runs in this view's width (width[q] == v.bits): values + q * 2 * (1 + rows + cols)
// receives D, column cols - 1 (rows values) and row rows - 1 (cols values) as (lo, hi) limbs; basis + q * (rows - 1)
// its basis.
template <class T> __global__ __launch_bounds__(kXThreads) void k_xbb_readback(XbView v, const int32_t *width, int64_t *values, int64_t *basis)
{
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    if (width[q] != v.bits) return;
    const int64_t R = v.rows, C = v.cols, m = R - 1;
    const T *M = (const T *)v.T + q * R * C;
    int64_t *out = values + q * 2 * (1 + R + C);
    auto put = [&](int64_t k, __int128 x) {
        out[2 * k] = (int64_t)(uint64_t)(xu128)x;
        out[2 * k + 1] = (int64_t)(x >> 64);
    };
    if (tid == 0) put(0, v.ctl[q].D);
    for (int64_t i = tid; i < R; i += kXThreads) put(1 + i, M[i * C + C - 1]);
    for (int64_t j = tid; j < C; j += kXThreads) put(1 + R + j, M[m * C + j]);
    for (int64_t i = tid; i < m; i += kXThreads) basis[q * m + i] = v.basis[q * m + i];
}

void launch_xbb_assemble(const XbView &mt, const XbView &at, const XbbBaseView &b, const XbbNodeRows &nr, int64_t q0,
                         int64_t count, hipStream_t s)
{
    const int bits = mt.T ? mt.bits : at.bits;
    const size_t lds = ((size_t)(b.rows - 1 + nr.d) * sizeof(int32_t) + 15) & ~(size_t)15;
    x_with_width(bits, [&](auto t) {
        hipLaunchKernelGGL(k_xbb_assemble<decltype(t)>, dim3((unsigned)count), dim3(kXThreads), lds, s, mt, at, b, nr, q0);
    });
}
void launch_xbb_readback(const XbView &v, const int32_t *width, int64_t *values, int64_t *basis, hipStream_t s)
{
    x_with_width(v.bits, [&](auto t) {
        hipLaunchKernelGGL(k_xbb_readback<decltype(t)>, dim3((unsigned)v.n), dim3(kXThreads), 0, s, v, width, values, basis);
    });
}
