// kernels_single.inc -- SINGLE-FLOAT tableaux: the reference's single-float path (src/utils.lisp:84-124
// with single-float-epsilon, src/simplex.lisp:337-461) in IEEE binary32 throughout.  No double appears
// in this file: keys, quotients, thresholds, products and differences are floats, a product is rounded,
// then the difference is rounded (-ffp-contract=off), division is true division.
// Part of simplex_kernels.hip (ONE translation unit: included there, in this order, inside namespace mi355x).
//
// ONE copy of the selection code -- s_block_price, s_block_gather_ratio, s_block_scale_row, the float
// versions of block_price / block_gather_ratio / block_scale_row without the compact-representation
// branches -- and two solve forms that are loops around it:
//     k_s_select + k_s_update   any size: the tableau in HBM, two launches per pivot
//     k_s_solve                 small tableaux: tableau, column snapshot and pivot row in LDS, the whole
//                               n-solve-tableau loop in one launch of one 1024-thread workgroup (s_solve_in_lds,
//                               the loop that k_sb_solve of kernels_single_batch.inc runs once per member)
// The functions take plain pointers: called on HBM rows by the pair, on LDS rows by k_s_solve.

// ------------------------------------------------------------------ candidates and reductions
struct SCand {
    float    v;
    int      i;           // < 0 : empty
    unsigned s;           // payload that travels with the winner (never compared): 1 = the NaN in column 0 of a
                          // pricing candidate / the bit pattern of the pivot element of a ratio candidate
};
struct SScratch { float v[kSelWaves]; int i[kSelWaves]; unsigned s[kSelWaves]; };

// lexicographic (value, index) minimum; an empty slot loses against anything (vi_min's rules)
__device__ __forceinline__ SCand sc_min(SCand a, SCand b)
{
    const bool a_empty = a.i < 0, b_empty = b.i < 0;
    const bool better  = (b.v < a.v) | ((b.v == a.v) & (b.i < a.i));
    const bool take_b  = a_empty | (!b_empty & better);
    SCand r;
    r.v = take_b ? b.v : a.v;
    r.i = take_b ? b.i : a.i;
    r.s = take_b ? b.s : a.s;
    return r;
}
__device__ __forceinline__ SCand sc_empty() { SCand c; c.v = 0.0f; c.i = -1; c.s = 0u; return c; }

// price_cand's NaN rules: a NaN key is no candidate, except in column 0, where it is the unbeatable one
__device__ __forceinline__ SCand s_price_cand(float key, int column)
{
    SCand c; c.v = key; c.i = column; c.s = 0u;
    if (key != key) {
        if (column == 0) { c.v = -__builtin_inff(); c.s = 1u; }
        else             c.i = -1;
    }
    return c;
}
// (fp< v 0 factor/8) on the winner: nothing to enter <=> the tableau is optimal
__device__ __forceinline__ bool s_price_says_optimal(const SCand &e, float price_tol)
{
    return e.i < 0 || e.s == 1u || !(e.v < 0.0f - price_tol);
}

__device__ __forceinline__ SCand sc_wave_min(SCand x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {     // (a lane whose partner lies past the wave combines with itself)
        SCand y;
        y.v = __shfl_down(x.v, off, 64);
        y.i = __shfl_down(x.i, off, 64);
        y.s = (unsigned)__shfl_down((int)x.s, off, 64);
        x = sc_min(x, y);
    }
    return x;
}
// Block-wide lexicographic arg-min over THREADS threads; result valid in every thread.
template <int THREADS>
__device__ __forceinline__ SCand sc_block_min(SCand x, SScratch *sc)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = sc_wave_min(x);
    __syncthreads();                       // protects the scratch across calls
    if (lane == 0) { sc->v[wave] = x.v; sc->i[wave] = x.i; sc->s[wave] = x.s; }
    __syncthreads();
    SCand r; r.v = sc->v[0]; r.i = sc->i[0]; r.s = sc->s[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) {
        SCand y; y.v = sc->v[w]; y.i = sc->i[w]; y.s = sc->s[w];
        r = sc_min(r, y);
    }
    return r;
}

typedef float vec4f __attribute__((ext_vector_type(4)));    // one global_load/store_dwordx4, one ds_read/write_b128

// ------------------------------------------------------------------ the selection code (one copy)
// find-entering-column (src/simplex.lisp:362-379) over columns [0, ncols) of the objective row `obj` (16-byte
// aligned).  sgn = +1 max problems (arg-min), -1 min problems.  The lowest-index strict extremum in key space;
// the caller applies the threshold.  kBatch 16-byte loads in flight per thread.
template <int THREADS>
__device__ __forceinline__ SCand s_block_price(const float *__restrict__ obj, int ncols, float sgn, SScratch *sc)
{
    SCand best = sc_empty();
    const int nquad = ncols >> 2;
    const vec4f *obj4 = reinterpret_cast<const vec4f *>(obj);
    for (int base = 0; base < nquad; base += kBatch * THREADS) {
        vec4f v[kBatch];
#pragma unroll
        for (int g = 0; g < kBatch; ++g) {
            const int p = base + g * THREADS + (int)threadIdx.x;
            if (p < nquad) v[g] = obj4[p];
            else { v[g].x = 0.0f; v[g].y = 0.0f; v[g].z = 0.0f; v[g].w = 0.0f; }
        }
#pragma unroll
        for (int g = 0; g < kBatch; ++g) {
            const int p = base + g * THREADS + (int)threadIdx.x;
            if (p < nquad) {
                best = sc_min(best, s_price_cand(v[g].x * sgn, 4 * p));
                best = sc_min(best, s_price_cand(v[g].y * sgn, 4 * p + 1));
                best = sc_min(best, s_price_cand(v[g].z * sgn, 4 * p + 2));
                best = sc_min(best, s_price_cand(v[g].w * sgn, 4 * p + 3));
            }
        }
    }
    if ((int)threadIdx.x < (ncols & 3)) {           // the one to three columns behind the last whole quad
        const int c = 4 * nquad + (int)threadIdx.x;
        best = sc_min(best, s_price_cand(obj[c] * sgn, c));
    }
    return sc_block_min<THREADS>(best, sc);
}

// Gather the entering column of the rows x (vc + 1) tableau M (leading dimension ld), snapshot it into
// col_out[0 .. rows), and run find-pivoting-row (src/simplex.lisp:382-389): block_gather_ratio's rules --
// the lowest row of the strict minimum; a NaN quotient wins only as the FIRST eligible row.
template <int THREADS>
__device__ __forceinline__ SCand s_block_gather_ratio(const float *M, int64_t ld, int rows, int vc, int ec,
                                                      float *col_out, float ratio_thr, SScratch *sc)
{
    const int m = rows - 1;
    int nanq = 0;
    SCand best = sc_empty(), first = sc_empty();
    for (int base = 0; base < rows; base += kBatch * THREADS) {
        float a[kBatch], b[kBatch];
#pragma unroll
        for (int g = 0; g < kBatch; ++g) {           // the strided gathers: all in flight at once
            const int r = base + g * THREADS + (int)threadIdx.x;
            a[g] = r < rows ? M[(int64_t)r * ld + ec] : 0.0f;
            b[g] = r < m ? M[(int64_t)r * ld + vc] : 0.0f;
        }
#pragma unroll
        for (int g = 0; g < kBatch; ++g) {
            const int r = base + g * THREADS + (int)threadIdx.x;
            if (r < rows) col_out[r] = a[g];
            if (r < m && ratio_thr < a[g]) {         // (fp< 0 a factor/2) -> (< (+ 0 thr) a)
                const float q = b[g] / a[g];
                if (first.i < 0) { first.i = r; first.s = __float_as_uint(a[g]); }
                if (q != q) nanq = 1;                // no candidate (unless it is the FIRST eligible row: below)
                else if (best.i < 0 || q < best.v) { best.v = q; best.i = r; best.s = __float_as_uint(a[g]); }
            }
        }
    }
    best = sc_block_min<THREADS>(best, sc);
    if (__syncthreads_or(nanq)) {
        first = sc_block_min<THREADS>(first, sc);
        if (first.i >= 0) {
            const float a0 = __uint_as_float(first.s);
            const float q0 = M[(int64_t)first.i * ld + vc] / a0;
            if (q0 != q0) { best.v = q0; best.i = first.i; best.s = first.s; }
        }
    }
    return best;
}

// prow[c] = row[c] / row_scale (src/simplex.lisp:343-348) over the nquad quads of a row; columns >= cols
// (padding) are zero in the pivot row.
template <int THREADS>
__device__ __forceinline__ void s_block_scale_row(const float *row, float *prow, int nquad, int cols, float row_scale)
{
    const vec4f *src = reinterpret_cast<const vec4f *>(row);
    vec4f *dst = reinterpret_cast<vec4f *>(prow);
    for (int base = 0; base < nquad; base += kBatch * THREADS) {
        vec4f v[kBatch];
#pragma unroll
        for (int g = 0; g < kBatch; ++g) {
            const int p = base + g * THREADS + (int)threadIdx.x;
            if (p < nquad) v[g] = src[p];
            else { v[g].x = 0.0f; v[g].y = 0.0f; v[g].z = 0.0f; v[g].w = 0.0f; }
        }
#pragma unroll
        for (int g = 0; g < kBatch; ++g) {
            const int p = base + g * THREADS + (int)threadIdx.x;
            if (p < nquad) {
                vec4f o;
                o.x = (4 * p     < cols) ? v[g].x / row_scale : 0.0f;
                o.y = (4 * p + 1 < cols) ? v[g].y / row_scale : 0.0f;
                o.z = (4 * p + 2 < cols) ? v[g].z / row_scale : 0.0f;
                o.w = (4 * p + 3 < cols) ? v[g].w / row_scale : 0.0f;
                dst[p] = o;
            }
        }
    }
}

// the bookkeeping of one pivot (ONE thread), record_pivot's protocol on the shared Ctl
__device__ __forceinline__ void s_record_pivot(const SView &t, const Ctl &c0, int64_t ec, int64_t cr)
{
    Ctl *ctl = t.ctl;
    ctl->ec = ec;
    ctl->cr = cr;
    if (t.rows > 1) t.basis[cr] = ec;               // src/simplex.lisp:358
    if (t.trace_ec && c0.trace_n < t.trace_cap) {
        t.trace_ec[c0.trace_n] = ec;
        t.trace_cr[c0.trace_n] = cr;
    }
    ctl->trace_n  = c0.trace_n + 1;
    ctl->n_pivots = c0.n_pivots + 1;
}

// ------------------------------------------------------------------ the pair
// k_s_select: one workgroup.  Prices, does the ratio test, writes the column snapshot and the scaled pivot
// row, records the pivot; k_select's Ctl protocol (status, max_pivots, trace).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_s_select(SView t, float sgn, float price_tol, float ratio_thr)
{
    __shared__ SScratch sc;
    Ctl *ctl = t.ctl;
    const Ctl c0 = *ctl;                            // in flight together with the pricing inputs
    const int rows = (int)t.rows, vc = (int)t.cols - 1;
    const SCand e = s_block_price<THREADS>(t.M + (int64_t)(rows - 1) * t.ld, vc, sgn, &sc);
    if (c0.status != kRunning) return;
    if (s_price_says_optimal(e, price_tol)) {
        if (threadIdx.x == 0) ctl->status = 0;      // MI_OPTIMAL
        return;
    }
    if (c0.max_pivots > 0 && c0.n_pivots >= c0.max_pivots) {
        if (threadIdx.x == 0) ctl->status = 3;      // MI_MAX_PIVOTS
        return;
    }
    const SCand q = s_block_gather_ratio<THREADS>(t.M, t.ld, rows, vc, e.i, t.col, ratio_thr, &sc);
    if (q.i < 0) {
        if (threadIdx.x == 0) ctl->status = 1;      // MI_UNBOUNDED
        return;
    }
    s_block_scale_row<THREADS>(t.M + (int64_t)q.i * t.ld, t.prow, (int)(t.ld >> 2), (int)t.cols, __uint_as_float(q.s));
    if (threadIdx.x == 0) s_record_pivot(t, c0, e.i, q.i);
}

// find-entering-column only: ctl->ec = column or -1
__global__ __launch_bounds__(kSelThreads) void k_s_price_only(SView t, float sgn, float price_tol)
{
    __shared__ SScratch sc;
    const SCand e = s_block_price<kSelThreads>(t.M + (t.rows - 1) * t.ld, (int)t.cols - 1, sgn, &sc);
    if (threadIdx.x == 0) t.ctl->ec = s_price_says_optimal(e, price_tol) ? -1 : e.i;
}
// find-pivoting-row only (given ec): ctl->cr = row or -1.  Writes the column snapshot, not the tableau.
__global__ __launch_bounds__(kSelThreads) void k_s_ratio_only(SView t, int ec, float ratio_thr)
{
    __shared__ SScratch sc;
    const SCand q = s_block_gather_ratio<kSelThreads>(t.M, t.ld, (int)t.rows, (int)t.cols - 1, ec, t.col, ratio_thr, &sc);
    if (threadIdx.x == 0) t.ctl->cr = q.i;
}
// Forced pivot (n-pivot-row with caller-chosen ec, cr): snapshot column + scaled row; k_s_update follows.
__global__ __launch_bounds__(kSelThreads) void k_s_prepare_pivot(SView t, int ec, int cr)
{
    for (int r = threadIdx.x; r < (int)t.rows; r += kSelThreads)
        t.col[r] = t.M[(int64_t)r * t.ld + ec];
    s_block_scale_row<kSelThreads>(t.M + (int64_t)cr * t.ld, t.prow, (int)(t.ld >> 2), (int)t.cols, t.M[(int64_t)cr * t.ld + ec]);
    if (threadIdx.x == 0) {
        const Ctl c0 = *t.ctl;
        t.ctl->status = kRunning;
        s_record_pivot(t, c0, ec, cr);
    }
}

// k_s_update: the rank-1 update, k_update at twice the elements per access.  Tile = (strip_quads <= BLOCK
// 16-byte quads of FOUR columns) x (tr rows).  A lane owns one quad: its four pivot-row entries stay in VGPRs
// for the tile; per row one global_load_dwordx4, 4 v_mul_f32 + 4 v_sub_f32 (never fused) and one
// global_store_dwordx4.  U rows are in flight before the first use.  col[r] is uniform -> scalar loads.  The
// pivot row is written from prow.
template <int BLOCK, int U>
__global__ __launch_bounds__(BLOCK) void k_s_update(SView t, const int tr, const int strip_quads)
{
    float *__restrict__ M = t.M;
    const float *__restrict__ col  = t.col;
    const float *__restrict__ prow = t.prow;
    const Ctl *__restrict__ ctl = t.ctl;
    if (ctl->status != kRunning) return;
    const int64_t cr  = ctl->cr;
    const int64_t ldq = t.ld >> 2;                             // row length in 16-byte quads
    const int64_t quad = (int64_t)blockIdx.x * strip_quads + threadIdx.x;
    if ((int)threadIdx.x >= strip_quads || quad >= ldq) return;
    const int64_t r0 = (int64_t)blockIdx.y * tr;
    const int64_t r1 = (r0 + tr < t.rows) ? r0 + tr : t.rows;
    vec4f *Mp = reinterpret_cast<vec4f *>(M) + quad;
    const vec4f p = reinterpret_cast<const vec4f *>(prow)[quad];
    int64_t r = r0;
    for (; r + U <= r1; r += U) {
        vec4f v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = Mp[(r + u) * ldq];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float s = col[r + u];
            const float m0 = s * p.x, m1 = s * p.y, m2 = s * p.z, m3 = s * p.w;     // rounded products
            vec4f o;
            o.x = v[u].x - m0;                                 // rounded differences
            o.y = v[u].y - m1;
            o.z = v[u].z - m2;
            o.w = v[u].w - m3;
            if (r + u == cr) o = p;                            // the pivot row itself
            Mp[(r + u) * ldq] = o;
        }
    }
    for (; r < r1; ++r) {                                      // row tail of the tile
        const vec4f x = Mp[r * ldq];
        const float s = col[r];
        const float m0 = s * p.x, m1 = s * p.y, m2 = s * p.z, m3 = s * p.w;
        vec4f o;
        o.x = x.x - m0;
        o.y = x.y - m1;
        o.z = x.z - m2;
        o.w = x.w - m3;
        if (r == cr) o = p;
        Mp[r * ldq] = o;
    }
}

// ------------------------------------------------------------------ the LDS-resident solve
// One workgroup of THREADS threads runs n-solve-tableau (src/simplex.lisp:453-461) on a tableau it holds in LDS: rows x
// ldl floats (ldl = cols rounded up to a quad), then the pivot row (ldl), then the column snapshot (rows rounded up
// to a quad).  At most `cap` pivots per launch; max_pivots is honoured exactly (k_s_select's order of tests).
// On exit the tableau goes back to HBM, so a solve continued call by call makes the pivots of one long call.
template <int THREADS>
__device__ __forceinline__ void s_solve_in_lds(const SView &t, float sgn, float price_tol, float ratio_thr, int cap)
{
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    __shared__ SScratch sc;
    Ctl *ctl = t.ctl;
    const Ctl c0 = *ctl;
    if (c0.status != kRunning) return;
    const int rows = (int)t.rows, cols = (int)t.cols, vc = cols - 1;
    const int ldlq = (cols + 3) >> 2, ldl = 4 * ldlq;         // LDS row length in quads / floats
    const int64_t ldq = t.ld >> 2;
    float *L    = s_lds;
    float *prow = L + (size_t)rows * ldl;
    float *col  = prow + ldl;
    vec4f *L4 = reinterpret_cast<vec4f *>(L);
    vec4f *G4 = reinterpret_cast<vec4f *>(t.M);
    const int nq = rows * ldlq;                               // quads of the LDS tableau
    // thread's walk over the quads: (row, quad of the row) advances by THREADS quads per step
    const int step_r = THREADS / ldlq, step_q = THREADS % ldlq;
    {
        int r = (int)threadIdx.x / ldlq, qd = (int)threadIdx.x % ldlq;
        for (int idx = threadIdx.x; idx < nq; idx += THREADS) {
            L4[idx] = G4[(int64_t)r * ldq + qd];
            r += step_r; qd += step_q;
            if (qd >= ldlq) { qd -= ldlq; ++r; }
        }
    }
    __syncthreads();
    int32_t status = kRunning;
    int64_t n = c0.n_pivots, trace_n = c0.trace_n, last_ec = c0.ec, last_cr = c0.cr;
    for (int k = 0; ; ++k) {
        const SCand e = s_block_price<THREADS>(L + (size_t)(rows - 1) * ldl, vc, sgn, &sc);
        if (s_price_says_optimal(e, price_tol)) { status = 0; break; }                 // MI_OPTIMAL
        if (c0.max_pivots > 0 && n >= c0.max_pivots) { status = 3; break; }            // MI_MAX_PIVOTS
        if (k >= cap) break;                                   // the launch's bound: still running
        const SCand q = s_block_gather_ratio<THREADS>(L, ldl, rows, vc, e.i, col, ratio_thr, &sc);
        if (q.i < 0) { status = 1; break; }                    // MI_UNBOUNDED
        const int cr = q.i;
        s_block_scale_row<THREADS>(L + (size_t)cr * ldl, prow, ldlq, cols, __uint_as_float(q.s));
        __syncthreads();
        {
            const vec4f *P4 = reinterpret_cast<const vec4f *>(prow);
            int r = (int)threadIdx.x / ldlq, qd = (int)threadIdx.x % ldlq;
            for (int idx = threadIdx.x; idx < nq; idx += THREADS) {
                const vec4f p = P4[qd], v = L4[idx];
                const float s = col[r];
                const float m0 = s * p.x, m1 = s * p.y, m2 = s * p.z, m3 = s * p.w;     // rounded products
                vec4f o;
                o.x = v.x - m0;                                // rounded differences
                o.y = v.y - m1;
                o.z = v.z - m2;
                o.w = v.w - m3;
                if (r == cr) o = p;                            // the pivot row itself
                L4[idx] = o;
                r += step_r; qd += step_q;
                if (qd >= ldlq) { qd -= ldlq; ++r; }
            }
        }
        if (threadIdx.x == 0) {
            if (rows > 1) t.basis[cr] = e.i;                   // src/simplex.lisp:358
            if (t.trace_ec && trace_n < t.trace_cap) { t.trace_ec[trace_n] = e.i; t.trace_cr[trace_n] = cr; }
        }
        ++n; ++trace_n; last_ec = e.i; last_cr = cr;
        __syncthreads();
    }
    __syncthreads();
    {
        int r = (int)threadIdx.x / ldlq, qd = (int)threadIdx.x % ldlq;
        for (int idx = threadIdx.x; idx < nq; idx += THREADS) {
            G4[(int64_t)r * ldq + qd] = L4[idx];
            r += step_r; qd += step_q;
            if (qd >= ldlq) { qd -= ldlq; ++r; }
        }
    }
    if (threadIdx.x == 0) {
        ctl->status = status; ctl->n_pivots = n; ctl->trace_n = trace_n; ctl->ec = last_ec; ctl->cr = last_cr;
    }
}
// one tableau behind a handle: one 1024-thread workgroup (the batch form is k_sb_solve, kernels_single_batch.inc)
__global__ __launch_bounds__(kSelThreads) void k_s_solve(SView t, float sgn, float price_tol, float ratio_thr, int cap)
{
    s_solve_in_lds<kSelThreads>(t, sgn, price_tol, ratio_thr, cap);
}

// ------------------------------------------------------------------ two-phase hand-over, the copy
// src/simplex.lisp:437-441: main[r][0..nv) = art[r][0..nv), main[r][nv] = art[r][nav], r < m.
__global__ __launch_bounds__(256) void k_s_handover_copy(SView art, SView mt)
{
    const int64_t nv = mt.cols - 1, nav = art.cols - 1, m = mt.rows - 1;
    for (int64_t r = blockIdx.y; r < m; r += gridDim.y)
        for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c <= nv; c += (int64_t)gridDim.x * blockDim.x)
            mt.M[r * mt.ld + c] = art.M[r * art.ld + (c < nv ? c : nav)];
}

// ------------------------------------------------------------------ host-side launchers
SingleThresholds single_thresholds(double fp_factor)
{
    // computed in float from the factor: (* (/ factor 8) single-float-epsilon) and its kin
    const float f = (float)fp_factor;
    SingleThresholds th;
    th.price = (f / 8.0f) * kClEpsilonSingle;
    th.ratio = 0.0f + (f / 2.0f) * kClEpsilonSingle;
    th.feasible = f * kClEpsilonSingle;
    return th;
}
static inline float s_sgn_of(int is_max) { return is_max ? 1.0f : -1.0f; }

void launch_s_ctl_reset(const SView &t, int64_t max_pivots, int reset_trace, hipStream_t s)
{
    hipLaunchKernelGGL(k_ctl_reset, dim3(1), dim3(1), 0, s, t.ctl, max_pivots, reset_trace);
}
void launch_s_select(const SView &t, int is_max, double f, hipStream_t s)
{
    const SingleThresholds th = single_thresholds(f);
    if (t.rows <= 1024 && t.ld <= 8192)
        hipLaunchKernelGGL(k_s_select<256>, dim3(1), dim3(256), 0, s, t, s_sgn_of(is_max), th.price, th.ratio);
    else
        hipLaunchKernelGGL(k_s_select<kSelThreads>, dim3(1), dim3(kSelThreads), 0, s, t, s_sgn_of(is_max), th.price, th.ratio);
}
void launch_s_price_only(const SView &t, int is_max, double f, hipStream_t s)
{
    hipLaunchKernelGGL(k_s_price_only, dim3(1), dim3(kSelThreads), 0, s, t, s_sgn_of(is_max), single_thresholds(f).price);
}
void launch_s_ratio_only(const SView &t, int64_t ec, double f, hipStream_t s)
{
    hipLaunchKernelGGL(k_s_ratio_only, dim3(1), dim3(kSelThreads), 0, s, t, (int)ec, single_thresholds(f).ratio);
}
void launch_s_prepare_pivot(const SView &t, int64_t ec, int64_t cr, hipStream_t s)
{
    hipLaunchKernelGGL(k_s_prepare_pivot, dim3(1), dim3(kSelThreads), 0, s, t, (int)ec, (int)cr);
}

// Tile shape of k_s_update: equal-width strips of a multiple of 8 quads (128 bytes), and rows per workgroup such
// that the whole grid is resident in ONE balanced round (256 CUs x 8 workgroups of 256 threads), never fewer
// than U rows.
SingleUpdateShape single_update_shape(const SView &t)
{
    constexpr int block = 256, unroll = 4;
    const int64_t ldq = t.ld >> 2;
    SingleUpdateShape g;
    g.strips = (int)((ldq + block - 1) / block);
    int64_t sq = (ldq + g.strips - 1) / g.strips;
    sq = (sq + 7) / 8 * 8;
    if (sq > block) sq = block;
    g.strip_quads = (int)sq;
    g.strips = (int)((ldq + sq - 1) / sq);
    const int64_t slots = (int64_t)kCUs * (kThreadsPerCU / block);
    int64_t by = slots / g.strips;
    if (by < 1) by = 1;
    int64_t tr = (t.rows + by - 1) / by;
    if (tr < unroll) tr = unroll;
    tr = (tr + unroll - 1) / unroll * unroll;
    while ((t.rows + tr - 1) / tr > 65535) tr *= 2;            // grid.y limit
    g.tr = (int)tr;
    g.row_chunks = (int)((t.rows + tr - 1) / tr);
    return g;
}
void launch_s_update(const SView &t, hipStream_t s)
{
    const SingleUpdateShape g = single_update_shape(t);
    hipLaunchKernelGGL((k_s_update<256, 4>), dim3((unsigned)g.strips, (unsigned)g.row_chunks), dim3(256), 0, s, t,
                       g.tr, g.strip_quads);
}

// dynamic LDS of k_s_solve for this shape: stored tableau + pivot row + column snapshot
size_t single_lds_bytes(const SView &t)
{
    const size_t ldl = (size_t)((t.cols + 3) / 4 * 4), rp = (size_t)((t.rows + 3) / 4 * 4);
    return ((size_t)t.rows * ldl + ldl + rp) * sizeof(float);
}
// false: the shape does not fit the budget, or the attribute could not be raised (the caller takes the pair)
bool single_lds_available(const SView &t)
{
    if (single_lds_bytes(t) > kSingleLdsBudget || t.cols < 2) return false;
    // (once per handle, on the handle's device)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_s_solve),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSingleLdsBudget);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;
}
void launch_s_solve(const SView &t, int is_max, double f, int cap, hipStream_t s)
{
    const SingleThresholds th = single_thresholds(f);
    hipLaunchKernelGGL(k_s_solve, dim3(1), dim3(kSelThreads), single_lds_bytes(t), s, t, s_sgn_of(is_max), th.price,
                       th.ratio, cap);
}
void launch_s_handover_copy(const SView &art, const SView &mt, hipStream_t s)
{
    const int64_t m = mt.rows - 1;
    if (m < 1) return;
    int bx = (int)((mt.cols + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(k_s_handover_copy, dim3(bx, (unsigned)(m < 32768 ? m : 32768)), dim3(256), 0, s, art, mt);
}
