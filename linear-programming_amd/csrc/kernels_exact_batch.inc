// kernels_exact_batch.inc -- many exact rational LPs of one shape side by side, one workgroup per LP.
// Part of simplex_kernels.hip (ONE translation unit: included there after kernels_exact.inc, whose rules
// -- x_price, x_ratio, x_record, x_snapshot, x_update_elem, x_handover_column -- it only loops around).
//
//   k_xb_solve<T, kRules>  the whole n-solve-tableau loop (src/simplex.lisp:453-461, rational dispatch) of one
//                    member inside one launch: pricing, ratio test, pivot record, snapshots of the
//                    entering column (times sgn) and the pivot row in LDS, the update in place
//   k_xb_between<T>  everything between the phases (src/simplex.lisp:405-451) of one member: the exact
//                    feasibility test, the drive-out pivots, the hand-over into the main member
//
// Workgroup size 256 = four waves, one per SIMD of the CU.  A member's pivot is a chain of barriers
// (two reductions, the snapshots, the update), so its latency is what counts: the tableaux this is for
// have a few hundred entries, and 256 threads update such a tableau in one or two trips with the
// 256-bit products of the 128-bit form issuing on all four SIMDs at once, where one wave would walk it
// in a serial loop.  More waves per member would only add barrier cost.  Members run side by side
// instead: at the 128-bit form's register count (DESIGN.md quotes the compiler's report) several
// waves fit a SIMD, and the LDS of a small member (the reduction scratch, about 10 KiB at 128 bits,
// plus the two snapshots) allows more than ten workgroups per CU, so registers, not LDS, bound the
// residency.  The snapshots are dynamic LDS, (rows + cols) values of the width; a shape whose
// snapshots at 128 bits exceed kXbSnapshotLimit is declined at creation (capi_exact_batch.inc).

// Snapshots and the update of the pivot in *rec (written by thread 0, *s_err zeroed with it): every
// thread of the workgroup calls this.  0, kXOverflow or kXInexact (the tableau is garbage then).
template <class T> __device__ inline int xb_apply(T *M, int R, int C, T *col, T *prow, const XPivot *rec, int *s_err)
{
    const int tid = threadIdx.x;
    __syncthreads();
    const XPivotT<T> p(*rec);
    x_snapshot<T>(M, R, C, p, col, prow);
    __syncthreads();
    // element k = r * C + j of this thread: k = tid, tid + 256, ... walked as (r, j) without a division per element
    const int dr = kXThreads / C, dj = kXThreads % C;
    int r = tid / C, j = tid % C;
    int err = 0;
    while (r < R) {
        err = max(err, x_update_elem<T>(M + (int64_t)r * C + j, r, col[r], prow[j], p));
        r += dr;
        j += dj;
        if (j >= C) { j -= C; r += 1; }
    }
    if (err) atomicMax(s_err, err);
    __syncthreads();
    return *s_err;
}

// kRules: as for k_x_select
template <class T, bool kRules> __global__ __launch_bounds__(kXThreads) void k_xb_solve(XbView v, int is_max, int64_t launch_cap)
{
    extern __shared__ __int128 xb_lds[];
    __shared__ T sv[kXThreads], sa[kXThreads];
    __shared__ int64_t si[kXThreads], sk[kRules ? kXThreads : 1];
    __shared__ XPivot rec;
    __shared__ int s_err, s_go;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    XbCtl *c = v.ctl + q;
    if (tid == 0) s_go = c->status == kRunning;
    __syncthreads();
    if (!s_go) return;
    const int R = (int)v.rows, C = (int)v.cols;
    const int64_t m = R - 1, nv = C - 1;
    T *M = (T *)v.T + q * (int64_t)R * C;
    T *col = (T *)xb_lds, *prow = col + R;
    int64_t *basis = v.basis + q * m;
    int64_t *tec = v.trace_ec + q * v.trace_cap, *tcr = v.trace_cr + q * v.trace_cap;
    // the member's state, the same in every thread; thread 0 stores it at the end
    int64_t n_pivots = c->n_pivots, trace_n = c->trace_n;
    const int64_t cap_at = c->cap_at;
    const int rule = kRules ? v.rule : 0;
    int stall = kRules ? c->stall : 0;
    __int128 D = c->D;
    int status = kRunning;
    for (int64_t it = 0; it < launch_cap; ++it) {
        if (cap_at > 0 && n_pivots >= cap_at) { status = 3; break; }                       // MI_MAX_PIVOTS
        const bool bland = x_bland(rule, stall);
        const int64_t ec = x_price<T>(M + m * C, nv, is_max, bland, sv, si);
        if (ec < 0) { status = 0; break; }                                                  // MI_OPTIMAL
        const int64_t cr = x_ratio<T>(M, m, C, nv, ec, basis, bland, sv, sa, si, sk);
        if (cr < 0) { status = 1; break; }                                                  // MI_UNBOUNDED
        // a degenerate pivot: rule 2 selects by Bland's rule next (read before xb_apply's first barrier, so
        // before any thread updates the tableau)
        if (rule == 2) stall = M[cr * C + nv] == 0;
        if (tid == 0) {
            x_record<T>(&rec, M, C, ec, cr, D);
            s_err = 0;
            basis[cr] = ec;
            if (trace_n < v.trace_cap) { tec[trace_n] = ec; tcr[trace_n] = cr; }
        }
        trace_n += 1;
        n_pivots += 1;
        const int e = xb_apply<T>(M, R, C, col, prow, &rec, &s_err);
        D = rec.pa;
        if (e) { status = e; break; }
    }
    if (tid == 0) {
        c->status = status;
        c->n_pivots = n_pivots;
        c->trace_n = trace_n;
        if (kRules) c->stall = stall;
        c->D = D;
    }
}

// Between the phases of member q, on the device: runs when phase 1 has just ended MI_OPTIMAL (tp == 0).
// Outcome in the artificial member's control block: tp = 1 and the main member kRunning (or
// MI_MAX_PIVOTS when the drive-outs used the call's pivots up), tp = 2 with tp_status MI_INFEASIBLE /
// MI_ART_NONZERO / MI_ART_STUCK, or status kXOverflow / kXInexact.  Main's aux holds, per member, cl_j =
// L_c * c_j (cols values) and then L_c, 0 where they do not fit the width.
template <class T> __global__ __launch_bounds__(kXThreads) void k_xb_between(XbView a, XbView mt)
{
    extern __shared__ __int128 xb_lds[];
    __shared__ XPivot rec;
    __shared__ int s_err, s_go, s_j;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    XbCtl *ca = a.ctl + q, *cm = mt.ctl + q;
    if (tid == 0) s_go = ca->status == 0 && ca->tp == 0;
    __syncthreads();
    if (!s_go) return;
    const int R = (int)a.rows, C = (int)a.cols, Cm = (int)mt.cols;
    const int64_t m = R - 1, nav = C - 1, nv = Cm - 1;
    T *A = (T *)a.T + q * (int64_t)R * C;
    T *col = (T *)xb_lds, *prow = col + R;
    int64_t *basis = a.basis + q * m;
    // the exact feasibility test (src/simplex.lisp:405-410)
    if (A[m * C + nav] != 0) {
        if (tid == 0) { ca->tp = 2; ca->tp_status = 2; }                                     // MI_INFEASIBLE
        return;
    }
    // the drive-out loop (src/simplex.lisp:418-436): forced pivots, negative ones included
    __int128 D = ca->D;
    int64_t driveouts = ca->driveouts;
    for (int64_t i = 0; i < m; ++i) {
        if (basis[i] < nv) continue;
        int end = 0;
        if (A[i * C + nav] != 0) end = 4;                                                   // MI_ART_NONZERO
        if (!end) {
            if (tid == 0) s_j = (int)nv;
            __syncthreads();
            for (int64_t j = tid; j < nv; j += kXThreads) {
                if (A[i * C + j] == 0) continue;
                bool basic = false;
                for (int64_t k = 0; k < m && !basic; ++k) basic = basis[k] == j;
                if (!basic) { atomicMin(&s_j, (int)j); break; }
            }
            __syncthreads();
            if (s_j == nv) end = 5;                                                          // MI_ART_STUCK
        }
        if (end) {
            if (tid == 0) { ca->tp = 2; ca->tp_status = end; ca->D = D; ca->driveouts = driveouts; }
            return;
        }
        const int64_t j = s_j;
        if (tid == 0) {
            x_record<T>(&rec, A, C, j, i, D);
            s_err = 0;
            basis[i] = j;
        }
        driveouts += 1;
        const int e = xb_apply<T>(A, R, C, col, prow, &rec, &s_err);
        D = rec.pa;
        if (e) {
            if (tid == 0) { ca->status = e; ca->D = D; ca->driveouts = driveouts; }
            return;
        }
    }
    // the hand-over (src/simplex.lisp:437-451): x_handover_column with w_i = cl[basis[i]]
    T *Mm = (T *)mt.T + q * (int64_t)R * Cm;
    const T *cl = (const T *)mt.aux + q * (int64_t)(Cm + 1);
    const T lc = cl[Cm];
    const T Da = (T)D;
    T *w = col;
    int64_t *mbasis = mt.basis + q * m;
    if (tid == 0) s_err = lc == 0 ? kXOverflow : 0;
    for (int64_t i = tid; i < m; i += kXThreads) { w[i] = cl[basis[i]]; mbasis[i] = basis[i]; }
    __syncthreads();
    int err = 0;
    if (s_err == 0)
        for (int j = tid; j < Cm; j += kXThreads)
            if (!x_handover_column<T>(A, C, Mm, Cm, m, j, Da, w, cl, lc)) err = kXOverflow;
    if (err) atomicMax(&s_err, err);
    __syncthreads();
    if (tid == 0) {
        T d = 0;
        int e = s_err;
        if (!e && !xfit(xmul(lc, Da), &d)) e = kXOverflow;
        ca->D = D;
        ca->driveouts = driveouts;
        if (e) { ca->status = e; return; }
        // what is left of the call's pivots goes to phase 2 (cap_at of the artificial member: the
        // target of both phases together)
        const int64_t target = ca->cap_at, n1 = ca->n_pivots + driveouts;
        cm->D = (__int128)d;
        cm->n_pivots = 0;
        cm->trace_n = 0;
        cm->stall = 0;
        cm->cap_at = target > 0 && target > n1 ? target - n1 : 0;
        cm->status = target > 0 && target <= n1 ? 3 : kRunning;                             // MI_MAX_PIVOTS
        ca->tp = 1;
    }
}

size_t xb_snapshot_bytes(const XbView &v) { return (size_t)(v.rows + v.cols) * (v.bits / 8); }

void launch_xb_solve(const XbView &v, int is_max, int64_t launch_cap, hipStream_t s)
{
    const size_t lds = xb_snapshot_bytes(v);
    x_with_width(v.bits, [&](auto t) {
        typedef decltype(t) T;
        if (v.rule) hipLaunchKernelGGL((k_xb_solve<T, true>), dim3((unsigned)v.n), dim3(kXThreads), lds, s, v, is_max, launch_cap);
        else        hipLaunchKernelGGL((k_xb_solve<T, false>), dim3((unsigned)v.n), dim3(kXThreads), lds, s, v, is_max, launch_cap);
    });
}
void launch_xb_between(const XbView &art, const XbView &mt, hipStream_t s)
{
    const size_t lds = xb_snapshot_bytes(art);
    x_with_width(art.bits, [&](auto t) {
        hipLaunchKernelGGL(k_xb_between<decltype(t)>, dim3((unsigned)art.n), dim3(kXThreads), lds, s, art, mt);
    });
}
