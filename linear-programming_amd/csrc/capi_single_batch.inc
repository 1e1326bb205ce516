// capi_single_batch.inc -- mi355x_sbatch_*: n_lps SINGLE-FLOAT tableaux of one shape behind a handle, one workgroup
// per member for its whole solve, the member's tableau in LDS (form 2, kernels_single_batch.inc) or left in HBM (form
// 3, the opt-in global form for members beyond the LDS budget: kernels_single_global.inc).  The contract is member by
// member: what a member ends with
// -- status, pivot counts, trace, basis, every tableau entry -- is what mi355x_stab_solve / _solve_two_phase gives that
// member alone under the same sequence of calls.  No double touches a tableau entry.
// Form 4, the RAGGED batch (capi_single_ragged.inc makes it): every member its own shape and sense, the same entries.
// Part of simplex_capi.hip (ONE translation unit: included there, in this order).

namespace {
int g_sbatch_threads = 0;                 // tuning / test hook: 0 auto (sbatch_threads_for), 256 or 1024
int g_sbatch_launch_cap = 0;              // tuning / test hook: 0 = the form's default, else pivots per member and launch
int g_sbatch_global_threads = 0;          // tuning / test hook, global form: 0 auto (sgbatch_threads_for), 256 or 1024
int g_sbatch_ragged_classes = 0;          // tuning / test hook, ragged batches: 0 the default (one class), 1 one class, 4 up to four
constexpr int kSbFormLds = 2, kSbFormGlobal = 3, kSbFormRagged = 4;   // (continuing mi355x_stab_info's numbering: 1 pair, 2 LDS)
// an occupancy class of a ragged batch: `count` member indices from d_index + first, launched with `lds` bytes (the
// class's largest member's) at `per_cu` resident workgroups per compute unit
struct SrClass { int64_t first, count; size_t lds; int per_cu; };
}  // namespace

struct mi355x_sbatch {
    int         device = 0;
    SbView      v{};
    hipStream_t stream = nullptr;
    int         form = 2;                 // 2: the member's tableau in LDS (k_sb_solve), 3: in HBM (SolveInHbm), 4: ragged (SrView)
    int         threads = 0;              // snapshot of the form's rule (or its hook) at create
    int         launch_cap = kSingleLaunchCap;
    int         members_per_cu = 0;       // hipOccupancyMaxActiveBlocksPerMultiprocessor of the form's solve kernel at this shape
    void       *rb = nullptr;         // mi355x_sbatch_readback's gather buffer (made at its first call)
    int32_t    *d_phase = nullptr;        // artificial batch of a two-phase pair: per member (state, status between the phases)
    std::vector<Ctl>     h;               // the control blocks as the last read-back left them
    std::vector<int32_t> h_phase;
    std::atomic<int> cancel{0};
    // form 4 (v keeps M, basis, ctl, the traces and n_lps; its rows, cols, ld and stride are 0)
    SrView      r{};
    SrMember   *d_members = nullptr;      // r.members
    int32_t    *d_index = nullptr;        // the classes' member lists, one after the other
    size_t      lds_max = 0;              // the dynamic LDS of the form's solve kernel for the largest member (forms 2, 3: every member)
    int64_t     m_total = 0;              // floats of all members as stored
    int64_t    *d_col_off = nullptr;      // mi355x_sbatch_readback_ragged: per member the columns of the members before it
    std::vector<SrMember> hm;             // the descriptors, host copy
    std::vector<int>      member_class;   // per member: index into classes
    std::vector<SrClass>  classes;        // the class of the largest members first
};

namespace {

void free_sbatch(mi355x_sbatch *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    (void)hipFree(b->v.M);
    (void)hipFree(b->v.basis);
    (void)hipFree(b->v.ctl);
    (void)hipFree(b->v.trace_ec);
    (void)hipFree(b->v.trace_cr);
    (void)hipFree(b->d_phase);
    (void)hipFree(b->rb);
    (void)hipFree(b->d_members);
    (void)hipFree(b->d_index);
    (void)hipFree(b->d_col_off);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

// the ONE failure path of a create: the handle(s) freed, "<what> failed: <the runtime's words>"
int sb_failed(mi355x_sbatch *b, mi355x_sbatch *other, hipError_t e, const char *what)
{
    (void)hipGetLastError();
    free_sbatch(b);
    free_sbatch(other);
    return fail(e == hipErrorOutOfMemory ? MI_NO_MEMORY : MI_HIP_ERROR, "%s failed: %s", what, hipGetErrorString(e));
}

int sb_read(mi355x_sbatch *b, hipStream_t s, bool with_phase)
{
    HIP_TRY(hipMemcpyAsync(b->h.data(), b->v.ctl, b->h.size() * sizeof(Ctl), hipMemcpyDeviceToHost, s));
    if (with_phase)
        HIP_TRY(hipMemcpyAsync(b->h_phase.data(), b->d_phase, b->h_phase.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MI_OK;
}

inline bool sb_carried_on(int32_t st) { return st == kRunning || st == MI_MAX_PIVOTS; }

// Member q's descriptor for any form: computed for a batch of one shape (sb_descriptor, the kernels' own rule; hm is
// not made for those -- n_lps goes to 2^30), read from hm for a ragged one.
SrMember sb_host_member(const mi355x_sbatch *b, int64_t q)
{
    return b->form == kSbFormRagged ? b->hm[(size_t)q] : sb_descriptor(b->v, q);
}

// The ONE skeleton of a handle, for every form: the host copies of the control blocks and the phase state, the stream,
// the device buffers for n_lps members of n_floats floats and n_basis basis entries in all, the phase state zeroed
// (zero_tableaux: the tableaux as well).  b is the caller's new handle with its form's fields filled in; on a failure
// it is freed here.  what: the failure message's subject.
int sb_alloc(mi355x_sbatch *b, int64_t n_lps, int64_t n_floats, int64_t n_basis, bool zero_tableaux, const char *what)
{
    SbView &v = b->v;
    v.n_lps = n_lps;
    v.trace_cap = MI355X_SBATCH_TRACE_CAP;
    try {
        b->h.resize((size_t)n_lps);
        b->h_phase.assign((size_t)(2 * n_lps), 0);
    } catch (const std::bad_alloc &) {
        delete b;
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    const size_t mbytes = (size_t)n_floats * sizeof(float);
    hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&v.M, mbytes);
    if (e == hipSuccess) e = hipMalloc((void **)&v.basis, (size_t)std::max<int64_t>(n_basis, 1) * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&v.ctl, (size_t)n_lps * sizeof(Ctl));
    if (e == hipSuccess) e = hipMalloc((void **)&v.trace_ec, (size_t)(n_lps * v.trace_cap) * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&v.trace_cr, (size_t)(n_lps * v.trace_cap) * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_phase, (size_t)(2 * n_lps) * sizeof(int32_t));
    if (e == hipSuccess && zero_tableaux) e = hipMemsetAsync(v.M, 0, mbytes, b->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_phase, 0, (size_t)(2 * n_lps) * sizeof(int32_t), b->stream);
    if (e != hipSuccess) return sb_failed(b, nullptr, e, what);
    return MI_OK;
}

// An empty batch of the shape: the checks of mi355x_sbatch_create, the handle, its stream and its device buffers
// (zero_padding: the tableaux zeroed where a row has padding -- for members that are uploaded tight).
// MI_UNSUPPORTED: the shape does not fit the LDS budget (form 3: its pivot row and column snapshot do not).
int sb_new(mi355x_sbatch **out, int64_t n_lps, int64_t rows, int64_t cols, int device, bool zero_padding,
           int form = kSbFormLds)
{
    if (n_lps < 1 || n_lps > (1LL << 30)) return fail(MI_BAD_ARG, "n_lps=%lld must be in [1, 2^30]", (long long)n_lps);
    if (rows < 1 || cols < 1) return fail(MI_BAD_ARG, "rows=%lld cols=%lld must be >= 1", (long long)rows, (long long)cols);
    if (rows > 65535LL * 16) return fail(MI_BAD_ARG, "rows=%lld exceeds the supported 1048560", (long long)rows);
    if (cols > (1LL << 30)) return fail(MI_BAD_ARG, "cols=%lld exceeds the supported 2^30", (long long)cols);
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(MI_BAD_ARG, "device %d out of range [0,%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    mi355x_sbatch *b = new (std::nothrow) mi355x_sbatch;
    if (!b) return fail(MI_NO_MEMORY, "host allocation failed");
    b->device = device;
    SbView &v = b->v;
    v.rows = rows;
    v.cols = cols;
    v.ld = (cols + kSingleLdAlign - 1) / kSingleLdAlign * kSingleLdAlign;
    v.stride = rows * v.ld;
    b->form = form;
    bool fits;
    if (form == kSbFormGlobal) {
        b->threads = g_sbatch_global_threads ? g_sbatch_global_threads : sgbatch_threads_for(rows, v.ld);
        b->launch_cap = g_sbatch_launch_cap ? g_sbatch_launch_cap : sgbatch_launch_cap_for(rows, v.ld);
        b->lds_max = sgbatch_lds_bytes(v);
        fits = sgbatch_available(v, b->threads, &b->members_per_cu);
    } else {
        b->threads = g_sbatch_threads ? g_sbatch_threads : sbatch_threads_for(rows, cols);
        b->launch_cap = g_sbatch_launch_cap ? g_sbatch_launch_cap : kSingleLaunchCap;
        b->lds_max = sbatch_lds_bytes(v);
        fits = sbatch_available(v, b->threads, &b->members_per_cu);
    }
    // the shapes the form does not hold (or may not have) are declined: the LDS form's members go one by one
    if (!fits || b->members_per_cu < 1) {
        delete b;
        return fail(MI_UNSUPPORTED, "%s %lldx%lld single-float member does not fit the LDS budget of %lld bytes",
                    form == kSbFormGlobal ? "the pivot row and column snapshot of a" : "a",
                    (long long)rows, (long long)cols, (long long)kSingleLdsBudget);
    }
    const int rc = sb_alloc(b, n_lps, n_lps * v.stride, n_lps * std::max<int64_t>(rows - 1, 1), zero_padding && v.ld != v.cols,
                            "single-float batch allocation");
    if (rc != MI_OK) return rc;
    *out = b;
    return MI_OK;
}

// every member MI_RUNNING with no pivots and an empty trace, on the device and in b->h; waits for the batch's stream
hipError_t sb_fresh_ctl(mi355x_sbatch *b)
{
    launch_sb_ctl_reset(b->v, b->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(b->h.data(), b->v.ctl, (size_t)b->v.n_lps * sizeof(Ctl), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    return e;
}

// the form's solve kernel on every member the gate lets run (form 4: one launch per occupancy class, the members'
// own senses)
void sb_launch_solve(const mi355x_sbatch *b, int is_max, double f, const int32_t *gate, hipStream_t s)
{
    if (b->form == kSbFormRagged)
        for (const SrClass &c : b->classes)                 // (one class holds every member: no list to go through)
            launch_sb_solve(b->r, b->classes.size() == 1 ? nullptr : b->d_index + c.first, c.count, c.lds, b->threads, f,
                            b->launch_cap, gate, s);
    else if (b->form == kSbFormGlobal) launch_sg_solve(b->v, b->threads, is_max, f, b->launch_cap, gate, s);
    else launch_sb_solve(b->v, b->threads, is_max, f, b->launch_cap, gate, s);
}

// the form's step between the phases (form 4: one launch per class of the artificial batch)
void sb_launch_between(const mi355x_sbatch *art, const mi355x_sbatch *mt, double f, int64_t max_pivots, hipStream_t s)
{
    if (art->form == kSbFormRagged)
        for (const SrClass &c : art->classes)
            launch_sb_between(art->r, mt->r, art->classes.size() == 1 ? nullptr : art->d_index + c.first, c.count, c.lds,
                              art->threads, art->d_phase, f, max_pivots, s);
    else if (art->form == kSbFormGlobal) launch_sg_between(art->v, mt->v, art->threads, art->d_phase, f, max_pivots, s);
    else launch_sb_between(art->v, mt->v, art->threads, art->d_phase, f, max_pivots, s);
}

// a ragged batch carries its members' senses: the call's is_max must say so
int sb_check_sense(const mi355x_sbatch *b, int is_max)
{
    if (b->form == kSbFormRagged && is_max != -1)
        return fail(MI_BAD_ARG, "is_max=%d on a ragged batch (form 4): pass -1, the sense is each member's own", is_max);
    return MI_OK;
}

// mi355x_sbatch_create / _create_global: the checks, the handle of the form, the upload
int sb_create(mi355x_sbatch **out, int64_t n_lps, int64_t rows, int64_t cols, const float *matrices, const int64_t *basis,
              int device, int form)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (!matrices) return fail(MI_BAD_ARG, "matrices is NULL");
    if (rows > 1 && !basis) return fail(MI_BAD_ARG, "basis is NULL");
    mi355x_sbatch *b = nullptr;
    const int rc = sb_new(&b, n_lps, rows, cols, device, /*zero_padding=*/true, form);
    if (rc != MI_OK) return rc;
    SbView &v = b->v;
    hipError_t e = hipMemcpy2DAsync(v.M, v.ld * sizeof(float), matrices, cols * sizeof(float), cols * sizeof(float),
                                    (size_t)(n_lps * rows), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess && rows > 1)
        e = hipMemcpyAsync(v.basis, basis, (size_t)(n_lps * (rows - 1)) * sizeof(int64_t), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) e = sb_fresh_ctl(b);
    if (e != hipSuccess) return sb_failed(b, nullptr, e, "single-float batch upload");
    *out = b;
    return MI_OK;
}

// device memory of a create, freed with the scope (the creates of capi_single_bb.inc, capi_single_lps.inc and capi_single_ragged_build.inc)
struct SbDeviceMem {
    void *mem = nullptr;
    ~SbDeviceMem() { (void)hipFree(mem); }
};
inline size_t sb_align(size_t x) { return (x + 255) & ~(size_t)255; }

// The ONE (main, artificial) pair of batches around an assembly, for every form.  make(&handle, artificial) makes an
// empty handle (sb_new, sr_new); two == false: no artificial batch.  The larger shape first: a pair the budget declines
// allocates nothing.  fill(main, artificial or nullptr) -> hipError_t allocates, uploads and launches on the main
// handle's stream; what it allocates has to live until this function returns.
template <class Make, class Fill>
int sb_pair_build(mi355x_sbatch **out_main, mi355x_sbatch **out_art, bool two, const char *what, Make make, Fill fill)
{
    mi355x_sbatch *mt = nullptr, *art = nullptr;
    int rc = MI_OK;
    if (two) rc = make(&art, true);
    if (rc == MI_OK) rc = make(&mt, false);
    if (rc != MI_OK) {
        free_sbatch(mt);
        free_sbatch(art);
        return rc;
    }
    // the assembly runs on the main handle's stream and reads the artificial handle's descriptors where there are any
    // (a ragged batch): they have landed
    hipError_t e = art && art->d_members ? hipStreamSynchronize(art->stream) : hipSuccess;
    if (e == hipSuccess) e = fill(mt, art);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = sb_fresh_ctl(mt);                              // (waits for the assembly as well)
    if (e == hipSuccess && art) e = sb_fresh_ctl(art);
    if (e != hipSuccess) return sb_failed(mt, art, e, what);
    *out_main = mt;
    *out_art = art;
    return MI_OK;
}
// the pair of one shape (rows, cols) and n_art more columns in the artificial batch; form: both handles'
template <class Fill>
int sb_pair_build(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n, int64_t rows, int64_t cols, int64_t n_art,
                  int device, const char *what, Fill fill, int form)
{
    return sb_pair_build(out_main, out_art, n_art != 0, what, [&](mi355x_sbatch **h, bool artificial) {
        return sb_new(h, n, rows, artificial ? cols + n_art : cols, device, /*zero_padding=*/false, form);
    }, [&](mi355x_sbatch *mt, mi355x_sbatch *art) { return fill(mt->stream, mt->v, art ? art->v : SbView{}); });
}

// The ONE body of the light read-back, for every form: the members' rows and columns in all say the three plane sizes
// (a member has rows - 1 basis entries).  One buffer, the basis plane first (8-byte entries), then the two float
// planes; one gather, one copy.
int sb_readback(mi355x_sbatch *b, int64_t n_rows, int64_t n_cols, float *rhs, float *obj_row, int64_t *basis)
{
    HIP_TRY(hipSetDevice(b->device));
    const int64_t n = b->v.n_lps;
    const size_t nbasis = (size_t)(n_rows - n) * sizeof(int64_t), nrhs = (size_t)n_rows * sizeof(float), nobj = (size_t)n_cols * sizeof(float);
    std::vector<char> host;
    try {
        if (b->form == kSbFormRagged && !b->d_col_off) {                    // (once per handle: the running sums of cols)
            std::vector<int64_t> off((size_t)n);
            int64_t c = 0;
            for (int64_t q = 0; q < n; ++q) { off[q] = c; c += b->hm[q].cols; }
            HIP_TRY(hipMalloc((void **)&b->d_col_off, (size_t)n * sizeof(int64_t)));
            HIP_TRY(hipMemcpy(b->d_col_off, off.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
        }
        host.resize(nbasis + nrhs + nobj);
    } catch (const std::bad_alloc &) {
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    if (!b->rb) HIP_TRY(hipMalloc(&b->rb, nbasis + nrhs + nobj));
    char *d = (char *)b->rb;
    float *d_rhs = (float *)(d + nbasis), *d_obj = (float *)(d + nbasis + nrhs);
    if (b->form == kSbFormRagged) launch_sb_readback(b->r, b->d_col_off, d_rhs, d_obj, (int64_t *)d, b->stream);
    else launch_sb_readback(b->v, d_rhs, d_obj, (int64_t *)d, b->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host.data(), d, host.size(), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (nbasis > 0) std::memcpy(basis, host.data(), nbasis);
    std::memcpy(rhs, host.data() + nbasis, nrhs);
    std::memcpy(obj_row, host.data() + nbasis + nrhs, nobj);
    return MI_OK;
}

}  // namespace

extern "C" {

int mi355x_sbatch_create(mi355x_sbatch **out, int64_t n_lps, int64_t rows, int64_t cols, const float *matrices,
                         const int64_t *basis, int device)
{
    return sb_create(out, n_lps, rows, cols, matrices, basis, device, kSbFormLds);
}

int mi355x_sbatch_create_global(mi355x_sbatch **out, int64_t n_lps, int64_t rows, int64_t cols, const float *matrices,
                                const int64_t *basis, int device)
{
    return sb_create(out, n_lps, rows, cols, matrices, basis, device, kSbFormGlobal);
}

void mi355x_sbatch_destroy(mi355x_sbatch *b) { free_sbatch(b); }

int mi355x_sbatch_info(const mi355x_sbatch *b, int64_t *n_lps, int64_t *rows, int64_t *cols, int64_t *ld,
                       int *workgroup_threads, int64_t *lds_bytes_per_member, int *members_per_cu)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    // (a ragged batch has no one shape: its v says 0; the largest member's LDS, the smallest class's residency)
    if (n_lps) *n_lps = b->v.n_lps;
    if (rows) *rows = b->v.rows;
    if (cols) *cols = b->v.cols;
    if (ld) *ld = b->v.ld;
    if (workgroup_threads) *workgroup_threads = b->threads;
    if (lds_bytes_per_member) *lds_bytes_per_member = (int64_t)b->lds_max;
    if (members_per_cu) *members_per_cu = b->members_per_cu;
    return MI_OK;
}

int mi355x_sbatch_form(const mi355x_sbatch *b, int *form)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (form) *form = b->form;
    return MI_OK;
}

// n-solve-tableau, single tableau (src/simplex.lisp:453-461), on every member the call carries on: bounded launches,
// one read-back of the control blocks per round, the cancel flag looked at between rounds.
int mi355x_sbatch_solve(mi355x_sbatch *b, int is_max, double f, int64_t max_pivots, int32_t *status, int64_t *n_pivots)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    if (sb_check_sense(b, is_max) != MI_OK) return MI_BAD_ARG;
    HIP_TRY(hipSetDevice(b->device));
    const int64_t n = b->v.n_lps;
    std::vector<char> live((size_t)n);
    for (int64_t q = 0; q < n; ++q) live[q] = sb_carried_on(b->h[q].status);
    launch_sb_begin(b->v, max_pivots, nullptr, 0, b->stream);
    bool cancelled = false;
    for (;;) {
        sb_launch_solve(b, is_max, f, nullptr, b->stream);
        HIP_TRY(hipGetLastError());
        const int rc = sb_read(b, b->stream, false);
        if (rc != MI_OK) return rc;
        bool running = false;
        for (int64_t q = 0; q < n && !running; ++q) running = b->h[q].status == kRunning;
        // (a cancel that arrives while the last round finishes goes with the call: it never reaches the next one)
        const int c = b->cancel.exchange(0, std::memory_order_acq_rel);
        if (!running) break;
        if (c) { cancelled = true; break; }                                  // (whole pivots only)
    }
    for (int64_t q = 0; q < n; ++q) {
        if (status) status[q] = b->h[q].status;
        if (n_pivots) n_pivots[q] = live[q] ? b->h[q].n_pivots : 0;
    }
    return cancelled ? MI_CANCELLED : MI_OK;
}

// n-solve-tableau's two-phase branch (src/simplex.lisp:402-452) per member, resumable as mi355x_stab_solve_two_phase
// is: max_pivots caps a member's pivots of THIS call, both phases and the drive-outs together.  A round is phase 1 on
// the artificial batch, the step between the phases for the members whose phase 1 just ended, phase 2 on the main batch.
int mi355x_sbatch_solve_two_phase(mi355x_sbatch *art, mi355x_sbatch *mt, int main_is_max, double f, int64_t max_pivots,
                                  int32_t *status, int64_t *n_pivots)
{
    if (!art || !mt) return fail(MI_BAD_ARG, "NULL handle");
    if (art == mt) return fail(MI_BAD_ARG, "artificial and main batch are the same handle");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    if (art->v.n_lps != mt->v.n_lps || art->v.rows != mt->v.rows || art->v.cols < mt->v.cols || art->device != mt->device)
        return fail(MI_BAD_ARG, "artificial and main batch do not match");
    if (art->form != mt->form) return fail(MI_BAD_ARG, "artificial and main batch are of different forms");
    if (sb_check_sense(mt, main_is_max) != MI_OK) return MI_BAD_ARG;
    if (art->form == kSbFormRagged)                        // (one shape: the test above has said it for every member)
        for (int64_t q = 0; q < art->v.n_lps; ++q)
            if (art->hm[q].rows != mt->hm[q].rows || art->hm[q].cols < mt->hm[q].cols)
                return fail(MI_BAD_ARG, "artificial and main batch do not match at member %lld", (long long)q);
    if (art->form == kSbFormGlobal && sgbatch_between_lds_bytes(art->v) > kSingleLdsBudget)
        return fail(MI_UNSUPPORTED, "the step between the phases of a %lldx%lld artificial member does not fit the LDS "
                    "budget of %lld bytes", (long long)art->v.rows, (long long)art->v.cols, (long long)kSingleLdsBudget);
    HIP_TRY(hipSetDevice(art->device));
    const int64_t n = art->v.n_lps;
    hipStream_t s = art->stream;
    HIP_TRY(hipStreamSynchronize(mt->stream));
    std::vector<char> live_a((size_t)n), live_m((size_t)n);
    for (int64_t q = 0; q < n; ++q) {
        const int32_t ph = art->h_phase[2 * q];
        live_a[q] = ph == 0 && (sb_carried_on(art->h[q].status) || art->h[q].status == MI_OPTIMAL);
        live_m[q] = ph == 1 && sb_carried_on(mt->h[q].status);
    }
    launch_sb_begin(art->v, max_pivots, art->d_phase, 0, s);
    launch_sb_begin(mt->v, max_pivots, art->d_phase, 1, s);
    bool cancelled = false, phase1 = false;
    for (int64_t q = 0; q < n && !phase1; ++q) phase1 = live_a[q];
    for (;;) {
        if (phase1) {
            sb_launch_solve(art, /*is_max=*/0, f, nullptr, s);                                       // simplex.lisp:403
            sb_launch_between(art, mt, f, max_pivots, s);
        }
        sb_launch_solve(mt, main_is_max, f, art->d_phase, s);                                        // simplex.lisp:452
        HIP_TRY(hipGetLastError());
        int rc = sb_read(art, s, true);
        if (rc == MI_OK) rc = sb_read(mt, s, false);
        if (rc != MI_OK) return rc;
        bool running = false;
        phase1 = false;
        for (int64_t q = 0; q < n; ++q) {
            const int32_t ph = art->h_phase[2 * q];
            if (ph == 0 && art->h[q].status == kRunning) phase1 = running = true;
            else if (ph == 1 && mt->h[q].status == kRunning) running = true;
        }
        int c = art->cancel.exchange(0, std::memory_order_acq_rel);         // (as in mi355x_sbatch_solve)
        c |= mt->cancel.exchange(0, std::memory_order_acq_rel);
        if (!running) break;
        if (c) { cancelled = true; break; }                                  // (whole pivots only)
    }
    for (int64_t q = 0; q < n; ++q) {
        const int32_t ph = art->h_phase[2 * q];
        if (status) status[q] = ph == 2 ? art->h_phase[2 * q + 1] : ph == 1 ? mt->h[q].status : art->h[q].status;
        if (n_pivots) {
            n_pivots[2 * q] = live_a[q] ? art->h[q].n_pivots : 0;
            n_pivots[2 * q + 1] = ph == 1 && (live_a[q] || live_m[q]) ? mt->h[q].n_pivots : 0;
        }
    }
    return cancelled ? MI_CANCELLED : MI_OK;
}

int mi355x_sbatch_download(mi355x_sbatch *b, int64_t q, float *hm, int64_t *hb, float *last_row, float *last_col)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (q < 0 || q >= b->v.n_lps) return fail(MI_BAD_ARG, "lp_index %lld out of range [0,%lld)", (long long)q, (long long)b->v.n_lps);
    HIP_TRY(hipSetDevice(b->device));
    const SrMember d = sb_host_member(b, q);
    const int rc = download_parts(b->v.M + d.m_off, d.ld, d.rows, d.cols, b->v.basis + d.basis_off, b->stream, hm, hb,
                                  last_row, last_col);
    if (rc != MI_OK) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return MI_OK;
}

int mi355x_sbatch_trace(mi355x_sbatch *b, int64_t q, int64_t *ecs, int64_t *crs, int64_t cap, int64_t *n)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (q < 0 || q >= b->v.n_lps) return fail(MI_BAD_ARG, "lp_index %lld out of range [0,%lld)", (long long)q, (long long)b->v.n_lps);
    HIP_TRY(hipSetDevice(b->device));
    Ctl c{};
    HIP_TRY(hipMemcpyAsync(&c, b->v.ctl + q, sizeof(Ctl), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return download_trace(b->v.trace_ec + q * b->v.trace_cap, b->v.trace_cr + q * b->v.trace_cap, c.trace_n, b->v.trace_cap,
                          b->stream, ecs, crs, cap, n);
}

int mi355x_sbatch_cancel(mi355x_sbatch *b)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    b->cancel.store(1, std::memory_order_release);
    return MI_OK;
}

int mi355x_tune_set_sbatch_threads(int threads)
{
    if (threads != 0 && threads != 256 && threads != 1024) return fail(MI_BAD_ARG, "threads must be 0 (auto), 256 or 1024");
    g_sbatch_threads = threads;
    return MI_OK;
}

int mi355x_tune_set_sbatch_global_threads(int threads)
{
    if (threads != 0 && threads != 256 && threads != 1024) return fail(MI_BAD_ARG, "threads must be 0 (auto), 256 or 1024");
    g_sbatch_global_threads = threads;
    return MI_OK;
}

int mi355x_tune_set_sbatch_launch_cap(int cap)
{
    if (cap < 0) return fail(MI_BAD_ARG, "cap must be 0 (the default) or a count of pivots");
    g_sbatch_launch_cap = cap;
    return MI_OK;
}

}  // extern "C"
