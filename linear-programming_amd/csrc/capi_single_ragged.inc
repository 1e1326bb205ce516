// capi_single_ragged.inc -- mi355x_sbatch_create_ragged: n_lps SINGLE-FLOAT tableaux of their OWN shapes and senses
// behind ONE mi355x_sbatch handle (form 4), one workgroup per member for its whole solve, the member's tableau in LDS
// (kernels_single_batch.inc over an SrView).  The solve, download, trace, cancel and destroy entries are capi_single_batch.inc's,
// with their member-by-member contract: what a member ends with is what mi355x_stab_solve / _solve_two_phase
// (n-solve-tableau, src/simplex.lisp:402-461) gives that member alone under the same sequence of calls.
// A launch has one dynamic-LDS size.  The members are sorted at create into occupancy classes and a round is one
// launch per class, the class of the largest members first.  The default is ONE class -- every member at the largest
// member's LDS size, one launch per round: measured faster than a launch per class, which the stream runs one after
// the other (profiles/sbatch_ragged_rate.txt, part 4).  Under the hook (mi355x_tune_set_sbatch_ragged_classes(4))
// there are up to four classes: the workgroups the runtime reports resident per compute unit at the member's own
// LDS size, capped at 4.
// Part of simplex_capi.hip (ONE translation unit: included there, after capi_single_batch.inc).

namespace {
constexpr int kSrMaxClass = 4;

constexpr const char *kSrUpload = "ragged single-float batch allocation or upload";

// The skeleton of a ragged batch, in two steps around the device check.
// sr_check_shapes: the members' shapes against sb_new's limits (MI_BAD_ARG, no device is looked for); *n_basis: their
// basis entries in all.
int sr_check_shapes(int64_t n_lps, const int64_t *rows, const int64_t *cols, int64_t *n_basis_out)
{
    if (n_lps < 1 || n_lps > (1LL << 30)) return fail(MI_BAD_ARG, "n_lps=%lld must be in [1, 2^30]", (long long)n_lps);
    int64_t n_basis = 0;
    for (int64_t q = 0; q < n_lps; ++q) {
        if (rows[q] < 1 || cols[q] < 2)
            return fail(MI_BAD_ARG, "member %lld: rows=%lld must be >= 1 and cols=%lld >= 2", (long long)q, (long long)rows[q],
                        (long long)cols[q]);
        if (rows[q] > 65535LL * 16) return fail(MI_BAD_ARG, "member %lld: rows=%lld exceeds the supported 1048560", (long long)q, (long long)rows[q]);
        if (cols[q] > (1LL << 30)) return fail(MI_BAD_ARG, "member %lld: cols=%lld exceeds the supported 2^30", (long long)q, (long long)cols[q]);
        n_basis += rows[q] - 1;
    }
    *n_basis_out = n_basis;
    return MI_OK;
}

// sr_new: a form-4 handle of those shapes and senses (is_max NULL: every member `min`) on `device`, WITHOUT the members'
// data -- the budget check per member (nothing is allocated before), the SrMember layout, the classes, the device
// buffers, the descriptors and class lists on their way up the handle's stream.  The caller fills v.M and v.basis
// (an upload, or an assembly kernel once this stream has been waited for), then calls sb_fresh_ctl, which waits for
// the stream; `index` (the class lists' host copy) has to live until then.  On a failure nothing is left behind.
int sr_new(mi355x_sbatch **out, int64_t n_lps, const int64_t *rows, const int64_t *cols, const int32_t *is_max, int64_t n_basis,
           int device, std::vector<int32_t> &index)
{
    HIP_TRY(hipSetDevice(device));
    // the same rule and the same budget as mi355x_sbatch_create, member by member (nothing is allocated before)
    std::vector<size_t> lds;
    try {
        lds.resize((size_t)n_lps);
    } catch (const std::bad_alloc &) {
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    for (int64_t q = 0; q < n_lps; ++q) {
        SView t{};
        t.rows = rows[q]; t.cols = cols[q];
        lds[q] = single_lds_bytes(t);
        if (lds[q] > kSingleLdsBudget)
            return fail(MI_UNSUPPORTED, "member %lld: a %lldx%lld single-float member does not fit the LDS budget of %lld bytes",
                        (long long)q, (long long)rows[q], (long long)cols[q], (long long)kSingleLdsBudget);
    }
    mi355x_sbatch *b = new (std::nothrow) mi355x_sbatch;
    if (!b) return fail(MI_NO_MEMORY, "host allocation failed");
    b->device = device;
    b->form = kSbFormRagged;
    b->threads = g_sbatch_threads ? g_sbatch_threads : 256;                 // (the measured rule: 256 inside the budget)
    b->launch_cap = g_sbatch_launch_cap ? g_sbatch_launch_cap : kSingleLaunchCap;
    const bool one_class = g_sbatch_ragged_classes != kSrMaxClass;         // (0: the default, measured: one class)
    if (!sragged_raise(b->threads)) {
        delete b;
        return fail(MI_UNSUPPORTED, "the dynamic LDS of the ragged batch kernels could not be raised to %lld bytes",
                    (long long)kSingleLdsBudget);
    }
    SbView &v = b->v;
    int64_t m_total = 0;
    try {
        b->hm.resize((size_t)n_lps);
        b->member_class.resize((size_t)n_lps);
        index.resize((size_t)n_lps);
        int64_t b_off = 0;
        for (int64_t q = 0; q < n_lps; ++q) {
            SrMember &d = b->hm[q];
            d.rows = rows[q]; d.cols = cols[q];
            d.ld = (cols[q] + kSingleLdAlign - 1) / kSingleLdAlign * kSingleLdAlign;
            d.m_off = m_total; d.basis_off = b_off;
            d.sgn = is_max && is_max[q] ? 1.0f : -1.0f;
            m_total += d.rows * d.ld;
            b_off += d.rows - 1;
            b->lds_max = std::max(b->lds_max, lds[q]);
        }
    } catch (const std::bad_alloc &) {
        delete b;
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    b->m_total = m_total;
    // the classes: one, every member at the largest member's size; under the hook the residency at the member's own
    // LDS size (queried once per distinct size), capped
    int count_of[kSrMaxClass + 1] = {0, 0, 0, 0, 0};       // members per residency
    try {
        std::map<size_t, int> seen;
        for (int64_t q = 0; q < n_lps; ++q) {
            const size_t bytes = one_class ? b->lds_max : lds[q];
            auto it = seen.find(bytes);
            if (it == seen.end()) {
                int nb = 0;
                if (!sragged_occupancy(b->threads, bytes, &nb) || nb < 1) {
                    delete b;
                    return fail(MI_UNSUPPORTED, "member %lld: no workgroup of %d threads with %lld bytes of LDS is resident",
                                (long long)q, b->threads, (long long)bytes);
                }
                it = seen.emplace(bytes, std::min(nb, kSrMaxClass)).first;
            }
            b->member_class[q] = it->second;               // (the residency for now; the class index below)
            ++count_of[it->second];
        }
        int class_of[kSrMaxClass + 1] = {-1, -1, -1, -1, -1};
        int64_t first = 0;
        for (int k = 1; k <= kSrMaxClass; ++k) {     // fewest resident = largest members first
            if (!count_of[k]) continue;
            class_of[k] = (int)b->classes.size();
            b->classes.push_back(SrClass{first, 0, 0, k});
            first += count_of[k];
        }
        for (int64_t q = 0; q < n_lps; ++q) {
            SrClass &c = b->classes[(size_t)class_of[b->member_class[q]]];
            b->member_class[q] = class_of[b->member_class[q]];
            index[(size_t)(c.first + c.count++)] = (int32_t)q;
            c.lds = std::max(c.lds, lds[q]);
        }
    } catch (const std::bad_alloc &) {
        delete b;
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    b->members_per_cu = b->classes.front().per_cu;          // the smallest class

    const int rc = sb_alloc(b, n_lps, m_total, n_basis, /*zero_tableaux=*/false, kSrUpload);
    if (rc != MI_OK) return rc;
    hipError_t e = hipMalloc((void **)&b->d_members, (size_t)n_lps * sizeof(SrMember));
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_index, (size_t)n_lps * sizeof(int32_t));
    if (e == hipSuccess)
        e = hipMemcpyAsync(b->d_members, b->hm.data(), (size_t)n_lps * sizeof(SrMember), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(b->d_index, index.data(), (size_t)n_lps * sizeof(int32_t), hipMemcpyHostToDevice, b->stream);
    if (e != hipSuccess) return sb_failed(b, nullptr, e, kSrUpload);
    SrView &r = b->r;
    r.M = v.M; r.basis = v.basis; r.ctl = v.ctl;
    r.trace_ec = v.trace_ec; r.trace_cr = v.trace_cr; r.trace_cap = v.trace_cap;
    r.n_lps = n_lps;
    r.members = b->d_members;
    *out = b;
    return MI_OK;
}

}  // namespace

extern "C" {

int mi355x_sbatch_create_ragged(mi355x_sbatch **out, int64_t n_lps, const int64_t *rows, const int64_t *cols,
                                const int32_t *is_max, const float *matrices, const int64_t *basis, int device)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (!rows || !cols) return fail(MI_BAD_ARG, "rows or cols is NULL");
    if (!matrices) return fail(MI_BAD_ARG, "matrices is NULL");
    int64_t n_basis = 0;
    int rc = sr_check_shapes(n_lps, rows, cols, &n_basis);
    if (rc != MI_OK) return rc;
    if (n_basis > 0 && !basis) return fail(MI_BAD_ARG, "basis is NULL");
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(MI_BAD_ARG, "device %d out of range [0,%d)", device, ndev);
    mi355x_sbatch *b = nullptr;
    std::vector<int32_t> index;
    rc = sr_new(&b, n_lps, rows, cols, is_max, n_basis, device, index);
    if (rc != MI_OK) return rc;
    std::vector<float> staged;                // the members as stored: rows of ld floats, padding zero
    try {
        staged.assign((size_t)b->m_total, 0.0f);
    } catch (const std::bad_alloc &) {
        free_sbatch(b);
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    {
        const float *src = matrices;
        for (int64_t q = 0; q < n_lps; ++q) {
            const SrMember &d = b->hm[q];
            for (int64_t r = 0; r < d.rows; ++r, src += d.cols)
                std::memcpy(staged.data() + d.m_off + r * d.ld, src, (size_t)d.cols * sizeof(float));
        }
    }
    SbView &v = b->v;
    hipError_t e = hipMemcpyAsync(v.M, staged.data(), (size_t)b->m_total * sizeof(float), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess && n_basis > 0)
        e = hipMemcpyAsync(v.basis, basis, (size_t)n_basis * sizeof(int64_t), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) e = sb_fresh_ctl(b);               // (waits for the stream: the staged copies are done)
    if (e != hipSuccess) return sb_failed(b, nullptr, e, kSrUpload);
    *out = b;
    return MI_OK;
}

int mi355x_sbatch_member_shape(const mi355x_sbatch *b, int64_t q, int64_t *rows, int64_t *cols, int64_t *ld, int32_t *is_max,
                               int *occupancy_class)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (q < 0 || q >= b->v.n_lps) return fail(MI_BAD_ARG, "lp_index %lld out of range [0,%lld)", (long long)q, (long long)b->v.n_lps);
    const bool ragged = b->form == kSbFormRagged;         // (one shape: the sense is the solve call's, one class)
    const SrMember d = sb_host_member(b, q);
    if (rows) *rows = d.rows;
    if (cols) *cols = d.cols;
    if (ld) *ld = d.ld;
    if (is_max) *is_max = !ragged ? -1 : d.sgn > 0.0f ? 1 : 0;
    if (occupancy_class) *occupancy_class = ragged ? b->classes[(size_t)b->member_class[(size_t)q]].per_cu : b->members_per_cu;
    return MI_OK;
}

int mi355x_tune_set_sbatch_ragged_classes(int classes)
{
    if (classes != 0 && classes != 1 && classes != kSrMaxClass)
        return fail(MI_BAD_ARG, "classes must be 0 (the default: one class), 1 (one class) or 4 (up to four occupancy classes)");
    g_sbatch_ragged_classes = classes;
    return MI_OK;
}

}  // extern "C"
