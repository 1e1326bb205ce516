// capi_single_bb.inc -- single-float branch-and-bound (simplex-solver in single-float, src/simplex.lisp:462-542):
// node batches assembled on the device and the light read-back.  Part of simplex_capi.hip (ONE translation unit:
// included there after capi_single_batch.inc, whose handle, sb_pair_build, SbDeviceMem and sb_readback it uses).
//
// The search itself, build-tableau of the base problem (with Lisp's contagion) and the reading of a solution stay in
// the host language; the library turns (base, node rows) into the members of two mi355x_sbatch handles
// (k_sbb_assemble) and gathers what the read-back functions need (k_sb_readback).
//
// The guard.  Lisp sums the artificial objective row (:302-316) with integers exact among themselves; the kernel
// sums floats.  The two agree when every integer partial sum is exact in a float, which holds while the sum of the
// absolute values of a column's integer entries is at most 2^24.  The base hands in that sum per column
// (col_int_sum, over its constraint rows); a node row adds 1 in its variable's column(s) and its own slack column and
// |rhs| in the last column (counted whenever rhs is integer-valued).  A group with a column beyond 2^24 is declined
// (MI_UNSUPPORTED): the host builds those nodes itself.

struct SbbBase {
    int      device = 0;
    int64_t  rows = 0, cols = 0, ncv = 0, nb = 0, n_vars = 0, n_art = 0;
    int      is_max = -1;             // mi355x_sbb_base_set_sense (ragged node batches carry the sense per member); -1: not said
    std::vector<int64_t> vcol;
    std::vector<int32_t> kind;
    std::vector<float>   off;
    std::vector<double>  col_int_sum;
    float   *d_B = nullptr, *d_off = nullptr;
    int64_t *d_basis = nullptr, *d_vcol = nullptr;
    int32_t *d_kind = nullptr;
    ~SbbBase()
    {
        (void)hipSetDevice(device);
        (void)hipFree(d_B); (void)hipFree(d_off); (void)hipFree(d_basis); (void)hipFree(d_vcol); (void)hipFree(d_kind);
    }
};

struct mi355x_sbb_base { std::unique_ptr<SbbBase> p; };

namespace {

constexpr double kSbbExactInts = 16777216.0;                                // 2^24
constexpr size_t kSbbAssembleLdsLimit = 48 * 1024;                          // k_sbb_assemble's dynamic LDS, never raised

// a node row's right-hand side as k_sbb_assemble computes it (one float subtraction)
inline float sbb_rhs(const SbbBase &b, int64_t var, int64_t bound)
{
    const float f = (float)bound;
    return b.kind[var] == 2 ? f : f - b.off[var];
}

}  // namespace

extern "C" {

int mi355x_sbb_base_create(mi355x_sbb_base **out, int64_t rows, int64_t cols, const float *matrix, const int64_t *basis,
                           int64_t ncv, int64_t nb, int64_t n_vars, const int32_t *kind, const int64_t *col,
                           const float *offset, const double *col_int_sum, int device)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (rows < 1 || cols < 1 || !matrix || (rows > 1 && !basis) || n_vars < 1 || !kind || !col || !offset || !col_int_sum)
        return fail(MI_BAD_ARG, "bad shape or NULL array");
    if (rows > (1 << 24) || cols > (1 << 24) || n_vars > cols) return fail(MI_BAD_ARG, "shape out of range");
    if (ncv < n_vars || nb < 0 || nb > rows - 1 || ncv + nb > cols - 1) return fail(MI_BAD_ARG, "bad column or row counts");
    for (int64_t v = 0; v < n_vars; ++v)
        if (kind[v] < 0 || kind[v] > 2 || col[v] < 0 || col[v] + (kind[v] == 2 ? 1 : 0) >= ncv)
            return fail(MI_BAD_ARG, "bad mapping of variable %lld", (long long)v);
    for (int64_t i = 0; i < rows - 1; ++i)
        if (basis[i] < 0 || basis[i] > cols) return fail(MI_BAD_ARG, "basis entry %lld out of range", (long long)i);
    for (int64_t c = 0; c < cols; ++c)
        if (!(col_int_sum[c] >= 0)) return fail(MI_BAD_ARG, "col_int_sum[%lld] is not a sum of absolute values", (long long)c);
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(MI_BAD_ARG, "device %d out of range [0,%d)", device, ndev);
    std::unique_ptr<SbbBase> b(new (std::nothrow) SbbBase);
    if (!b) return fail(MI_NO_MEMORY, "host allocation failed");
    b->device = device;
    b->rows = rows; b->cols = cols; b->ncv = ncv; b->nb = nb; b->n_vars = n_vars;
    b->kind.assign(kind, kind + n_vars);
    b->vcol.assign(col, col + n_vars);
    b->off.assign(offset, offset + n_vars);
    b->col_int_sum.assign(col_int_sum, col_int_sum + cols);
    const int64_t m = rows - 1;
    for (int64_t i = 0; i < m; ++i) b->n_art += basis[i] == cols;
    HIP_TRY(hipSetDevice(device));
    if (hipMalloc((void **)&b->d_B, (size_t)(rows * cols) * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&b->d_off, n_vars * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&b->d_basis, std::max<int64_t>(m, 1) * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void **)&b->d_vcol, n_vars * sizeof(int64_t)) != hipSuccess ||
        hipMalloc((void **)&b->d_kind, n_vars * sizeof(int32_t)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MI_NO_MEMORY, "device allocation failed");
    }
    HIP_TRY(hipMemcpy(b->d_B, matrix, (size_t)(rows * cols) * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_off, offset, n_vars * sizeof(float), hipMemcpyHostToDevice));
    if (m > 0) HIP_TRY(hipMemcpy(b->d_basis, basis, m * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_vcol, col, n_vars * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->d_kind, kind, n_vars * sizeof(int32_t), hipMemcpyHostToDevice));
    mi355x_sbb_base *h = new (std::nothrow) mi355x_sbb_base;
    if (!h) return fail(MI_NO_MEMORY, "host allocation failed");
    h->p = std::move(b);
    *out = h;
    return MI_OK;
}

void mi355x_sbb_base_destroy(mi355x_sbb_base *base) { delete base; }

int mi355x_sbb_base_set_sense(mi355x_sbb_base *base, int is_max)
{
    if (!base) return fail(MI_BAD_ARG, "base is NULL");
    if (is_max != 0 && is_max != 1) return fail(MI_BAD_ARG, "is_max=%d must be 0 (min) or 1 (max)", is_max);
    base->p->is_max = is_max;
    return MI_OK;
}

}  // extern "C"

namespace {

// one node's rows [k0, k0 + depth) of var / sense / bound: the argument check, *n_art its artificial rows with the
// base's, and the guard -- this node's integer entries on top of the base's, column by column (extra: one zero per
// base column, left as it was found); *exact_sums is cleared where a column goes beyond 2^24
int sbb_node_check(const SbbBase &b, int64_t k0, int64_t depth, const int64_t *var, const int32_t *sense, const int64_t *bound,
                   std::vector<double> &extra, int64_t *n_art, bool *exact)
{
    bool exact_sums = *exact;
    int64_t a = b.n_art;
    for (int64_t k = k0; k < k0 + depth; ++k) {
        if (var[k] < 0 || var[k] >= b.n_vars || sense[k] < 0 || sense[k] > 1 || bound[k] == INT64_MIN)
            return fail(MI_BAD_ARG, "bad node row %lld", (long long)k);
        const float rhs = sbb_rhs(b, var[k], bound[k]);
        a += row_word_artificial(row_word(rhs < 0.0f, sense[k]));
        const int64_t c = b.vcol[var[k]];
        const double r = std::fabs((double)rhs);
        extra[c] += 1.0;
        if (b.kind[var[k]] == 2) extra[c + 1] += 1.0;
        if (r == std::floor(r)) extra[b.cols - 1] += r;
    }
    for (int64_t k = k0; k < k0 + depth; ++k) {
        const int64_t c = b.vcol[var[k]];
        exact_sums = exact_sums && b.col_int_sum[c] + extra[c] <= kSbbExactInts;
        if (b.kind[var[k]] == 2) exact_sums = exact_sums && b.col_int_sum[c + 1] + extra[c + 1] <= kSbbExactInts;
    }
    exact_sums = exact_sums && b.col_int_sum[b.cols - 1] + extra[b.cols - 1] <= kSbbExactInts;
    for (int64_t k = k0; k < k0 + depth; ++k) {
        const int64_t c = b.vcol[var[k]];
        extra[c] = 0.0;
        if (b.kind[var[k]] == 2) extra[c + 1] = 0.0;
    }
    extra[b.cols - 1] = 0.0;
    *n_art = a;
    *exact = exact_sums;
    return MI_OK;
}

// mi355x_sbatch_create_nodes / _create_nodes_global: the checks, the guard, the pair of the form, the assembly
int sbb_create_nodes(mi355x_sbatch **out_main, mi355x_sbatch **out_art, const mi355x_sbb_base *base, int64_t n_nodes,
                     int64_t depth, const int64_t *var, const int32_t *sense, const int64_t *bound, int form)
{
    if (!out_main || !out_art) return fail(MI_BAD_ARG, "out is NULL");
    *out_main = *out_art = nullptr;
    if (!base || n_nodes < 1 || depth < 1 || !var || !sense || !bound) return fail(MI_BAD_ARG, "bad counts or NULL array");
    if (n_nodes > (1 << 24) || depth > (1 << 24)) return fail(MI_BAD_ARG, "shape out of range");
    const SbbBase &b = *base->p;
    int64_t n_art = -1;
    bool exact_sums = true;
    std::vector<double> extra;
    try {
        extra.assign((size_t)b.cols, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    for (int64_t c = 0; c < b.cols; ++c) exact_sums = exact_sums && b.col_int_sum[c] <= kSbbExactInts;
    for (int64_t q = 0; q < n_nodes; ++q) {
        int64_t a = 0;
        const int rc = sbb_node_check(b, q * depth, depth, var, sense, bound, extra, &a, &exact_sums);
        if (rc != MI_OK) return rc;
        if (n_art >= 0 && a != n_art) return fail(MI_BAD_ARG, "the nodes have different numbers of artificial rows");
        n_art = a;
    }
    if (!exact_sums)
        return fail(MI_UNSUPPORTED, "a column's integer entries sum beyond 2^24: the float sum of the artificial "
                                    "objective row would not be the reference's");
    const int64_t rows = b.rows + depth, cols = b.cols + depth;
    if (form == kSbFormLds && sbb_assemble_lds(rows - 1, depth) > kSbbAssembleLdsLimit)
        return fail(MI_UNSUPPORTED, "%lld rows at depth %lld do not fit the assembly's LDS", (long long)rows, (long long)depth);
    SbDeviceMem nd;                                                         // var, bound, sense, the global form's scratch planes
    return sb_pair_build(out_main, out_art, n_nodes, rows, cols, n_art, b.device, "node assembly",
                         [&](hipStream_t s, const SbView &mv, const SbView &av) {
        const size_t nk = (size_t)(n_nodes * depth);
        const size_t oB = sb_align(nk * sizeof(int64_t)), oS = oB + sb_align(nk * sizeof(int64_t));
        const size_t oW = oS + sb_align(nk * sizeof(int32_t));
        hipError_t e = hipMalloc(&nd.mem, form == kSbFormGlobal ? oW + sga_nodes_scratch_bytes(n_nodes, rows - 1) : oW);
        char *p = (char *)nd.mem;
        if (e == hipSuccess) e = hipMemcpyAsync(p, var, nk * sizeof(int64_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p + oB, bound, nk * sizeof(int64_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p + oS, sense, nk * sizeof(int32_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            const SbbBaseView bv{b.d_B, b.d_off, b.rows, b.cols, b.ncv, b.nb, b.d_basis, b.d_kind, b.d_vcol};
            const XbbNodeRows nr{(const int64_t *)p, (const int32_t *)(p + oS), (const int64_t *)(p + oB), depth};
            if (form == kSbFormGlobal) launch_sga_nodes(mv, av, bv, nr, (int32_t *)(p + oW), s);
            else launch_sbb_assemble(mv, av, bv, nr, s);
        }
        return e;
    }, form);
}

}  // namespace

extern "C" {

int mi355x_sbatch_create_nodes(mi355x_sbatch **out_main, mi355x_sbatch **out_art, const mi355x_sbb_base *base,
                               int64_t n_nodes, int64_t depth, const int64_t *var, const int32_t *sense,
                               const int64_t *bound)
{
    return sbb_create_nodes(out_main, out_art, base, n_nodes, depth, var, sense, bound, kSbFormLds);
}

int mi355x_sbatch_create_nodes_global(mi355x_sbatch **out_main, mi355x_sbatch **out_art, const mi355x_sbb_base *base,
                                      int64_t n_nodes, int64_t depth, const int64_t *var, const int32_t *sense,
                                      const int64_t *bound)
{
    return sbb_create_nodes(out_main, out_art, base, n_nodes, depth, var, sense, bound, kSbFormGlobal);
}

int mi355x_sbatch_readback(mi355x_sbatch *b, float *rhs, float *obj_row, int64_t *basis)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (!rhs || !obj_row) return fail(MI_BAD_ARG, "rhs or obj_row is NULL");
    if (b->form == kSbFormRagged)
        return fail(MI_UNSUPPORTED, "mi355x_sbatch_readback gathers planes of one shape: not on a ragged batch (form 4)");
    const SbView &v = b->v;
    if (v.rows > 1 && !basis) return fail(MI_BAD_ARG, "basis is NULL");
    return sb_readback(b, v.n_lps * v.rows, v.n_lps * v.cols, rhs, obj_row, basis);
}

}  // extern "C"
