// capi_single_ragged_build.inc -- RAGGED single-float batches (form 4, capi_single_ragged.inc) whose tableaux the
// device builds: mi355x_sbatch_create_lps_ragged from the members' problem rows (build-tableau, src/simplex.lisp:243-328,
// under Lisp's int / single-float contagion), mi355x_sbatch_create_nodes_ragged from a branch-and-bound base and node
// rows of any depths (:214-221, :230-237), and mi355x_sbatch_readback_ragged, the light read-back (:74-107).
// The rules, the zero of a negated row and the 2^24 guard are those of capi_single_lps.inc and capi_single_bb.inc;
// the kernels are theirs, instantiated for a ragged view.  The handles are ordinary
// form-4 handles: sr_new makes them, every entry of capi_single_batch.inc works on them.
// All or none: either no member has artificial rows (*out_art = NULL), or every member has at least one -- the counts
// may differ -- and the result is a pair.  A mixture is MI_BAD_ARG; the caller splits its list.
// Part of simplex_capi.hip (ONE translation unit: included there after capi_single_lps.inc).

namespace {

// the pair of form-4 handles of main shapes (rows, cols) and artificial shapes (rows, acols) (two == false: no
// artificial batch) around an assembly: sb_pair_build behind the shapes' and the device's checks.  fill(stream, main
// view, artificial view) as for a pair of one shape.
template <class Fill>
int sr_pair_build(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n, const std::vector<int64_t> &rows,
                  const std::vector<int64_t> &cols, const std::vector<int64_t> &acols, const int32_t *is_max, bool two, int device,
                  const char *what, Fill fill)
{
    int64_t n_basis = 0;
    const int rc = sr_check_shapes(n, rows.data(), two ? acols.data() : cols.data(), &n_basis);
    if (rc != MI_OK) return rc;
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(MI_BAD_ARG, "device %d out of range [0,%d)", device, ndev);
    std::vector<int32_t> index_m, index_a;                                  // (alive until the streams have been waited for)
    return sb_pair_build(out_main, out_art, two, what, [&](mi355x_sbatch **h, bool artificial) {
        return artificial ? sr_new(h, n, rows.data(), acols.data(), nullptr, n_basis, device, index_a)
                          : sr_new(h, n, rows.data(), cols.data(), is_max, n_basis, device, index_m);
    }, [&](mi355x_sbatch *mt, mi355x_sbatch *art) { return fill(mt->stream, mt->r, art ? art->r : SrView{}); });
}

// the all-or-none rule: member q has n_art artificial rows, the members before it were `two` (-1: q is the first)
int sr_all_or_none(const char *member, int64_t q, int64_t n_art, int *two)
{
    const int mine = n_art > 0 ? 1 : 0;
    if (*two >= 0 && mine != *two)
        return fail(MI_BAD_ARG, "%s %lld has %lld artificial rows, the %ss before it %s: a ragged create takes members that "
                    "all have artificial rows or members that have none", member, (long long)q, (long long)n_art, member,
                    *two ? "have some" : "have none");
    *two = mine;
    return MI_OK;
}

int sr_budget_declined(const char *member, int64_t q, int64_t rows, int64_t cols)
{
    return fail(MI_UNSUPPORTED, "%s %lld: a %lldx%lld single-float member does not fit the LDS budget of %lld bytes", member,
                (long long)q, (long long)rows, (long long)cols, (long long)kSingleLdsBudget);
}

bool sr_fits(int64_t rows, int64_t cols)
{
    SView t{};
    t.rows = rows; t.cols = cols;
    return single_lds_bytes(t) <= kSingleLdsBudget;
}

}  // namespace

extern "C" {

int mi355x_sbatch_create_lps_ragged(mi355x_sbatch **out_main, mi355x_sbatch **out_art, int64_t n_lps, const int64_t *m,
                                    const int64_t *ncv, const int32_t *is_max, const float *lps, const int32_t *sense,
                                    const double *col_int_sum, int device)
{
    if (!out_main || !out_art) return fail(MI_BAD_ARG, "out is NULL");
    *out_main = *out_art = nullptr;
    if (!m || !ncv || !is_max) return fail(MI_BAD_ARG, "m, ncv or is_max is NULL");
    if (!lps) return fail(MI_BAD_ARG, "lps is NULL");
    if (!sense) return fail(MI_BAD_ARG, "sense is NULL");
    if (n_lps < 1 || n_lps > (1LL << 30)) return fail(MI_BAD_ARG, "n_lps=%lld must be in [1, 2^30]", (long long)n_lps);
    std::vector<int64_t> rows, cols, acols;
    std::vector<SrlpMember> desc;
    try {
        rows.resize((size_t)n_lps); cols.resize((size_t)n_lps); acols.resize((size_t)n_lps); desc.resize((size_t)n_lps);
    } catch (const std::bad_alloc &) {
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    int two = -1;
    int64_t l_off = 0, s_off = 0;
    for (int64_t q = 0; q < n_lps; ++q) {
        if (m[q] < 1 || ncv[q] < 1)
            return fail(MI_BAD_ARG, "member %lld: m=%lld ncv=%lld must be >= 1", (long long)q, (long long)m[q], (long long)ncv[q]);
        if (m[q] > (1 << 24) || ncv[q] > (1 << 24))
            return fail(MI_BAD_ARG, "member %lld: m=%lld ncv=%lld out of range", (long long)q, (long long)m[q], (long long)ncv[q]);
        int64_t n_eq = 0, n_art = 0;
        int rc = lps_member_counts(q, m[q], ncv[q], lps + l_off, sense + s_off, &n_eq, &n_art);
        if (rc == MI_OK) rc = sr_all_or_none("member", q, n_art, &two);
        if (rc != MI_OK) return rc;
        rows[q] = m[q] + 1;
        cols[q] = ncv[q] + (m[q] - n_eq) + 1;
        acols[q] = cols[q] + n_art;
        desc[q] = SrlpMember{l_off, s_off, (int32_t)m[q], (int32_t)ncv[q], (int32_t)(m[q] - n_eq), (int32_t)n_art};
        l_off += (m[q] + 1) * (ncv[q] + 1);
        s_off += m[q];
    }
    const double *sums = col_int_sum;                                       // the guard (NULL: no entry is an integer)
    for (int64_t q = 0; sums && q < n_lps; sums += ncv[q] + 1, ++q)
        if (slp_guard(q, ncv[q], sums) != MI_OK) return MI_UNSUPPORTED;
    for (int64_t q = 0; q < n_lps; ++q)                                     // (a two-phase member: its artificial shape)
        if (m[q] > kSlpMaxRows || !sr_fits(rows[q], two ? acols[q] : cols[q]))
            return sr_budget_declined("member", q, rows[q], two ? acols[q] : cols[q]);
    SbDeviceMem d;
    return sr_pair_build(out_main, out_art, n_lps, rows, cols, acols, is_max, two == 1, device, "ragged assembly from rows",
                         [&](hipStream_t s, const SrView &mv, const SrView &av) {
        const size_t bL = (size_t)l_off * sizeof(float), bS = (size_t)s_off * sizeof(int32_t), bD = (size_t)n_lps * sizeof(SrlpMember);
        const size_t oS = sb_align(bL), oD = sb_align(oS + bS);
        hipError_t e = hipMalloc(&d.mem, oD + bD);
        if (e == hipSuccess) e = hipMemcpyAsync(d.mem, lps, bL, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync((char *)d.mem + oS, sense, bS, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync((char *)d.mem + oD, desc.data(), bD, hipMemcpyHostToDevice, s);
        if (e == hipSuccess)
            launch_slp_assemble(mv, av, SrlpView{(const float *)d.mem, (const int32_t *)((const char *)d.mem + oS),
                                                 (const SrlpMember *)((const char *)d.mem + oD)}, s);
        return e;
    });
}

int mi355x_sbatch_create_nodes_ragged(mi355x_sbatch **out_main, mi355x_sbatch **out_art, const mi355x_sbb_base *base,
                                      int64_t n_nodes, const int64_t *depth, const int64_t *var, const int32_t *sense,
                                      const int64_t *bound)
{
    if (!out_main || !out_art) return fail(MI_BAD_ARG, "out is NULL");
    *out_main = *out_art = nullptr;
    if (!base || n_nodes < 1 || !depth || !var || !sense || !bound) return fail(MI_BAD_ARG, "bad counts or NULL array");
    if (n_nodes > (1 << 24)) return fail(MI_BAD_ARG, "shape out of range");
    const SbbBase &b = *base->p;
    // a form-4 handle carries the sense per member (mi355x_sbatch_solve takes -1 there): every node has the base's
    if (b.is_max < 0) return fail(MI_BAD_ARG, "the base has no sense yet: call mi355x_sbb_base_set_sense first");
    std::vector<int64_t> rows, cols, acols;
    std::vector<SrbbNode> desc;
    std::vector<int32_t> senses;
    std::vector<double> extra;
    try {
        rows.resize((size_t)n_nodes); cols.resize((size_t)n_nodes); acols.resize((size_t)n_nodes); desc.resize((size_t)n_nodes);
        senses.assign((size_t)n_nodes, 0);
        extra.assign((size_t)b.cols, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(MI_NO_MEMORY, "host allocation failed");
    }
    bool base_exact = true;
    for (int64_t c = 0; c < b.cols; ++c) base_exact = base_exact && b.col_int_sum[c] <= kSbbExactInts;
    int two = -1;
    int64_t off = 0, inexact = -1, lds_declined = -1, budget_declined = -1;
    size_t lds = 0;
    for (int64_t q = 0; q < n_nodes; ++q) {
        if (depth[q] < 1 || depth[q] > (1 << 24)) return fail(MI_BAD_ARG, "node %lld: depth=%lld out of range", (long long)q, (long long)depth[q]);
        int64_t n_art = 0;
        bool exact = base_exact;
        int rc = sbb_node_check(b, off, depth[q], var, sense, bound, extra, &n_art, &exact);
        if (rc == MI_OK) rc = sr_all_or_none("node", q, n_art, &two);
        if (rc != MI_OK) return rc;
        if (!exact && inexact < 0) inexact = q;
        rows[q] = b.rows + depth[q];
        cols[q] = b.cols + depth[q];
        acols[q] = cols[q] + n_art;
        desc[q] = SrbbNode{off, (int32_t)depth[q]};
        const size_t bytes = sbb_assemble_lds(rows[q] - 1, depth[q]);
        if (bytes > kSbbAssembleLdsLimit && lds_declined < 0) lds_declined = q;
        if (!sr_fits(rows[q], two ? acols[q] : cols[q]) && budget_declined < 0) budget_declined = q;
        lds = std::max(lds, bytes);
        off += depth[q];
    }
    // (every MI_BAD_ARG above comes first, as in mi355x_sbatch_create_nodes; nothing has been allocated)
    if (inexact >= 0)
        return fail(MI_UNSUPPORTED, "node %lld: a column's integer entries sum beyond 2^24: the float sum of the artificial "
                                    "objective row would not be the reference's", (long long)inexact);
    if (lds_declined >= 0)
        return fail(MI_UNSUPPORTED, "node %lld: %lld rows at depth %lld do not fit the assembly's LDS", (long long)lds_declined,
                    (long long)rows[lds_declined], (long long)depth[lds_declined]);
    if (budget_declined >= 0)
        return sr_budget_declined("node", budget_declined, rows[budget_declined], (two ? acols : cols)[budget_declined]);
    for (int64_t q = 0; q < n_nodes; ++q) senses[q] = b.is_max;
    SbDeviceMem d;
    return sr_pair_build(out_main, out_art, n_nodes, rows, cols, acols, senses.data(), two == 1, b.device, "ragged node assembly",
                         [&](hipStream_t s, const SrView &mv, const SrView &av) {
        const size_t nk = (size_t)off;
        const size_t oB = sb_align(nk * sizeof(int64_t)), oS = oB + sb_align(nk * sizeof(int64_t));
        const size_t oD = oS + sb_align(nk * sizeof(int32_t)), bD = (size_t)n_nodes * sizeof(SrbbNode);
        hipError_t e = hipMalloc(&d.mem, oD + bD);
        char *p = (char *)d.mem;
        if (e == hipSuccess) e = hipMemcpyAsync(p, var, nk * sizeof(int64_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p + oB, bound, nk * sizeof(int64_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p + oS, sense, nk * sizeof(int32_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p + oD, desc.data(), bD, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            const SbbBaseView bv{b.d_B, b.d_off, b.rows, b.cols, b.ncv, b.nb, b.d_basis, b.d_kind, b.d_vcol};
            launch_sbb_assemble(mv, av, bv, SrbbNodeRows{(const int64_t *)p, (const int32_t *)(p + oS), (const int64_t *)(p + oB),
                                                         (const SrbbNode *)(p + oD)}, lds, s);
        }
        return e;
    });
}

int mi355x_sbatch_readback_ragged(mi355x_sbatch *b, float *rhs, float *obj_row, int64_t *basis)
{
    if (!b) return fail(MI_BAD_ARG, "handle is NULL");
    if (!rhs || !obj_row) return fail(MI_BAD_ARG, "rhs or obj_row is NULL");
    if (b->form != kSbFormRagged)
        return fail(MI_UNSUPPORTED, "mi355x_sbatch_readback_ragged gathers a ragged batch (form 4): on a batch of one shape "
                                    "(form %d) call mi355x_sbatch_readback", b->form);
    const int64_t n = b->v.n_lps;
    int64_t n_rows = 0, n_cols = 0;
    for (int64_t q = 0; q < n; ++q) { n_rows += b->hm[q].rows; n_cols += b->hm[q].cols; }
    if (n_rows - n > 0 && !basis) return fail(MI_BAD_ARG, "basis is NULL");
    return sb_readback(b, n_rows, n_cols, rhs, obj_row, basis);
}

}  // extern "C"
