// capi_bb.inc -- branch-and-bound node batches assembled on the devices (kernels_bb.inc); internal to
// the library: host_bb.inc (the search) calls these through the `_`-suffixed names below.
struct mi355x_bb_base {
    // host copy of the base problem's general-form main tableau and what the kernels read with it
    int64_t rows = 0, cols = 0, ncv = 0, nb = 0, n_vars = 0;
    std::vector<double>  M;
    std::vector<int32_t> flip, kind;
    std::vector<int64_t> basis, vcol;
    std::vector<double>  voff;
    struct Dev { int device = -1; void *mem = nullptr; BBBaseView v{}; };
    std::vector<Dev> dev;                     // uploaded once per device, on first use
    ~mi355x_bb_base() { for (Dev &d : dev) { (void)hipSetDevice(d.device); (void)hipFree(d.mem); } }
};

extern "C" __attribute__((visibility("hidden"))) int mi355x_bb_base_create_(mi355x_bb_base **out, int64_t rows, int64_t cols, const double *M,
                                      const int32_t *flip, const int64_t *basis, int64_t ncv, int64_t nb,
                                      int64_t n_vars, const int32_t *kind, const int64_t *vcol, const double *voff)
{
    mi355x_bb_base *b = new (std::nothrow) mi355x_bb_base;
    if (!b) return fail(MI_NO_MEMORY, "host allocation failed");
    b->rows = rows; b->cols = cols; b->ncv = ncv; b->nb = nb; b->n_vars = n_vars;
    b->M.assign(M, M + rows * cols);
    b->flip.assign(flip, flip + (rows - 1)); b->basis.assign(basis, basis + (rows - 1));
    b->kind.assign(kind, kind + n_vars); b->vcol.assign(vcol, vcol + n_vars); b->voff.assign(voff, voff + n_vars);
    *out = b;
    return MI_OK;
}

extern "C" __attribute__((visibility("hidden"))) void mi355x_bb_base_destroy_(mi355x_bb_base *b) { delete b; }

static int bb_base_on(mi355x_bb_base *b, int device, hipStream_t s, BBBaseView *out)
{
    for (auto &d : b->dev) if (d.device == device) { *out = d.v; return MI_OK; }
    const int64_t m = b->rows - 1, nv = b->n_vars;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t oM = 0, oF = al(oM + b->M.size() * 8), oB = al(oF + m * 4 + 4), oK = al(oB + m * 8 + 8),
                 oC = al(oK + nv * 4), oO = al(oC + nv * 8), total = al(oO + nv * 8);
    mi355x_bb_base::Dev d;
    d.device = device;
    HIP_TRY(hipMalloc(&d.mem, total));
    char *p = (char *)d.mem;
    HIP_TRY(hipMemcpyAsync(p + oM, b->M.data(), b->M.size() * 8, hipMemcpyHostToDevice, s));
    if (m > 0) {
        HIP_TRY(hipMemcpyAsync(p + oF, b->flip.data(), m * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(p + oB, b->basis.data(), m * 8, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(p + oK, b->kind.data(), nv * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p + oC, b->vcol.data(), nv * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(p + oO, b->voff.data(), nv * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    d.v = BBBaseView{(const double *)(p + oM), b->rows, b->cols, b->ncv, b->nb, (const int32_t *)(p + oF),
                     (const int64_t *)(p + oB), (const int32_t *)(p + oK), (const int64_t *)(p + oC),
                     (const double *)(p + oO)};
    b->dev.push_back(d);
    *out = d.v;
    return MI_OK;
}

// n nodes of depth d >= 1 and n_art artificial rows each, node k's rows at var/sense/bound[k*d ..]:
// their main tableaux (and, n_art > 0, artificial tableaux) as multibatches over n_devices devices,
// written by launch_node_assemble.  Every node must have exactly n_art artificial rows (the caller groups).
extern "C" __attribute__((visibility("hidden"))) int mi355x_bb_assemble_(mi355x_bb_base *b, int64_t n, int64_t d, const int64_t *var, const int32_t *sense,
                                   const double *bound, int64_t n_art, int n_devices, const int *device_ids,
                                   mi355x_multibatch **main_out, mi355x_multibatch **art_out)
{
    *main_out = nullptr; if (art_out) *art_out = nullptr;
    if (!b || n < 1 || d < 1 || !var || !sense || !bound || n_art < 0) return fail(MI_BAD_ARG, "bad arguments");
    for (int64_t i = 0; i < n * d; ++i)
        if (var[i] < 0 || var[i] >= b->n_vars || sense[i] < 0 || sense[i] > 1) return fail(MI_BAD_ARG, "bad node row");
    const int64_t rows = b->rows + d, cols = b->cols + d;
    return multibatch_pair_build(main_out, art_out, n, rows, cols, n_art, n_devices, device_ids,
                                 [&](mi355x_tab *t[2], int64_t k0, int64_t count, int device) {
        const size_t nrow = (size_t)count * d;
        return tab_pair_build(t, count, rows, cols, n_art, device, nrow * (8 + 4 + 8) + (size_t)count * (rows - 1) * 4 + 64,
                              [&](hipStream_t st, const TabView &mv, const TabView &av, char *p) {
            BBBaseView bv{};
            const int rc = bb_base_on(b, device, st, &bv);
            if (rc != MI_OK) return rc;
            int64_t *dv = (int64_t *)p; double *db = (double *)(p + nrow * 8); int32_t *ds = (int32_t *)(p + nrow * 16);
            int32_t *scratch = (int32_t *)(p + ((nrow * 20 + 63) & ~(size_t)63));
            HIP_TRY(hipMemcpyAsync(dv, var + k0 * d, nrow * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(db, bound + k0 * d, nrow * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ds, sense + k0 * d, nrow * 4, hipMemcpyHostToDevice, st));
            launch_node_assemble(mv, av, bv, BBNodeRows{dv, ds, db, d, 0}, scratch, st);
            return (int)MI_OK;
        });
    });
}
