// kernels_launch.inc -- host-side launchers and tuning state.
// Part of simplex_kernels.hip (ONE translation unit: included there, in this order, inside namespace mi355x).

// ------------------------------------------------------------------ host-side launchers
static inline double sgn_of(int is_max) { return is_max ? 1.0 : -1.0; }

void launch_select(const TabView &t, int is_max, double f, int n_part, hipStream_t s)
{
    // one workgroup per tableau; a narrow workgroup when there is little to do per phase (its
    // barriers and reductions are the cost): measured on config 2, 10.3 us with 1024 threads
    const dim3 grid(1, 1, (unsigned)t.n_lps);
    const double ptol = (f / 8.0) * kClEpsilon, rthr = 0.0 + (f / 2.0) * kClEpsilon;
    if (t.rows <= 2048 && t.ld <= 4096)
        hipLaunchKernelGGL(k_select<256>, grid, dim3(256), 0, s, t, sgn_of(is_max), ptol, rthr, n_part);
    else
        hipLaunchKernelGGL(k_select<kSelThreads>, grid, dim3(kSelThreads), 0, s, t, sgn_of(is_max),
                           ptol, rthr, n_part);
}
void launch_select_split(const TabView &t, int is_max, double f, int n_part, hipStream_t s)
{
    const int g1 = (int)((t.rows + kGatherThreads - 1) / kGatherThreads);
    const int g2 = (int)(((t.ld >> 1) + kScaleThreads - 1) / kScaleThreads);
    hipLaunchKernelGGL(k_select_gather, dim3(g1, 1, (unsigned)t.n_lps), dim3(kGatherThreads), 0, s, t,
                       sgn_of(is_max), (f / 8.0) * kClEpsilon, 0.0 + (f / 2.0) * kClEpsilon, n_part);
    hipLaunchKernelGGL(k_select_scale, dim3(g2, 1, (unsigned)t.n_lps), dim3(kScaleThreads), 0, s, t, g1,
                       0.0 + (f / 2.0) * kClEpsilon);
}
bool select_split_supported(const TabView &t)
{
    return (t.rows + kGatherThreads - 1) / kGatherThreads <= t.part_cap / 2;
}
void launch_price_only(const TabView &t, int is_max, double f, hipStream_t s)
{
    hipLaunchKernelGGL(k_price_only, dim3(1), dim3(kSelThreads), 0, s, t, sgn_of(is_max),
                       (f / 8.0) * kClEpsilon, (int64_t)0, (double *)nullptr, 0, P2pArgs());
}
void launch_ratio_only(const TabView &t, int64_t ec, double f, hipStream_t s)
{
    hipLaunchKernelGGL(k_ratio_only, dim3(1), dim3(kSelThreads), 0, s, t, ec,
                       0.0 + (f / 2.0) * kClEpsilon);
}
void launch_prepare_pivot(const TabView &t, int64_t ec, int64_t cr, hipStream_t s)
{
    hipLaunchKernelGGL(k_prepare_pivot, dim3(1), dim3(kSelThreads), 0, s, t, ec, cr);
}
void launch_shard_price(const TabView &t, int is_max, int64_t col_offset, double *out2, int n_part,
                        hipStream_t s, const P2pArgs &x)
{
    hipLaunchKernelGGL(k_price_only, dim3(1), dim3(kSelThreads), 0, s, t, sgn_of(is_max), 0.0,
                       col_offset, out2, n_part, x);
}
void launch_shard_contribute(const TabView &t, const double *gathered, int n_shards,
                             int64_t col_offset, double f, int64_t *bits_out, int64_t *ec_out,
                             hipStream_t s)
{
    int blocks = (int)((t.rows + kSelThreads - 1) / kSelThreads);
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(k_shard_contribute, dim3(blocks), dim3(kSelThreads), 0, s, t, gathered,
                       n_shards, col_offset, (f / 8.0) * kClEpsilon, (long long *)bits_out, ec_out);
}
void launch_shard_prepare(const TabView &t, const double *col, const int64_t *ec_dev, double f,
                          hipStream_t s, int64_t forced_cr)
{
    hipLaunchKernelGGL(k_shard_prepare, dim3(1), dim3(kSelThreads), 0, s, t, col, ec_dev,
                       0.0 + (f / 2.0) * kClEpsilon, forced_cr);
}
void launch_shard_forced_contribute(const TabView &t, int64_t ec, int64_t col_offset, int64_t *bits_out,
                                    int64_t *ec_out, hipStream_t s)
{
    int blocks = (int)((t.rows + kSelThreads - 1) / kSelThreads);
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(k_shard_forced_contribute, dim3(blocks), dim3(kSelThreads), 0, s, t, ec, col_offset,
                       (long long *)bits_out, ec_out);
}
void launch_shard_handover(const TabView &art, const TabView &mt, const int64_t *keep, const double *obj0,
                           const double *scales, hipStream_t s)
{
    hipLaunchKernelGGL(k_shard_handover, dim3((unsigned)((mt.cols + 255) / 256)), dim3(256), 0, s, art, mt,
                       keep, obj0, scales);
}
void launch_shard_la_contribute(const TabView &t, int j, const double *gathered, int n_shards,
                                int64_t col_offset, double f, int64_t *bits_out, int64_t *ec_out,
                                hipStream_t s, const P2pArgs &x)
{
    // 256-thread workgroups, one row per thread: the strided gather of the entering column (a 64-byte
    // sector per row) needs many workgroups' memory pipelines (33 x 1024 threads: 12.5 us at 32769 rows)
    int blocks = (int)((t.rows + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_shard_la_contribute, dim3(blocks), dim3(256), 0, s, t, j, gathered,
                       n_shards, col_offset, (f / 8.0) * kClEpsilon, (long long *)bits_out, ec_out, x);
}
static int g_shard_la_split = 0;                     // 0 by size, 1 always one workgroup, 2 always split
void set_shard_la_split(int mode) { g_shard_la_split = mode; }

template <int J>
static void launch_shard_la_scale_t(const TabView &t, int g2, int g1, const int64_t *ec_dev, int is_max, hipStream_t s)
{
    hipLaunchKernelGGL(k_shard_la_scale<J>, dim3(g2), dim3(kScaleThreads), 0, s, t, g1, ec_dev, sgn_of(is_max));
}

bool shard_la_split(const TabView &t)
{
    const int g1 = (int)((t.rows + kGatherThreads - 1) / kGatherThreads);
    const int g2 = (int)(((t.ld >> 1) + kScaleThreads - 1) / kScaleThreads);
    const bool fits = g1 <= t.part_cap / 2 && g2 * (kScaleThreads / 64) <= t.part_cap / 2;
    return fits && (g_shard_la_split == 2 || (g_shard_la_split == 0 && (t.rows > 4096 || t.ld > 8192)));
}

// (x.peers != nullptr is honoured by the split form only: the caller checks shard_la_split())
int launch_shard_la_prepare(const TabView &t, int j, const double *col, const int64_t *ec_dev, double f,
                            int is_max, hipStream_t s, const P2pArgs &x)
{
    // one workgroup for small shards (one launch, ~10 us), the split pair for large ones (rows or
    // column pairs in the tens of thousands: config 5 as one shard on one GPU 1 536 -> 2 287 pivots/s)
    const int g1 = (int)((t.rows + kGatherThreads - 1) / kGatherThreads);
    const int g2 = (int)(((t.ld >> 1) + kScaleThreads - 1) / kScaleThreads);
    const bool split = shard_la_split(t);
    if (!split) {
        hipLaunchKernelGGL(k_shard_la_prepare, dim3(1), dim3(kSelThreads), 0, s, t, j, col, ec_dev,
                           0.0 + (f / 2.0) * kClEpsilon, sgn_of(is_max));
        return kSelWaves;                            // pricing partials left for the next step
    }
    hipLaunchKernelGGL(k_shard_la_ratio, dim3(g1), dim3(kGatherThreads), 0, s, t, j, col, ec_dev,
                       0.0 + (f / 2.0) * kClEpsilon, x);
    switch (j) {
#define MI_SLA(J) case J: launch_shard_la_scale_t<J>(t, g2, g1, ec_dev, is_max, s); break;
        MI_SLA(0) MI_SLA(1) MI_SLA(2) MI_SLA(3) MI_SLA(4) MI_SLA(5) MI_SLA(6) MI_SLA(7)
        MI_SLA(8) MI_SLA(9) MI_SLA(10) MI_SLA(11) MI_SLA(12) MI_SLA(13) MI_SLA(14) MI_SLA(15)
        MI_SLA(16) MI_SLA(17) MI_SLA(18) MI_SLA(19) MI_SLA(20) MI_SLA(21) MI_SLA(22) MI_SLA(23)     // wide blocks
        MI_SLA(24) MI_SLA(25) MI_SLA(26) MI_SLA(27)
#undef MI_SLA
    }
    return g2 * (kScaleThreads / 64);
}
// the look-ahead step of a large shard in exchange mode 2 as TWO launches (see k_shard_p2p_step);
// returns the pricing partials it leaves, 0 when this shard / state needs the separate launches
int launch_shard_p2p_step(const TabView &t, int j, int n_part, int n_shards, int64_t col_offset, double f,
                          int is_max, int64_t *ec_dev, hipStream_t s, const P2pArgs &x)
{
    if (!x.peers || n_part <= 0 || !shard_la_split(t)) return 0;
    int blocks = (int)((t.rows + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    if (blocks > t.part_cap / 2) return 0;
    const int g2 = (int)(((t.ld >> 1) + kScaleThreads - 1) / kScaleThreads);
    hipLaunchKernelGGL(k_shard_p2p_step, dim3(blocks), dim3(256), 0, s, t, j, n_part, n_shards, col_offset,
                       (f / 8.0) * kClEpsilon, 0.0 + (f / 2.0) * kClEpsilon, ec_dev, x);
    switch (j) {
#define MI_SLA(J) case J: launch_shard_la_scale_t<J>(t, g2, blocks, ec_dev, is_max, s); break;
        MI_SLA(0) MI_SLA(1) MI_SLA(2) MI_SLA(3) MI_SLA(4) MI_SLA(5) MI_SLA(6) MI_SLA(7)
        MI_SLA(8) MI_SLA(9) MI_SLA(10) MI_SLA(11) MI_SLA(12) MI_SLA(13) MI_SLA(14) MI_SLA(15)
        MI_SLA(16) MI_SLA(17) MI_SLA(18) MI_SLA(19) MI_SLA(20) MI_SLA(21) MI_SLA(22) MI_SLA(23)     // wide blocks
        MI_SLA(24) MI_SLA(25) MI_SLA(26) MI_SLA(27)
#undef MI_SLA
    }
    return g2 * (kScaleThreads / 64);
}
// the objective row of `mt` re-eliminated over its basic rows with the scales in mt.col[0 .. m) (one thread per
// column; the caller put the scales there: src/simplex.lisp:444-451 with the scales already known)
void launch_handover_objective_columns(const TabView &mt, hipStream_t s)
{
    hipLaunchKernelGGL(k_handover_objective_columns, dim3((unsigned)((mt.cols + 255) / 256)), dim3(256), 0, s, mt);
}
void launch_handover(const TabView &art, const TabView &mt, bool unit_basis, hipStream_t s)
{
    const int64_t m = mt.rows - 1;
    if (m > 0) {
        int bx = (int)((mt.cols + 255) / 256);
        if (bx > 64) bx = 64;
        hipLaunchKernelGGL(k_handover_copy, dim3(bx, (unsigned)(m < 32768 ? m : 32768)), dim3(256), 0, s, art, mt);
    }
    if (unit_basis && m > 0) {
        hipLaunchKernelGGL(k_handover_scales, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, art, mt);
        hipLaunchKernelGGL(k_handover_objective_columns, dim3((unsigned)((mt.cols + 255) / 256)), dim3(256),
                           0, s, mt);
    } else {
        hipLaunchKernelGGL(k_handover_objective, dim3(1), dim3(kSelThreads), 0, s, art, mt);
    }
}
// one launch solves the whole batch; returns false if an LP does not fit the LDS budget
static int g_batch_block = 0;                                  // 0 = default (16), 1 = per-pivot k_batch_solve
void set_batch_block(int k) { g_batch_block = k; }

template <int KB>
static bool launch_batch_block_t(const TabView &t, int is_max, double f, hipStream_t s, int split = 0)
{
    const int64_t rp = (t.rows + 1) & ~(int64_t)1, ldv = t.ld >> 1;
    const size_t bytes = (size_t)((int64_t)KB * (t.ld + rp) + t.ld + rp + t.ld + rp) * 8 + (size_t)(rp + ldv) * 4;
    if (bytes > 150 * 1024) return false;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_batch_block<KB, false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_batch_block<KB, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        (void)hipGetLastError();
        attr_set = true;
    }
    if (split)
        hipLaunchKernelGGL((k_batch_block<KB, true>), dim3(1, 1, (unsigned)t.n_lps), dim3(kBbThreads), bytes, s, t,
                           sgn_of(is_max), (f / 8.0) * kClEpsilon, 0.0 + (f / 2.0) * kClEpsilon);
    else
        hipLaunchKernelGGL((k_batch_block<KB, false>), dim3(1, 1, (unsigned)t.n_lps), dim3(kBbThreads), bytes, s, t,
                           sgn_of(is_max), (f / 8.0) * kClEpsilon, 0.0 + (f / 2.0) * kClEpsilon);
    return true;
}

bool launch_batch_solve(const TabView &t, int is_max, double f, hipStream_t s)
{
    // blocked (compact representation), largest block that fits the LDS.  Measured at 257 x 513,
    // steady state (tools/batch_blocks.py): 128 LPs 2.0 M pivots/s per-pivot, 3.36 M at 8, 3.44 M
    // at 16; 1024 LPs 2.5 M per-pivot, 7.3 M at 8, 7.9 M at 16
    int kb = g_batch_block;
    if (kb == 0) kb = 16;
    if (t.p2l && kb > 1 && t.rows >= 2 && (t.ld >> 1) >= 1) {
        if (kb >= 16 && launch_batch_block_t<16>(t, is_max, f, s)) return true;
        if (kb >= 8 && launch_batch_block_t<8>(t, is_max, f, s)) return true;
        if (launch_batch_block_t<4>(t, is_max, f, s)) return true;
    }
    const size_t lds = (size_t)(t.ld + t.rows) * sizeof(double);
    if (lds > 96 * 1024 || t.ld / 2 < 1) return false;
    hipLaunchKernelGGL(k_batch_solve, dim3(1, 1, (unsigned)t.n_lps), dim3(kLpThreads), lds, s, t,
                       sgn_of(is_max), (f / 8.0) * kClEpsilon, 0.0 + (f / 2.0) * kClEpsilon);
    return true;
}
static int g_sweep_tr = 0, g_sweep_nt = -1;                     // 0 / -1: by size
static int g_sweepw_ring = 1;                                   // wide sweeps: rows through a per-wave LDS ring (k_sweepw_ring), 0: k_sweepw
void set_sweepw_ring(int on) { g_sweepw_ring = (on >= 0 && on <= 3) ? on : 1; }   // 1: non-temporal accesses by size (loads from 240 MiB, stores from 320 MiB); A/B: 2 neither, 3 stores only
static int g_sweep_impl = 0;                                    // 0: k_sweep16 for full blocks, 1: k_sweep always
bool launch_batch_block_split(const TabView &t, int is_max, double f, hipStream_t s)
{
    if (!t.p2l || !t.blk || !t.bk_col || !t.bk_prow || t.n_lps < 2 || t.rows < 2) return false;
    if (!launch_batch_block_t<16>(t, is_max, f, s, /*split=*/1)) return false;
    // the sweep of every LP's pending pivots: k_sweep copes with any number of pending pivots per
    // LP (an LP that has finished has none), grid.z = LP
    constexpr int block = 256;
    const int64_t ldv = t.ld >> 1;
    int strips = (int)((ldv + block - 1) / block);
    int64_t sp = (ldv + strips - 1) / strips;
    sp = (sp + 7) / 8 * 8;
    if (sp > block) sp = block;
    strips = (int)((ldv + sp - 1) / sp);
    // measured (tools/batch_sweep_ab.py, 257 x 513 stored per LP): k_sweep with 16-row tiles 7.2 /
    // 11.4 M pivots/s at 128 / 1024 LPs (32 rows 6.8 / 11.3); k_sweep16, whose partial-block form is
    // a slow one and every LP ends on a partial block, 6.7 / 10.2
    int64_t tr = g_sweep_tr ? g_sweep_tr : 16;
    while (tr > 4 && ((t.rows + tr - 1) / tr) * strips * t.n_lps < 2048) tr /= 2;
    const dim3 grid((unsigned)strips, (unsigned)((t.rows + tr - 1) / tr), (unsigned)t.n_lps);
    hipLaunchKernelGGL((k_sweep<256, 16, false>), grid, dim3(256), 0, s, t, (int)tr, (int)sp, sgn_of(is_max), 0, 0u, 0);
    return true;
}
void launch_verify_basis(const TabView &t, int *flag, hipStream_t s)
{
    const unsigned g = (unsigned)(t.rows < 16384 ? t.rows : 16384);
    hipLaunchKernelGGL(k_verify_basis, dim3(g, 1, (unsigned)t.n_lps), dim3(256), 0, s, t, flag);
}
void launch_compact(const TabView &d, const TabView &c, hipStream_t s)
{
    int bx = (int)((c.ld + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(k_compact, dim3(bx, (unsigned)(d.rows < 32768 ? d.rows : 32768), (unsigned)d.n_lps),
                       dim3(256), 0, s, d, c);
}
void launch_expand(const TabView &d, const TabView &c, int64_t *brow, hipStream_t s)
{
    const int64_t n = (d.cols > d.rows ? d.cols : d.rows);
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_basis_rows, dim3(g, 1, (unsigned)d.n_lps), dim3(256), 0, s, d, brow, 0);
    hipLaunchKernelGGL(k_basis_rows, dim3(g, 1, (unsigned)d.n_lps), dim3(256), 0, s, d, brow, 1);
    int bx = (int)((d.ld + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(k_expand, dim3(bx, (unsigned)(d.rows < 32768 ? d.rows : 32768), (unsigned)d.n_lps),
                       dim3(256), 0, s, d, c, brow);
}
void launch_ctl_reset(const TabView &t, int64_t max_pivots, int reset_trace, hipStream_t s)
{
    hipLaunchKernelGGL(k_ctl_reset, dim3((unsigned)t.n_lps), dim3(1), 0, s, t.ctl, max_pivots, reset_trace);
}
void launch_ctl_publish(const TabView &t, int64_t n, void *host_dst, unsigned long long *host_seq, unsigned long long seq, hipStream_t s)
{
    static_assert(sizeof(Ctl) % 8 == 0, "copied as 8-byte words");
    hipLaunchKernelGGL(k_ctl_publish, dim3(1), dim3(256), 0, s, t.ctl, reinterpret_cast<unsigned long long *>(host_dst),
                       n * (int64_t)(sizeof(Ctl) / 8), host_seq, seq);
}
void launch_ctl_resume(const TabView &t, hipStream_t s, int32_t from)
{
    hipLaunchKernelGGL(k_ctl_resume, dim3((unsigned)t.n_lps), dim3(1), 0, s, t.ctl, from);
}
void launch_ctl_finish(const TabView &t, hipStream_t s)
{
    hipLaunchKernelGGL(k_ctl_finish, dim3((unsigned)t.n_lps), dim3(1), 0, s, t.ctl);
}
void launch_synth_fill(const TabView &t, int64_t n, int64_t m, uint64_t seed,
                       const uint64_t *dev_seeds, int64_t cb, int64_t ce, hipStream_t s)
{
    int bx = (int)((t.ld + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(k_synth_fill, dim3(bx, (unsigned)(t.rows < 32768 ? t.rows : 32768), (unsigned)t.n_lps),
                       dim3(256), 0, s, t, n, m, seed, dev_seeds, cb, ce);
}

// ---- update-kernel variants (one is the default; the others exist for the tuning sweep)
struct UpdateVariant {
    const char *name;
    int block;            // threads per workgroup = max column pairs per strip
    int unroll;           // rows in flight per thread; rows per workgroup is a multiple of it
    int min_tr;           // never fewer rows per workgroup than this
    int rounds;           // aim for rounds * (resident workgroup slots) workgroups
    void (*launch)(const TabView &, dim3, int, int, double, int, int, hipStream_t);
};

template <int BLOCK, int U, bool NT>
static void launch_update_t(const TabView &t, dim3 grid, int tr, int strip_pairs, double sgn,
                            int price, int reverse, hipStream_t s)
{
    hipLaunchKernelGGL((k_update<BLOCK, U, NT>), grid, dim3(BLOCK), 0, s, t, tr, strip_pairs, sgn,
                       price, reverse);
}

#define MI_VARIANT(B, U, NT, MINTR, ROUNDS) \
    { "b" #B "_u" #U "_nt" #NT "_mintr" #MINTR "_x" #ROUNDS, (B), (U), (MINTR), (ROUNDS), &launch_update_t<B, U, NT> }

static const UpdateVariant kVariants[] = {
    MI_VARIANT(256, 4, true, 4, 0),     // 0: default -- 4-row tiles whatever the size; the
                                        //    launcher swaps in variant 1 (plain loads/stores)
                                        //    when the stored tableau fits the Infinity Cache
    MI_VARIANT(256, 4, false, 4, 0),
    MI_VARIANT(256, 4, true, 4, 16),
    MI_VARIANT(256, 4, true, 4, 8),
    MI_VARIANT(256, 2, true, 2, 0),
    MI_VARIANT(256, 2, false, 2, 0),
    MI_VARIANT(256, 8, true, 8, 0),
    MI_VARIANT(256, 8, false, 8, 0),
    MI_VARIANT(256, 8, true, 8, 4),
    MI_VARIANT(128, 4, false, 4, 0),
    MI_VARIANT(128, 8, true, 8, 0),
    MI_VARIANT(512, 4, true, 4, 0),
    MI_VARIANT(512, 4, false, 4, 0),
    MI_VARIANT(512, 2, false, 2, 0),
    MI_VARIANT(64, 4, false, 4, 0),
    MI_VARIANT(1024, 4, false, 4, 0),
    MI_VARIANT(256, 4, false, 8, 0),
    MI_VARIANT(256, 1, false, 1, 0),
};
static int g_variant = 0;
constexpr int kCUs = 256, kThreadsPerCU = 2048;

int         update_variant_count() { return (int)(sizeof(kVariants) / sizeof(kVariants[0])); }
const char *update_variant_name(int v) { return kVariants[v].name; }
void        set_update_variant(int v) { if (v >= 0 && v < update_variant_count()) g_variant = v; }
int         get_update_variant() { return g_variant; }
const char *update_kernel_symbol() { return "k_update"; }

// Non-temporal accesses pay off when the stored tableau is streamed from HBM every pivot
// (config 3 dense, 403 MB: 125 vs 145 us); when it (mostly) fits the 256 MiB Infinity Cache
// plain accesses are faster (config 3 compact, 269 MB: 82 vs 90 us).
constexpr double kNtThresholdBytes = 320.0 * 1024 * 1024;
// the ring sweep's LOADS alone go non-temporal from here on (a stored tableau that no longer fits the 256 MiB
// Infinity Cache: what a pass reads is not worth keeping, what it writes is what the look-ahead and the next pass
// read first) -- measured, pivots/s with / without: 144 MB 97.6 k / 100.2 k, 196 MB 92.6 k / 94.9 k, 268.5 MB 81.9 k / 80.8 k
constexpr double kNtLoadThresholdBytes = 240.0 * 1024 * 1024;

static int effective_variant(const TabView &t)
{
    if (g_variant != 0) return g_variant;
    const double bytes = (double)t.rows * (double)t.ld * 8.0 * (double)t.n_lps;
    return bytes > kNtThresholdBytes ? 0 : 1;
}

UpdateShape update_shape(const TabView &t)
{
    const UpdateVariant &v = kVariants[effective_variant(t)];
    const int64_t ldv = t.ld >> 1;
    UpdateShape g;
    g.strips = (int)((ldv + v.block - 1) / v.block);
    // equal-width strips, a multiple of 8 pairs (128 bytes) wide
    int64_t sp = (ldv + g.strips - 1) / g.strips;
    sp = (sp + 7) / 8 * 8;
    if (sp > v.block) sp = v.block;
    g.strip_pairs = (int)sp;
    g.strips = (int)((ldv + sp - 1) / sp);
    // Rows per workgroup.  Measured on config 3 (DESIGN.md 4.1): SMALL tiles win -- with 4-row
    // tiles dispatched x-fastest the resident workgroups cover one contiguous window of the
    // tableau that sweeps through memory once.  rounds == 0 selects that fixed small tile;
    // rounds > 0 is the older "rounds x resident slots" sizing kept for the tuning sweep.
    int64_t tr = v.min_tr;
    if (v.rounds > 0) {
        const int64_t slots = (int64_t)kCUs * (kThreadsPerCU / v.block) * v.rounds;
        int64_t by = slots / ((int64_t)g.strips * t.n_lps);
        if (by < 1) by = 1;
        tr = (t.rows + by - 1) / by;
        if (tr < v.min_tr) tr = v.min_tr;
    }
    tr = (tr + v.unroll - 1) / v.unroll * v.unroll;
    while ((t.rows + tr - 1) / tr > 65535) tr *= 2;            // grid.y limit
    g.tr = (int)tr;
    g.row_chunks = (int)((t.rows + tr - 1) / tr);
    g.waves_per_block = v.block / 64;
    g.n_partials = g.strips * g.waves_per_block;
    return g;
}

// measured: no gain (config 3 compact 82.9 vs 81.9 us, dense 131.7 vs 131.2 us) -- the Infinity
// Cache does not behave like an LRU over a slightly-too-large streamed working set.  Off.
static int g_alternate_sweep = 0;
void set_alternate_sweep(int on) { g_alternate_sweep = on ? 1 : 0; }

int launch_update(const TabView &t, double sgn, int price, hipStream_t s, int64_t launch_index)
{
    const UpdateVariant &v = kVariants[effective_variant(t)];
    const UpdateShape g = update_shape(t);
    if (price && g.n_partials > t.part_cap / 2) price = 0;
    v.launch(t, dim3((unsigned)g.strips, (unsigned)g.row_chunks, (unsigned)t.n_lps), g.tr,
             g.strip_pairs, sgn, price, (g_alternate_sweep && (launch_index & 1)) ? 1 : 0, s);
    return price ? g.n_partials : 0;
}

// ---- blocked pivoting launchers
bool block_supported(const TabView &t)
{
    return t.blk && t.bk_col && t.bk_prow && t.p2l && t.n_lps == 1 && select_split_supported(t) &&
           (int64_t)(((t.ld >> 1) + kScaleThreads - 1) / kScaleThreads) * (kScaleThreads / 64) <= t.part_cap / 2;
}

template <int J>
static int launch_lookahead_t(const TabView &t, int is_max, double f, int n_part, hipStream_t s)
{
    const int g1 = (int)((t.rows + kGatherThreads - 1) / kGatherThreads);
    const int g2 = (int)(((t.ld >> 1) + kScaleThreads - 1) / kScaleThreads);
    hipLaunchKernelGGL(k_la_gather<J>, dim3(g1), dim3(kGatherThreads), 0, s, t, sgn_of(is_max),
                       (f / 8.0) * kClEpsilon, 0.0 + (f / 2.0) * kClEpsilon, n_part);
    hipLaunchKernelGGL(k_la_scale<J>, dim3(g2), dim3(kScaleThreads), 0, s, t, g1, sgn_of(is_max));
    return g2 * (kScaleThreads / 64);
}

int launch_lookahead(const TabView &t, int j, int is_max, double f, int n_part, hipStream_t s)
{
    switch (j) {
#define MI_LA(J) case J: return launch_lookahead_t<J>(t, is_max, f, n_part, s);
        MI_LA(0) MI_LA(1) MI_LA(2) MI_LA(3) MI_LA(4) MI_LA(5) MI_LA(6) MI_LA(7)
        MI_LA(8) MI_LA(9) MI_LA(10) MI_LA(11) MI_LA(12) MI_LA(13) MI_LA(14) MI_LA(15)
        MI_LA(16) MI_LA(17) MI_LA(18) MI_LA(19) MI_LA(20) MI_LA(21) MI_LA(22) MI_LA(23)     // wide blocks
        MI_LA(24) MI_LA(25) MI_LA(26) MI_LA(27)
#undef MI_LA
    }
    return 0;
}

bool la_block_supported(const TabView &t)
{
    if (!block_supported(t) || !t.la_px || !t.la_rx) return false;
    const int64_t need = t.rows > (t.ld >> 1) ? t.rows : (t.ld >> 1);
    return (need + kLaThreads - 1) / kLaThreads <= kMaxLaWorkgroups;
}

static int      g_la_one_xcd = 1, g_la_fault = 0;
static unsigned g_la_max_spins = 1u << 21;
void set_la_one_xcd(int on) { g_la_one_xcd = on ? 1 : 0; }
void set_la_max_spins(unsigned n) { g_la_max_spins = n ? n : (1u << 21); }
#ifdef MI355X_TEST_HOOKS
void set_la_fault(int step_plus_1) { g_la_fault = step_plus_1; }
#endif

int la_block_workgroups(const TabView &t)
{
    const int64_t need = t.rows > (t.ld >> 1) ? t.rows : (t.ld >> 1);
    return (int)((need + kLaThreads - 1) / kLaThreads);
}

// The workgroups k_la_block is LAUNCHED with: a thread per constraint row and per pair that holds a non-RHS
// column (the objective row and the RHS column have no owner there).  What follows the launch follows this
// count -- the sweeps' and the rollback's la_nw, BlockCtl::done, one-XCD mode, records per wave or per workgroup;
// which tableaux take the persistent look-ahead and every block-size decision stay on la_block_workgroups().
int la_launch_workgroups(const TabView &t)
{
    const int64_t m = t.rows - 1, npair = t.cols >> 1;         // (ceil(vc / 2), vc = cols - 1)
    const int64_t need = m > npair ? m : npair;
    return need > 0 ? (int)((need + kLaThreads - 1) / kLaThreads) : 1;
}

void launch_la_rollback(const TabView &t, int la_nw, hipStream_t s)
{
    hipLaunchKernelGGL(k_la_rollback, dim3(1), dim3(1), 0, s, t, la_nw);
}

// ---- a shard's look-ahead of a whole block as ONE persistent launch (kernels_shard_block.inc)
static int g_shard_la_fault = 0;
#ifdef MI355X_TEST_HOOKS
void set_shard_la_fault(int step_plus_1) { g_shard_la_fault = step_plus_1; }
#endif
int shard_la_block_workgroups(const TabView &t)
{
    if (!t.blk || !t.bk_col || !t.bk_prow || !t.bk_rmask || !t.bk_smask || !t.bk_smask2 || !t.la_px || !t.la_rx ||
        t.n_lps != 1 || !t.M)
        return 0;
    const int64_t need = t.rows > (t.ld >> 1) ? t.rows : (t.ld >> 1);
    const int64_t nw = (need + kLaThreads - 1) / kLaThreads;
    return nw < kMaxShardLaWorkgroups ? (int)nw : 0;         // (the last record line carries the ratio exchange's decision)
}
void launch_shard_la_block(const ShardLaunch *dev_shards, int n_local, int nw_max, const P2pLayout &lay, int ksteps,
                           int is_max, double f, unsigned epoch_base, unsigned xepoch_base, unsigned p2p_spins, int hop,
                           hipStream_t s)
{
    const dim3 grid((unsigned)nw_max, (unsigned)n_local);
    const double price_tol = (f / 8.0) * kClEpsilon, ratio_thr = 0.0 + (f / 2.0) * kClEpsilon;
    if (ksteps <= kMaxBlock)
        hipLaunchKernelGGL(k_shard_la_block<kMaxBlock>, grid, dim3(kLaThreads), 0, s, dev_shards, lay, ksteps, sgn_of(is_max),
                           price_tol, ratio_thr, epoch_base, xepoch_base, g_la_max_spins, p2p_spins, hop, g_shard_la_fault);
    else
        hipLaunchKernelGGL(k_shard_la_block<kLaBlockMax>, grid, dim3(kLaThreads), 0, s, dev_shards, lay, ksteps, sgn_of(is_max),
                           price_tol, ratio_thr, epoch_base, xepoch_base, g_la_max_spins, p2p_spins, hop, g_shard_la_fault);
}
void launch_shard_la_rollback(const TabView &t, int la_nw, hipStream_t s)
{
    hipLaunchKernelGGL(k_shard_la_rollback, dim3(1), dim3(1), 0, s, t, la_nw);
}

// form: the block size that picks the kernel (<= 16: the 16-step look-ahead, above: the 24-step one)
void launch_la_block_form(const TabView &t, int form, int ksteps, int is_max, double f, unsigned epoch_base, hipStream_t s)
{
    const int nw = la_launch_workgroups(t);
    // one-XCD mode: 8 x nw blocks, every eighth takes part (the kernel verifies where they run); more than
    // kLaWaveRecordsMaxNw workgroups: records per workgroup, spread over the chip (an XCD has 32 CUs)
    const bool wgr = nw > kLaWaveRecordsMaxNw;
    const int one_xcd = g_la_one_xcd && nw > 1 && !wgr;
    const dim3 grid(one_xcd ? 8 * nw : nw);
    const double pt = (f / 8.0) * kClEpsilon, rt = 0.0 + (f / 2.0) * kClEpsilon;
    // (the pending pivots' col / prow entries live in LDS, 6 KB each: the 24-step form only where asked for)
    if (form > kMaxBlock) {
        if (wgr) hipLaunchKernelGGL((k_la_block<kLaBlockMax, true>), grid, dim3(kLaThreads), 0, s, t, ksteps, sgn_of(is_max), pt, rt,
                                    epoch_base, g_la_max_spins, one_xcd, g_la_fault);
        else     hipLaunchKernelGGL((k_la_block<kLaBlockMax, false>), grid, dim3(kLaThreads), 0, s, t, ksteps, sgn_of(is_max), pt, rt,
                                    epoch_base, g_la_max_spins, one_xcd, g_la_fault);
    } else {
        if (wgr) hipLaunchKernelGGL((k_la_block<kMaxBlock, true>), grid, dim3(kLaThreads), 0, s, t, ksteps, sgn_of(is_max), pt, rt,
                                    epoch_base, g_la_max_spins, one_xcd, g_la_fault);
        else     hipLaunchKernelGGL((k_la_block<kMaxBlock, false>), grid, dim3(kLaThreads), 0, s, t, ksteps, sgn_of(is_max), pt, rt,
                                    epoch_base, g_la_max_spins, one_xcd, g_la_fault);
    }
}
void launch_la_block(const TabView &t, int ksteps, int is_max, double f, unsigned epoch_base, hipStream_t s)
{
    launch_la_block_form(t, ksteps, ksteps, is_max, f, epoch_base, s);
}


// ---- the resident solve
static int g_res_fault = 0, g_res_poll = 0;
#ifdef MI355X_TEST_HOOKS
void set_resident_fault(int on) { g_res_fault = on; }
#endif
static int g_res_lds = 0;
void set_resident_lds(int mode) { g_res_lds = mode; }       // tuning: 1 = 24 of a strip's 64 columns in LDS (one row per thread), 0 = never (default)
void set_resident_poll(int mode) { g_res_poll = mode; }     // tuning: 0 / 2 every wave polls (default), 1 wave 0 polls

bool resident_plan(const TabView &c, ResidentPlan *p)
{
    if (!c.p2l || !c.l2p || c.rows < 2 || c.cols < 2) return false;
    const int64_t m = c.rows - 1, nnb = c.cols - 1;
    if (m > 1024) return false;
    const int TR = m <= 256 ? 1 : (m <= 512 ? 2 : 4);
    const int CW = 64 / TR;
    const int64_t G = (nnb + CW - 1) / CW;
    if (G > 32) return false;
    if (p) {
        p->TR = TR; p->CW = CW; p->G = (int)G;
        p->slot_granules = 8 + 2 * ((m + 1 + 7) / 8 * 8);
        p->lp_granules = G * 2 * p->slot_granules + 8;            // + the lost flag (padded)
    }
    return true;
}

size_t resident_xbuf_bytes(const TabView &c)
{
    ResidentPlan p;
    if (!resident_plan(c, &p)) return 0;
    return (size_t)c.n_lps * (size_t)p.lp_granules * sizeof(unsigned long long);
}

bool launch_resident(const TabView &c, unsigned long long *xbuf, int is_max, double f, int cap,
                     unsigned epoch_base, hipStream_t s)
{
    ResidentPlan p;
    if (!xbuf || cap < 1 || !resident_plan(c, &p)) return false;
    ResidentArgs a;
    a.sgn = sgn_of(is_max);
    a.price_tol = (f / 8.0) * kClEpsilon;
    a.ratio_thr = 0.0 + (f / 2.0) * kClEpsilon;
    a.xbuf = xbuf;
    a.xs_lp = p.lp_granules;
    a.xs_slot = p.slot_granules;
    a.G = p.G;
    a.cap = cap;
    a.epoch_base = epoch_base;
    a.spins_first = g_la_max_spins;
    a.spins = 1u << 27;
    a.fault = g_res_fault;
    const unsigned groups = (unsigned)((c.n_lps + 7) / 8);
    const dim3 grid(groups * 8u * (unsigned)p.G);
    // who polls the records: every wave for itself (no LDS hop, no workgroup barrier behind the
    // exchange) -- measured round 3, final loop: config 2 (32 workgroups) 257 k pivots/s against 247 k
    // with wave 0 polling for the workgroup, 128-LP batch 10.3 against 9.8 M
    const bool every = g_res_poll != 1;
#define MI_RES(TR_, CW_, CL_)                                                                                       \
    do {                                                                                                       \
        if (every) hipLaunchKernelGGL((k_resident<TR_, CW_, true, CL_>),  grid, dim3(kResThreads), 0, s, c, a);    \
        else       hipLaunchKernelGGL((k_resident<TR_, CW_, false, CL_>), grid, dim3(kResThreads), 0, s, c, a);    \
    } while (0)
    // part of the strip in LDS (three workgroups per CU, 96 LPs of the config-4 shape in flight
    // instead of 64): built and measured in round 4 -- NOT faster.  1 024 LPs: 9.6 ms against 9.7 ms
    // on the device, 128 LPs 1.71 against 1.55 ms: a pivot takes 7.0 us with three waves per SIMD
    // against 4.7 us with two, i.e. the SIMDs are issue-bound at two waves already (about 2.35 us of
    // instruction issue per pivot and wave) and a third wave only queues behind them.  Kept behind
    // the tuning knob (off by default) so that the measurement can be repeated (tools/resident_lds_ab.py).
    const bool lds = p.TR == 1 && g_res_lds == 1;
    if (p.TR == 1 && lds) MI_RES(1, 64, 24);
    else if (p.TR == 1)   MI_RES(1, 64, 0);
    else if (p.TR == 2)   MI_RES(2, 32, 0);
    else                  MI_RES(4, 16, 0);
#undef MI_RES
    return true;
}

static int g_sweep_u = 4;                                       // rows per step of k_sweep16: 4, or 8 (measured
                                                                // slower: 199 VGPRs, 2 waves per SIMD, 125 vs 103 us)
void set_sweep_shape(int tr, int nt) { g_sweep_tr = tr >= 4 ? tr / 4 * 4 : 0; g_sweep_nt = nt; }
void set_sweep_impl(int impl) { g_sweep_impl = (impl == 1 || impl == 3) ? impl : 0; if (impl == 4 || impl == 8) g_sweep_u = impl; }

template <int KMAX>
static void launch_sweep_t(const TabView &t, dim3 grid, int tr, int sp, double sgn, bool nt, unsigned stamp,
                           int la_nw, hipStream_t s)
{
    if (nt) hipLaunchKernelGGL((k_sweep<256, KMAX, true>),  grid, dim3(256), 0, s, t, tr, sp, sgn, 1, stamp, la_nw);
    else    hipLaunchKernelGGL((k_sweep<256, KMAX, false>), grid, dim3(256), 0, s, t, tr, sp, sgn, 1, stamp, la_nw);
}

// which kernel launch_sweep picks for a block of kmax pending pivots: 2 the wide pair (k_sweepw +
// k_sweepw_rest), 1 k_sweep16, 0 k_sweep<..> (short blocks)
static int g_sweep_skew = -1;                                    // k_sweepw_ring, one round: -1 by the tile height, 0 off, > 0 rows
void set_sweep_skew(int rows) { g_sweep_skew = rows < 0 ? -1 : rows / 4 * 4; }
static int g_sweep_xmap = 0;
void set_sweep_xmap(int on) { g_sweep_xmap = on ? 1 : 0; }
int sweep_kind(int kmax)
{
    if (kmax > kSweepK || (kmax == kSweepK && g_sweep_impl == 3)) return 2;
    return (kmax == kSweepK && g_sweep_impl == 0) ? 1 : 0;
}

// applies up to kmax pending pivots; returns the number of pricing partials it leaves
int launch_sweep(const TabView &t, int kmax, double sgn, hipStream_t s, unsigned stamp, int la_nw)
{
    constexpr int block = 256;
    const int64_t ldv = t.ld >> 1;
    int strips = (int)((ldv + block - 1) / block);
    int64_t sp = (ldv + strips - 1) / strips;
    sp = (sp + 7) / 8 * 8;
    if (sp > block) sp = block;
    strips = (int)((ldv + sp - 1) / sp);
    // rows per workgroup: 32 (config 3, measured: 8 rows 116 us, 16 rows 105, 32 rows 103, 64 rows
    // 114), fewer when the tableau would otherwise not fill the chip with workgroups
    int64_t tr = g_sweep_tr;
    if (tr == 0) {
        // (a short block leaves most of the registers free: more, smaller tiles in flight --
        // config 3, 4 pending pivots: 8 rows 87 us, 16 rows 89, 32 rows 97, 64 rows 95)
        tr = kmax <= 4 ? 8 : kmax <= 8 ? 16 : 32;
        while (tr > 4 && ((t.rows + tr - 1) / tr) * strips < 2048) tr /= 2;
    }
    while ((t.rows + tr - 1) / tr > 65535) tr *= 2;            // grid.y limit
    const dim3 grid((unsigned)strips, (unsigned)((t.rows + tr - 1) / tr));
    const double bytes = (double)t.rows * (double)t.ld * 8.0;
    const bool nt = g_sweep_nt < 0 ? bytes > kNtThresholdBytes : g_sweep_nt != 0;
    if (kmax > kSweepK || (kmax == kSweepK && g_sweep_impl == 3)) {
        // wide blocks (k_sweepw): the kernel compiled for the smallest K >= kmax; fewer pending
        // pivots than K (a block cut short) take its row-at-a-time path
        if (g_sweep_tr == 0 && kmax > kSweepK) {
            // measured per pass (round 5, ring kernel), 32 / 64 / 128 rows: 2.15 GB (an 8-GPU-sized shard) 731 /
            // 745 / 775 us, 2.3 GB 888 / 890 / 905, 6.4 GB 2 621 / 2 459 / 2 429, 17.2 GB (config 5) 8 297 / 7 168 /
            // 6 793 - 6 902 (192 and 256 rows: 6 848 / 6 830)
            // -- and 28 pivots per pass want the tall tile at every size (28 prow pairs per tile: 2.3 GB 55.6 us per
            // pivot with 32 rows, 49.2 with 128; 3.8 GB 82.4 / 70.8; a 2.15 GB shard shape 51.0 / 46.4)
            tr = (bytes > 4e9 || kmax > 24) ? 128 : 32;
            while ((t.rows + tr - 1) / tr > 65535) tr *= 2;
        }
        bool one_round = false;
        if (g_sweep_tr == 0 && g_sweepw_ring) {
            // ONE round: the ring kernel runs three workgroups per CU; where tiles of at most 128 rows can
            // cover the tableau with no more workgroups than that, they do -- no second, partly filled
            // round, fewer prologues.  Measured per pass, one round / 32-row tiles: 4095 x 3200 (36 rows)
            // 53 / 59 us, 6000 x 5000 (80 rows) 96 / 98.5, config 3 (92 rows: 765 workgroups instead of
            // 2 193) 107.6 / 109.4 over nine launches each; 8000 x 8000 would take 168-row tiles and loses
            // (194 / 188), hence the limit
            static const int n_cu = [] { int d = 0, n = 0; return (hipGetDevice(&d) == hipSuccess &&
                hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && n > 0) ? n : 256; }();
            const int64_t per_strip = (int64_t)3 * n_cu / strips;
            if (per_strip >= 1) {
                const int64_t tr1 = ((t.rows + per_strip - 1) / per_strip + 3) / 4 * 4;
                if (tr1 > tr && tr1 <= 128) { tr = tr1; one_round = true; }
            }
        }
        // (round 6) one round: the thirds of the tiles in dispatch order get tr + skew / tr / tr - skew rows (the
        // kernel says why).  Config 3 (tr 92), per pass: skew 0 108.2-109.4 us, 16 103.1-104.4, 24 102.0-103.4,
        // 28 101.1-103.0, 32 101.9-104.2, 36 103.3-104.4, 40 104.6-106.8, 48 108.5-109.4: five sixteenths of the
        // tile height (4095 x 3200: 54.5 -> 51.6 us, 6000 x 5000: 95.2 -> 89.0).  Taken back, four rows at a time,
        // while the first two thirds would leave the last one nothing (or more than tr rows per tile).
        // The last third (T - 2 (T / 3) tiles: one or two more than a third when T is not a multiple of three) shares
        // what the first two leave, in tiles of tr3 rows (a multiple of four; config 3: 64 = tr - skew; 8000 x 3000,
        // 47 tiles of 64: 84 / 64 / 48 -- with tr - skew = 44 the last tile was left with 77 rows and the pass took
        // 86.5 us instead of 81).
        int skew = 0, tr3 = (int)tr;
        if ((one_round || g_sweep_skew > 0) && g_sweepw_ring && g_sweep_xmap == 0 && tr <= 256) {   // (an explicit skew: whatever the grid -- tests)
            const int64_t T = (t.rows + tr - 1) / tr, T3 = T / 3, G3 = T - 2 * T3;
            skew = g_sweep_skew >= 0 ? g_sweep_skew : (int)(tr * 5 / 16 / 4 * 4);
            if (T3 < 2) skew = 0;
            for (; skew > 0; skew -= 4) {
                const int64_t left = t.rows - T3 * (tr + skew) - T3 * tr;          // rows of the last third
                if (left <= 0 || tr + skew > 256) continue;
                const int64_t h3 = ((left + G3 - 1) / G3 + 3) / 4 * 4;
                const int64_t r0_last = t.rows - left + (G3 - 1) * h3;
                if (h3 >= 4 && h3 <= tr && r0_last < t.rows) { tr3 = (int)h3; break; }   // (the last tile: 1 .. h3 rows)
            }
            if (skew <= 0) { skew = 0; tr3 = (int)tr; }
        }
        const dim3 gridw((unsigned)strips, (unsigned)((t.rows + tr - 1) / tr));
        const int kfull = kmax <= 16 ? 16 : (kmax <= 20 ? 20 : (kmax <= 24 ? 24 : 28));
        // the pivot-row groups (or, a block cut short, everything) and the pricing
        const dim3 gridr((unsigned)strips, (unsigned)kfull);
        // (round 5) the tile's rows through a per-wave LDS ring (k_sweepw_ring) unless switched off
#define MI_SWW(K) do { if (g_sweepw_ring && tr <= 256) { \
                           const int ntm = g_sweepw_ring == 2 ? 0 : (g_sweepw_ring == 3 ? 2 : (nt ? 3 : (bytes > kNtLoadThresholdBytes ? 1 : 0)));   /* bit 0: loads, bit 1: stores */ \
                           if (ntm == 3)      hipLaunchKernelGGL((k_sweepw_ring<K, true, true>),   gridw, dim3(256), kRingBytes, s, t, (int)tr, (int)sp, sgn, 1, stamp, la_nw, g_sweep_xmap, skew, tr3); \
                           else if (ntm == 1) hipLaunchKernelGGL((k_sweepw_ring<K, true, false>),  gridw, dim3(256), kRingBytes, s, t, (int)tr, (int)sp, sgn, 1, stamp, la_nw, g_sweep_xmap, skew, tr3); \
                           else if (ntm == 2) hipLaunchKernelGGL((k_sweepw_ring<K, false, true>),  gridw, dim3(256), kRingBytes, s, t, (int)tr, (int)sp, sgn, 1, stamp, la_nw, g_sweep_xmap, skew, tr3); \
                           else               hipLaunchKernelGGL((k_sweepw_ring<K, false, false>), gridw, dim3(256), kRingBytes, s, t, (int)tr, (int)sp, sgn, 1, stamp, la_nw, g_sweep_xmap, skew, tr3); \
                       } else if (nt) hipLaunchKernelGGL((k_sweepw<K, true>),  gridw, dim3(256), 0, s, t, (int)tr, (int)sp, stamp, la_nw); \
                       else           hipLaunchKernelGGL((k_sweepw<K, false>), gridw, dim3(256), 0, s, t, (int)tr, (int)sp, stamp, la_nw); } while (0)
        if (kfull == 16) MI_SWW(16); else if (kfull == 20) MI_SWW(20); else if (kfull == 24) MI_SWW(24); else MI_SWW(28);
#undef MI_SWW
        // (the ring form applies the general links itself and prices the objective row: ONE launch per pass)
        if (g_sweepw_ring && tr <= 256) return strips * (block / 64);
        if (nt) hipLaunchKernelGGL((k_sweepw_rest<true>),  gridr, dim3(256), 0, s, t, (int)sp, kfull, sgn, 1, stamp, la_nw);
        else    hipLaunchKernelGGL((k_sweepw_rest<false>), gridr, dim3(256), 0, s, t, (int)sp, kfull, sgn, 1, stamp, la_nw);
        return strips * (block / 64);
    }
    if (kmax == kSweepK && g_sweep_impl == 0) {
        // rows in flight per thread and step: 8 when the tile is a multiple of 8 rows (bk_rmask is
        // padded to a multiple of 16 rows, so the uint4 mask loads of the last tile stay inside)
        const bool u8 = g_sweep_u == 8 && tr % 8 == 0;
        if (u8) {
            if (nt) hipLaunchKernelGGL((k_sweep16<true, 8>),  grid, dim3(256), 0, s, t, (int)tr, (int)sp, sgn, 1, stamp, la_nw);
            else    hipLaunchKernelGGL((k_sweep16<false, 8>), grid, dim3(256), 0, s, t, (int)tr, (int)sp, sgn, 1, stamp, la_nw);
        } else {
            if (nt) hipLaunchKernelGGL((k_sweep16<true, 4>),  grid, dim3(256), 0, s, t, (int)tr, (int)sp, sgn, 1, stamp, la_nw);
            else    hipLaunchKernelGGL((k_sweep16<false, 4>), grid, dim3(256), 0, s, t, (int)tr, (int)sp, sgn, 1, stamp, la_nw);
        }
        return strips * (block / 64);
    }
    if (kmax <= 2)      launch_sweep_t<2>(t, grid, (int)tr, (int)sp, sgn, nt, stamp, la_nw, s);
    else if (kmax <= 4) launch_sweep_t<4>(t, grid, (int)tr, (int)sp, sgn, nt, stamp, la_nw, s);
    else if (kmax <= 8) launch_sweep_t<8>(t, grid, (int)tr, (int)sp, sgn, nt, stamp, la_nw, s);
    else                launch_sweep_t<16>(t, grid, (int)tr, (int)sp, sgn, nt, stamp, la_nw, s);
    return strips * (block / 64);
}

// wide blocks: 24 or 28 pivots per pass (what k_sweepw is compiled for; kWideMax is the largest)
constexpr int kWideMax = 28;
bool wide_block_size_ok(int k) { return k == 24 || k == 28; }
// A wide block pays where the pass over the stored tableau costs more than the extra links of the
// two-launch look-ahead's chains.  Measured per pivot, 16 / 24 per pass (round 5, one-launch ring pass):
// 134 MB stored 15.05 / 15.57 us, 200 MB 16.48 / 16.61, 226 MB 17.04 / 17.00, 273 MB 19.91 / 18.68,
// 396 MB 22.26 / 20.30, 649 MB 27.35 / 23.35 (round 4, two-launch pass: the switch was at 768 MiB)
int wide_block_default(const TabView &t)
{
    const double bytes = (double)t.rows * (double)t.ld * 8.0;
    // 24 or 28 (28 with 128-row tiles, launch_sweep): measured per pivot (round 5), 24 / 28: 0.86 GB 27.1 /
    // 28.9 us, 1.22 GB 33.2 / 33.9, 1.68 GB 40.5 / 39.9, 2.3 GB 51.9 / 49.2, 3.8 GB 78.4 / 70.8, 6.4 GB 118.5 /
    // 107.1, 17.2 GB (config 5) 287 / 264 (round 4: 28 from 8 GB on).  Column shards decide for themselves
    // (capi_colpart.inc: their step was measured with 24 up to 8 GB)
    return (t.bk_smask2 && bytes >= 240.0 * 1024 * 1024) ? (bytes >= 2e9 ? kWideMax : 24) : 0;
}
