// capi_tune.inc -- tuning / measurement / test hooks (include/mi355x_simplex_tune.h): not part of the reference boundary.
// Part of simplex_capi.hip (ONE translation unit: included there, in this order).

extern "C" {

// tuning hooks, used by bench.py / the microbenchmark only (not part of the reference boundary)
int         mi355x_tune_variant_count(void) { return update_variant_count(); }
const char *mi355x_tune_variant_name(int v) { return (v >= 0 && v < update_variant_count()) ? update_variant_name(v) : ""; }
int         mi355x_tune_set_variant(int v) { set_update_variant(v); return get_update_variant(); }
int         mi355x_tune_set_select_mode(int mode) { g_select_mode = mode; return g_select_mode; }
int         mi355x_tune_set_ld_extra(int doubles) { g_ld_extra = (doubles > 0 ? doubles : 0) / 16 * 16; return g_ld_extra; }
int         mi355x_tune_set_handover_mode(int mode) { g_handover_mode = mode; return mode; }
int         mi355x_tune_set_batch_mode(int mode) { g_batch_mode = mode; return g_batch_mode; }
int         mi355x_tune_set_alternate_sweep(int on) { set_alternate_sweep(on); return on; }
// pivots one tableau-update launch of this handle applies in its current representation
int         mi355x_tab_block_size(mi355x_tab *t) { return (t && block_mode(t)) ? block_size(t) : 1; }
int         mi355x_debug_rhs(mi355x_tab *t, double *out, int64_t n, int clear)
{
    double *buf = t->v.rhs ? t->v.rhs : t->v.col;          // batches have no rhs buffer: their col buffer
    if (hipMemcpy(out, buf, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (clear) (void)hipMemset(buf, 0, n * sizeof(double));
    return 0;
}
int         mi355x_tune_set_batch_block(int k) { set_batch_block(k); g_batch_block_k = k; return k; }
int         mi355x_tune_set_resident(int mode) { g_resident_mode = (mode == 1 || mode == 2) ? mode : 0; return g_resident_mode; }
#ifdef MI355X_TEST_HOOKS
int         mi355x_tune_set_resident_fault(int on) { set_resident_fault(on); return on; }
#endif
int         mi355x_tune_set_resident_poll(int mode) { set_resident_poll(mode); return mode; }
int         mi355x_tune_set_resident_lds(int mode) { mode = mode > 0 ? 1 : 0; set_resident_lds(mode); return mode; }
int         mi355x_tab_resident(mi355x_tab *t) { return (t && resident_mode(t)) ? 1 : 0; }
int         mi355x_tune_set_lookahead_mode(int mode) { g_la_mode = mode; return g_la_mode; }
int         mi355x_tune_set_block(int k)
{
    // 0: by size; 1: off; 2 .. 16; wide blocks: 24 or 28 (anything else above 16 -> the next smaller size)
    if (k <= 0) g_block_k = 0;
    else if (k <= kMaxBlock) g_block_k = k;
    else g_block_k = k >= 28 ? 28 : (k >= 24 ? 24 : kMaxBlock);
    return g_block_k;
}
int         mi355x_tune_set_sweep_shape(int tr, int nt) { set_sweep_shape(tr, nt); return tr; }
int         mi355x_tune_set_compact(int on) { g_compact_enabled = on ? 1 : 0; return g_compact_enabled; }
int         mi355x_tune_set_sweep_impl(int impl) { set_sweep_impl(impl); return impl; }
int         mi355x_tune_set_sweepw_ring(int on) { set_sweepw_ring(on); return on; }
int         mi355x_tune_set_prime(int on) { set_prime(on); return on; }
int         mi355x_tune_set_sweep_xcd_map(int on) { set_sweep_xmap(on); return on; }
int         mi355x_tune_set_sweep_skew(int rows) { set_sweep_skew(rows); return rows; }
int         mi355x_tune_set_ctl_wait(int mode) { set_ctl_wait(mode); return mode; }
int         mi355x_debug_last_wait(double *out2) { if (!out2) return MI_BAD_ARG; out2[0] = g_last_wait_us[0]; out2[1] = g_last_wait_us[1]; return MI_OK; }
int         mi355x_tune_set_shard_la_split(int mode) { set_shard_la_split(mode); return mode; }
int         mi355x_tune_set_tail_policy(int p) { g_tail_policy = p == 1 ? 1 : 0; return g_tail_policy; }
// exchange mode 2, blocked: the shard's look-ahead of a block as one persistent launch (0 wherever it fits, 1 never);
// a lone shard runs exchange A against its own buffer (what a shard of several pays minus the wire); polls
// before a shard gives a peer up (0: 2^24)
int         mi355x_tune_set_shard_la_block(int mode) { g_cp_la_block = mode == 1 ? 1 : 0; return g_cp_la_block; }
int         mi355x_tune_set_shard_self_hop(int on) { g_cp_self_hop = on ? 1 : 0; return g_cp_self_hop; }
int         mi355x_tune_set_p2p_spins(unsigned n) { g_cp_p2p_spins = n; return (int)n; }
#ifdef MI355X_TEST_HOOKS
int         mi355x_tune_set_shard_la_fault(int step_plus_1) { set_shard_la_fault(step_plus_1); return step_plus_1; }
#endif
int         mi355x_tune_set_colpart_exchange(int mode) { g_cp_exchange = (mode >= 1 && mode <= 3) ? mode : 0; return g_cp_exchange; }
/* measurement aid: the sweep of the CURRENT pending list launched n more times (the list is not
 * consumed by a sweep); average launch duration by HIP events.  Leaves the tableau meaningless. */
int         mi355x_debug_repeat_sweep(mi355x_tab *t, int n, double *avg_us)
{
    if (!t || n < 1 || !avg_us || !t->compact) return MI_BAD_ARG;
    if (hipSetDevice(t->device) != hipSuccess) return MI_HIP_ERROR;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return MI_HIP_ERROR;
    for (int i = 0; i < 3; ++i) (void)launch_sweep(t->c, block_size(t), 1.0, t->stream, 0);
    (void)hipEventRecord(a, t->stream);
    for (int i = 0; i < n; ++i) (void)launch_sweep(t->c, block_size(t), 1.0, t->stream, 0);
    (void)hipEventRecord(b, t->stream);
    (void)hipEventSynchronize(b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    *avg_us = ms * 1e3 / n;
    return MI_OK;
}
// persistent look-ahead: all workgroups on one XCD (1, default) or spread (0); polls before a
// workgroup gives up on a record (0 = default 2^21); test hook: the last workgroup stops
// publishing from step `step_plus_1 - 1` of every block on (0 = off)
int         mi355x_tune_set_la_one_xcd(int on) { set_la_one_xcd(on); return on; }
int         mi355x_tune_set_la_max_spins(unsigned n) { set_la_max_spins(n); return (int)n; }
#ifdef MI355X_TEST_HOOKS
int         mi355x_tune_set_la_fault(int step_plus_1) { set_la_fault(step_plus_1); return step_plus_1; }
#endif
// how often an exchange of the persistent look-ahead was lost on this handle (it then runs the
// two-launch look-ahead until it is re-armed: enqueue_block)
int         mi355x_tab_la_lost(const mi355x_tab *t) { return t ? t->la_losses : 0; }
// workgroups of the handle's last persistent look-ahead launch (la_launch_workgroups; 0: none so far)
int         mi355x_tab_la_workgroups(const mi355x_tab *t) { return t ? t->la_last_nw : 0; }
// test / measurement aid: clean two-launch blocks before a demoted handle tries the persistent form again
int         mi355x_debug_set_la_rearm(mi355x_tab *t, int64_t blocks) { if (!t) return MI_BAD_ARG; t->la_rearm_in = blocks; return MI_OK; }
// launches enqueued on this handle so far, by class: [0] per-pivot updates, [1] persistent look-ahead
// blocks, [2] two-launch look-ahead blocks, [3] k_sweep16 sweeps, [4] wide sweeps (k_sweepw +
// k_sweepw_rest), [5] short sweeps (k_sweep), [6] resident launches, [7] split selects
int         mi355x_tab_path_counts(const mi355x_tab *t, int64_t *out8)
{
    if (!t || !out8) return MI_BAD_ARG;
    for (int i = 0; i < 8; ++i) out8[i] = t->path_counts[i];
    return MI_OK;
}
// which driver mi355x_batch_solve ran on this batch so far: [0] resident launches, [1] blocks of the split
// form (k_batch_block look-ahead per LP + one k_sweep over all LPs), [2] one-workgroup-per-LP launches
// (k_batch_block / k_batch_solve), [3] lockstep (select, update) launch pairs
int         mi355x_batch_path_counts(const mi355x_batch *b, int64_t *out4)
{
    if (!b || !b->t || !out4) return MI_BAD_ARG;
    out4[0] = b->t->path_counts[kPathResident];
    for (int i = 0; i < 3; ++i) out4[1 + i] = b->t->batch_counts[i];
    return MI_OK;
}
#ifdef MI355X_TEST_HOOKS
// one arithmetic primitive of the exact kernels (kernels_exact.inc) over n operand tuples, one launch
// (limbs per element: 4 for mi355x_test_xarith, 8 for mi355x_test_xarith8)
static int  x_arith_probe(int limbs, int op, int64_t n, const int64_t *a, const int64_t *b, int64_t *out, int32_t *rc, int device)
{
    if (op < 0 || op >= (limbs == 4 ? (int)kXProbeOps : (int)kXProbe8Ops) || n < 1 || n > (1 << 24) || !a || !b || !out || !rc)
        return fail(MI_BAD_ARG, "bad opcode, count or NULL array");
    int st = x_check_device(device);
    if (st != MI_OK) return st;
    if (hipSetDevice(device) != hipSuccess) return fail(MI_HIP_ERROR, "hipSetDevice failed");
    const size_t bytes = (size_t)n * limbs * sizeof(int64_t);
    int64_t *da = nullptr, *db = nullptr, *dout = nullptr;
    int32_t *drc = nullptr;
    hipError_t e = hipMalloc(&da, bytes);
    if (e == hipSuccess) e = hipMalloc(&db, bytes);
    if (e == hipSuccess) e = hipMalloc(&dout, bytes);
    if (e == hipSuccess) e = hipMalloc(&drc, (size_t)n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(da, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (limbs == 4) launch_x_arith_probe(op, n, da, db, dout, drc, nullptr);
        else            launch_x_arith_probe8(op, n, da, db, dout, drc, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rc, drc, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout); (void)hipFree(drc);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? MI_NO_MEMORY : MI_HIP_ERROR, "mi355x_test_xarith: %s", hipGetErrorString(e));
    return MI_OK;
}
int         mi355x_test_xarith(int op, int64_t n, const int64_t *a, const int64_t *b, int64_t *out, int32_t *rc, int device)
{
    return x_arith_probe(4, op, n, a, b, out, rc, device);
}
// the primitives of the 256-bit width whose operands or results are 512 bits: elements of eight limbs
int         mi355x_test_xarith8(int op, int64_t n, const int64_t *a, const int64_t *b, int64_t *out, int32_t *rc, int device)
{
    return x_arith_probe(8, op, n, a, b, out, rc, device);
}
#endif

}  // extern "C"
