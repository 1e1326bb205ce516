// capi_colpart.inc -- mi355x_colpart_*: the column-partitioned tableau behind one handle -- run-time binding of RCCL, the exchange modes (all-reduce, rooted broadcast, P2P push), the per-pivot loops, two-phase, download.
// Part of simplex_capi.hip (ONE translation unit: included there, in this order).

// ---- column-partitioned tableau: the whole solve behind one handle ----------------------------
// The driver of the per-shard steps above, in the library (include/mi355x_simplex.h,
// mi355x_colpart_*): per pivot  price -> exchange A -> la_contribute -> exchange B -> la_pivot,
// after 16 pivots (or before the host looks) sweep.  Exchanges: RCCL on the shards' streams when
// every shard has its own device (one host thread per shard in the one-process form, so the
// enqueue work of N shards runs in parallel; in the one-process-per-GPU form the single local
// shard is driven inline), device-local kernels with the same semantics when the shards are
// logical shards of one device.

namespace {

// RCCL is bound at run time, to exactly ONE copy per process: a process that already holds a
// librccl (PyTorch wheels bundle their own, built against their own HIP runtime; two copies in one
// process interpose each other's symbols and corrupt the heap) uses that one, any other process
// (the Lisp host) gets librccl.so.1 of the ROCm installation.  No RCCL at all = MI_RCCL_ERROR from
// the entry points that need it; everything else in the library is unaffected.
struct RcclApi {
    decltype(&ncclGetUniqueId)    GetUniqueId = nullptr;
    decltype(&ncclCommInitRank)   CommInitRank = nullptr;
    decltype(&ncclCommInitAll)    CommInitAll = nullptr;
    decltype(&ncclCommDestroy)    CommDestroy = nullptr;
    decltype(&ncclAllGather)      AllGather = nullptr;
    decltype(&ncclAllReduce)      AllReduce = nullptr;
    decltype(&ncclBroadcast)      Broadcast = nullptr;
    decltype(&ncclCommAbort)      CommAbort = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string path, error;
    bool ok = false;
};

int rccl_find_loaded(struct dl_phdr_info *info, size_t, void *out)
{
    const char *name = info->dlpi_name ? info->dlpi_name : "";
    const char *base = strrchr(name, '/');
    base = base ? base + 1 : name;
    if (strncmp(base, "librccl.so", 10) == 0) { *static_cast<std::string *>(out) = name; return 1; }
    return 0;
}

const RcclApi &rccl()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void *h = nullptr;
        std::string loaded;
        dl_iterate_phdr(rccl_find_loaded, &loaded);
        if (!loaded.empty()) { h = dlopen(loaded.c_str(), RTLD_NOW | RTLD_NOLOAD); api.path = loaded; }
        for (const char *cand : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) {
            if (h) break;
            h = dlopen(cand, RTLD_NOW | RTLD_LOCAL);
            if (h) api.path = cand;
        }
        if (!h) { api.error = "no librccl found (dlopen: " + std::string(dlerror() ? dlerror() : "?") + ")"; return; }
#define MI_RCCL_SYM(name)                                                              \
        api.name = reinterpret_cast<decltype(api.name)>(dlsym(h, "nccl" #name));        \
        if (!api.name) { api.error = "nccl" #name " missing in " + api.path; return; }
        MI_RCCL_SYM(GetUniqueId) MI_RCCL_SYM(CommInitRank) MI_RCCL_SYM(CommInitAll) MI_RCCL_SYM(CommDestroy)
        MI_RCCL_SYM(AllGather) MI_RCCL_SYM(AllReduce) MI_RCCL_SYM(Broadcast) MI_RCCL_SYM(CommAbort)
        MI_RCCL_SYM(GetErrorString)
#undef MI_RCCL_SYM
        api.ok = true;
    });
    return api;
}

#define RCCL_NEED()                                                                            \
    do {                                                                                       \
        if (!rccl().ok) return fail(MI_RCCL_ERROR, "RCCL unavailable: %s", rccl().error.c_str()); \
    } while (0)

#define RCCL_TRY(expr)                                                                         \
    do {                                                                                       \
        ncclResult_t r_ = (expr);                                                              \
        if (r_ != ncclSuccess)                                                                 \
            return fail(MI_RCCL_ERROR, "%s failed: %s (%s:%d)", #expr, rccl().GetErrorString(r_), \
                        __FILE__, __LINE__);                                                   \
    } while (0)

// exchange B on one device: out[r] = sum over the shards of their contributions (owner's bit
// patterns + zeros), exactly what the int64 SUM all-reduce delivers to every rank
__global__ __launch_bounds__(256) void k_local_sum(const long long *all, long long *out, int64_t rows, int n)
{
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows;
         r += (int64_t)gridDim.x * blockDim.x) {
        long long acc = 0;
        for (int s = 0; s < n; ++s) acc += all[(int64_t)s * rows + r];
        out[r] = acc;
    }
}

// ---- exchange mode 2: the shards write straight into each other's memory (P2P over xGMI) -----------
// No collective and no host in the loop: every shard owns ONE fine-grained exchange buffer that its
// peers can write (peer access within a process, IPC handles between processes), laid out as
//     pairs  [2 parities][world][4 granules]     the local pricing winners (exchange A)
//     column [2 parities][2 x rows granules]     the entering column (exchange B)
// with every granule {tag = epoch of the pivot, 32 bits of payload} written by one 8-byte
// system-scope store and polled with system-scope loads until the tag matches -- self-validating,
// so nothing depends on the order in which stores from another GPU become visible, and there is no
// flag, fence or counter.  Producers never wait for anybody (a shard's pricing precedes its own
// waits in its stream), so the scheme cannot deadlock; a shard can run at most one pivot ahead of
// the slowest one (it needs that one's pair to go on), hence two parities.
// (layout and tag conventions: P2pLayout / P2pArgs in simplex_kernels.h.  The blocked shard steps run
// FUSED -- the pricing kernel pushes the pair, the contribution kernel waits for the pairs and pushes
// the column, the split look-ahead step waits for the column: four launches per pivot and shard; the
// kernels below are the unfused forms, used by the per-pivot path, the one-workgroup look-ahead step
// of small shards and the drive-out pivots of the two-phase hand-over)
__device__ __forceinline__ void st_sys(unsigned long long *p, unsigned long long v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned long long ld_sys(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// exchange A, producer: my (key, global column) pair into slot `rank` of EVERY shard's buffer
// (only while the solve is running: iterations enqueued blind behind the terminating pivot must
// not overwrite, with later tags, a pair some peer has not polled yet)
__global__ __launch_bounds__(64) void k_p2p_push_pair(const Ctl *ctl, const double *send2, unsigned long long *const *peers,
                                                      P2pLayout lay, int rank, unsigned epoch)
{
    const int r = threadIdx.x;
    if (ctl->status != kRunning || r >= lay.world) return;
    const unsigned long long kb = (unsigned long long)__double_as_longlong(send2[0]);
    const unsigned long long cb = (unsigned long long)__double_as_longlong(send2[1]);
    unsigned long long *dst = peers[r] + lay.pair_off(epoch & 1u, rank);
    const unsigned long long tg = (unsigned long long)epoch << 32;
    st_sys(dst + 0, tg | (kb & 0xffffffffull));
    st_sys(dst + 1, tg | (kb >> 32));
    st_sys(dst + 2, tg | (cb & 0xffffffffull));
    st_sys(dst + 3, tg | (cb >> 32));
}
// exchange A, consumer: wait for every shard's pair of this pivot -> the plain `gathered` array
__global__ __launch_bounds__(64) void k_p2p_wait_pairs(Ctl *ctl, const unsigned long long *mine, P2pLayout lay,
                                                       unsigned epoch, double *gathered, unsigned max_spins)
{
    const int r = threadIdx.x;
    if (ctl->status != kRunning || r >= lay.world) return;      // (iterations enqueued past termination: no-ops)
    const unsigned long long *src = mine + lay.pair_off(epoch & 1u, r);
    unsigned long long g[4];
    for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) { g[k] = ld_sys(src + k); ok &= (unsigned)(g[k] >> 32) == epoch; }
        if (ok) break;
        if (spins > max_spins) { ctl->status = kExchangeLost; return; }
    }
    gathered[2 * r]     = __longlong_as_double((long long)(((g[1] & 0xffffffffull) << 32) | (g[0] & 0xffffffffull)));
    gathered[2 * r + 1] = __longlong_as_double((long long)(((g[3] & 0xffffffffull) << 32) | (g[2] & 0xffffffffull)));
}
// exchange B, producer: the shard that owns the entering column (the contribution kernel left its
// bit patterns in `bits`; everybody else holds zeros there and stays silent) writes it to every shard
__global__ __launch_bounds__(256) void k_p2p_push_column(TabView t, const long long *bits, const int64_t *ec_dev,
                                                         int64_t col_offset, unsigned long long *const *peers,
                                                         P2pLayout lay, unsigned epoch)
{
    const int64_t ec = *ec_dev;
    if (ec < 0) return;
    const int64_t lc = t.l2p ? t.l2p[ec] : ec - col_offset;
    if (!(lc >= 0 && lc < t.cols - 1)) return;                  // not mine
    const unsigned long long tg = (unsigned long long)epoch << 32;
    const int64_t off = lay.col_off(epoch & 1u);
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < t.rows; r += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long vb = (unsigned long long)bits[r];
        for (int q = 0; q < lay.world; ++q) {
            unsigned long long *dst = peers[q] + off + 2 * r;
            st_sys(dst, tg | (vb & 0xffffffffull));
            st_sys(dst + 1, tg | (vb >> 32));
        }
    }
}
// exchange B, consumer: wait for the column of this pivot -> the plain `bits_in` array
__global__ __launch_bounds__(256) void k_p2p_wait_column(Ctl *ctl, const int64_t *ec_dev, const unsigned long long *mine,
                                                         P2pLayout lay, unsigned epoch, int64_t rows, long long *bits_in,
                                                         unsigned max_spins)
{
    if (ctl->status != kRunning || *ec_dev < 0) return;         // nothing enters (every shard decides the same)
    const unsigned long long *src = mine + lay.col_off(epoch & 1u);
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        unsigned long long lo, hi;
        for (unsigned spins = 0;; ++spins) {
            lo = ld_sys(src + 2 * r);
            hi = ld_sys(src + 2 * r + 1);
            if ((unsigned)(lo >> 32) == epoch && (unsigned)(hi >> 32) == epoch) break;
            if (spins > max_spins) { ctl->status = kExchangeLost; return; }
        }
        bits_in[r] = (long long)(((hi & 0xffffffffull) << 32) | (lo & 0xffffffffull));
    }
}

struct CpShard {
    mi355x_tab *t = nullptr;
    int         device = 0, index = 0;        // physical device, global shard index
    int64_t     col_begin = 0, col_end = 0;   // global logical columns (dense) / initial columns (compact)
    double     *send = nullptr, *gathered = nullptr;
    long long  *bits = nullptr, *bits_in = nullptr;   // contribution / exchanged column
    int64_t    *ec = nullptr;
    ncclComm_t  comm = nullptr;
    double     *h_gathered = nullptr;         // pinned: the all-gathered winners (exchange B as a rooted broadcast)
    // exchange mode 2 (P2P): my fine-grained exchange buffer, the device array of every shard's
    // buffer address as THIS process maps it, and what had to be opened through IPC
    unsigned long long  *xch = nullptr;
    unsigned long long **d_peers = nullptr;
    std::vector<void *>  ipc_opened;
    // k_shard_la_block: this shard's entry of the launch array in device memory (logical shards: the first
    // shard's buffer holds the entries of all of them -- they go in ONE launch)
    ShardLaunch *d_launch = nullptr;
    ShardLaunch  h_launch{};                   // what the device copy of this shard's entry holds (uploads only when it changes)
    bool         h_launch_valid = false;
    bool        aborted = false;              // its communicator was aborted after a failure: no stream syncs
    // exchange timing (mi355x_colpart_exchange_timing): event quads around the two collectives of
    // sampled pivots -- [before all-gather, after, before all-reduce, after]
    std::vector<hipEvent_t> ev;
    int ev_used = 0;
};

}  // namespace

struct mi355x_colpart {
    int     world = 1;                       // shards in total
    bool    rccl = false, multi_process = false, compact = false;
    bool    unit_dense = false;              // dense shards that cp_make_dense filled from compact ones and no pivot
                                             // of the solve loop has touched since: basic columns = unit vectors, +-0 elsewhere
    int64_t rows = 0, var_count = 0;
    int     block = kMaxBlock, j = 0;        // pivots per sweep, steps of the current block enqueued
    int     is_max = 1;
    int     timing_stride = 0;               // 0 = no exchange timing, k = every k-th pivot
    int     exchange = 0;                    // g_cp_exchange when the handle was created (3 -> 2 with p2p_merged off)
    bool    p2p_merged = true;               // mode 2: a shard that has its device to itself steps in two launches
    unsigned xepoch = 0;                     // P2P exchange: pivots exchanged so far (the granules' tags)
    unsigned p2p_spins = 1u << 24;           // polls before a shard gives a peer up (kExchangeLost)
    bool     p2p_connected = false;          // mode 2: every peer's buffer is mapped
    P2pLayout lay{};
    std::vector<CpShard> sh;                 // the shards of THIS process
    // logical shards: one allocation each, shared by all of them
    double    *l_gathered = nullptr;
    long long *l_bits_all = nullptr, *l_bits_sum = nullptr;
    std::vector<int> thread_rc;
    // exchange mode 2, blocked: the look-ahead of a whole block as ONE persistent launch per device
    // (k_shard_la_block) -- the knob as it was at creation (0 by size, 1 never, 2 whenever it fits), the epoch
    // base of the next launch's local records, and what single tableaux keep per handle: an exchange was lost
    // (the handle then runs the two-launch step until la_rearm_in clean blocks have gone by)
    int      la_block_mode = 0;
    int      self_hop = 0;                   // a lone shard runs exchange A against its own buffer (measurement: a shard of N minus the wire)
    unsigned la_epoch = 1;
    bool     la_lost = false;
    int      la_losses = 0;
    int64_t  la_rearm_in = 0;
    int64_t  la_blocks = 0;                  // blocks enqueued through k_shard_la_block (mi355x_colpart_la_stats)
    bool    dead = false;                    // communicators aborted after a failure: only destroy is left
    std::atomic<int> cancel{0};              // mi355x_colpart_cancel (any thread; one-process forms)
};

namespace {

void cp_free(mi355x_colpart *p)
{
    if (!p) return;
    for (CpShard &s : p->sh) {
        // (a shard whose communicator had to be aborted may have collectives on its stream that
        // can never complete: do not wait for them)
        if (s.t && !s.aborted) { (void)hipSetDevice(s.device); (void)hipStreamSynchronize(s.t->stream); }
        if (s.comm && rccl().ok) (void)rccl().CommDestroy(s.comm);
        for (hipEvent_t e : s.ev) (void)hipEventDestroy(e);
        if (s.h_gathered) (void)hipHostFree(s.h_gathered);
        for (void *q : s.ipc_opened) (void)hipIpcCloseMemHandle(q);
        if (s.xch) { (void)hipSetDevice(s.device); (void)hipFree(s.xch); }
        if (s.d_peers) { (void)hipSetDevice(s.device); (void)hipFree(s.d_peers); }
        if (s.d_launch) { (void)hipSetDevice(s.device); (void)hipFree(s.d_launch); }
        if (s.aborted && s.t) s.t->own_stream = nullptr;   // free_tab must not synchronise / destroy it either
    }
    for (CpShard &s : p->sh) {
        (void)hipSetDevice(s.device);
        if (p->rccl) { (void)hipFree(s.send); (void)hipFree(s.gathered); (void)hipFree(s.bits); }
        (void)hipFree(s.ec);
        if (s.t) free_tab(s.t);
    }
    if (!p->sh.empty()) (void)hipSetDevice(p->sh[0].device);
    (void)hipFree(p->l_gathered);
    (void)hipFree(p->l_bits_all);
    (void)hipFree(p->l_bits_sum);
    delete p;
}

// [begin, end) of shard r of n over `count` columns, sizes differing by at most one
void cp_partition(int64_t count, int n, int r, int64_t *b, int64_t *e)
{
    const int64_t base = count / n, extra = count % n;
    *b = r * base + std::min<int64_t>(r, extra);
    *e = *b + base + (r < extra ? 1 : 0);
}

// One process per GPU, exchange mode 2: map the other ranks' exchange buffers (`handles`: world x
// 64 bytes, the hipIpcMemHandle_t of every rank's buffer in rank order, this rank's own included)
int cp_p2p_connect(mi355x_colpart *p, const char *handles)
{
    CpShard &s = p->sh[0];
    HIP_TRY(hipSetDevice(s.device));
    std::vector<unsigned long long *> ptrs((size_t)p->world, nullptr);
    ptrs[(size_t)s.index] = s.xch;
    for (int r = 0; r < p->world; ++r) {
        if (r == s.index) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, handles + (size_t)64 * r, 64);
        void *q = nullptr;
        HIP_TRY(hipIpcOpenMemHandle(&q, h, hipIpcMemLazyEnablePeerAccess));
        s.ipc_opened.push_back(q);
        ptrs[(size_t)r] = (unsigned long long *)q;
    }
    HIP_TRY(hipMemcpy(s.d_peers, ptrs.data(), p->world * sizeof(unsigned long long *), hipMemcpyHostToDevice));
    p->p2p_connected = true;
    return MI_OK;
}

// Exchange mode 2: one fine-grained buffer per shard, every shard's address of every buffer.
// One process: the shards' devices get peer access to each other.  One process per GPU: the IPC
// handle of this rank's buffer is all-gathered over the (already initialised) communicator and the
// other ranks' buffers are opened -- set-up only, the pivots themselves use no collective.
int cp_setup_p2p(mi355x_colpart *p)
{
    // (the pair kernels index by threadIdx.x < world on one wave and stage 2 x 64 doubles in LDS)
    if (p->world > 64)
        return fail(MI_BAD_ARG, "exchange mode 2 (P2P push) supports at most 64 shards, not %d", p->world);
    p->lay.world = p->world;
    p->lay.rows_p = (p->rows + 7) / 8 * 8;
    const size_t bytes = (size_t)p->lay.granules() * sizeof(unsigned long long);
    for (CpShard &s : p->sh) {
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipExtMallocWithFlags((void **)&s.xch, bytes, hipDeviceMallocFinegrained));
        HIP_TRY(hipMemset(s.xch, 0, bytes));
        HIP_TRY(hipMalloc((void **)&s.d_peers, p->world * sizeof(unsigned long long *)));
        // (the first local shard's array has room for all local shards: logical shards go in ONE launch)
        HIP_TRY(hipMalloc((void **)&s.d_launch, p->sh.size() * sizeof(ShardLaunch)));
    }
    p->la_block_mode = g_cp_la_block;
    p->self_hop = g_cp_self_hop;
    p->p2p_spins = g_cp_p2p_spins ? g_cp_p2p_spins : (1u << 24);
    std::vector<unsigned long long *> ptrs((size_t)p->world, nullptr);
    if (!p->multi_process) {
        for (CpShard &s : p->sh) ptrs[(size_t)s.index] = s.xch;
        if (p->rccl)                                          // distinct devices: let them write to each other
            for (CpShard &a : p->sh) {
                HIP_TRY(hipSetDevice(a.device));
                for (CpShard &b : p->sh) {
                    if (a.device == b.device) continue;
                    const hipError_t e = hipDeviceEnablePeerAccess(b.device, 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                        return fail(MI_HIP_ERROR, "no peer access from device %d to device %d: %s", a.device, b.device,
                                    hipGetErrorString(e));
                    (void)hipGetLastError();
                }
            }
        for (CpShard &s : p->sh) {
            HIP_TRY(hipSetDevice(s.device));
            HIP_TRY(hipMemcpy(s.d_peers, ptrs.data(), p->world * sizeof(unsigned long long *), hipMemcpyHostToDevice));
        }
        p->p2p_connected = true;
        return MI_OK;
    }
    CpShard &s = p->sh[0];
    HIP_TRY(hipSetDevice(s.device));
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    if (p->world == 1) {
        ptrs[0] = s.xch;
        HIP_TRY(hipMemcpy(s.d_peers, ptrs.data(), sizeof(unsigned long long *), hipMemcpyHostToDevice));
        p->p2p_connected = true;
        return MI_OK;
    }
    if (!s.comm) return MI_OK;             // no communicator: the host passes the handles (mi355x_colpart_p2p_connect)
    RCCL_NEED();
    hipIpcMemHandle_t mine;
    HIP_TRY(hipIpcGetMemHandle(&mine, s.xch));
    char *d_buf = nullptr;                                    // [mine | everybody's], freed on every way out
    HIP_TRY(hipMalloc((void **)&d_buf, (size_t)64 * (p->world + 1)));
    struct Free { char *q; ~Free() { (void)hipFree(q); } } guard{d_buf};
    char *d_one = d_buf, *d_all = d_buf + 64;
    HIP_TRY(hipMemcpy(d_one, &mine, 64, hipMemcpyHostToDevice));
    RCCL_TRY(rccl().AllGather(d_one, d_all, 64, ncclChar, s.comm, s.t->stream));
    HIP_TRY(hipStreamSynchronize(s.t->stream));
    std::vector<char> all((size_t)64 * p->world);
    HIP_TRY(hipMemcpy(all.data(), d_all, (size_t)64 * p->world, hipMemcpyDeviceToHost));
    return cp_p2p_connect(p, all.data());
}

// the two exchanges of one pivot in mode 2, on shard s's stream (epoch = the pivot's tag)
int cp_p2p_push_pair(mi355x_colpart *p, CpShard &s, unsigned epoch)
{
    hipLaunchKernelGGL(k_p2p_push_pair, dim3(1), dim3(64), 0, s.t->stream, s.t->v.ctl, s.send, s.d_peers, p->lay, s.index, epoch);
    hipLaunchKernelGGL(k_p2p_wait_pairs, dim3(1), dim3(64), 0, s.t->stream, s.t->v.ctl, s.xch, p->lay, epoch, s.gathered,
                       p->p2p_spins);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
int cp_p2p_push_wait_pairs_split(mi355x_colpart *p, CpShard &s, unsigned epoch, bool push)
{
    if (push) hipLaunchKernelGGL(k_p2p_push_pair, dim3(1), dim3(64), 0, s.t->stream, s.t->v.ctl, s.send, s.d_peers, p->lay, s.index, epoch);
    else      hipLaunchKernelGGL(k_p2p_wait_pairs, dim3(1), dim3(64), 0, s.t->stream, s.t->v.ctl, s.xch, p->lay, epoch,
                                 s.gathered, p->p2p_spins);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}
int cp_p2p_column(mi355x_colpart *p, CpShard &s, unsigned epoch, bool push, bool wait)
{
    int blocks = (int)((p->rows + 255) / 256);
    if (blocks > 256) blocks = 256;
    if (push) hipLaunchKernelGGL(k_p2p_push_column, dim3(blocks), dim3(256), 0, s.t->stream, s.t->v, s.bits, s.ec,
                                 s.col_begin, s.d_peers, p->lay, epoch);
    if (wait) hipLaunchKernelGGL(k_p2p_wait_column, dim3(blocks), dim3(256), 0, s.t->stream, s.t->v.ctl, s.ec, s.xch,
                                 p->lay, epoch, p->rows, s.bits_in, p->p2p_spins);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// exchange buffers (+ communicators, unless they are handed over from another handle) once the
// shards' handles exist
int cp_finish_setup(mi355x_colpart *p, const void *id128, int rank, bool make_comms = true)
{
    const int nl = (int)p->sh.size();
    // pivots per sweep of a shard's slice: the knob, or by the size of a shard (the block structure is
    // local to a shard -- the exchanges are per pivot -- so ranks need not even agree on it)
    if (g_block_k > 1) p->block = g_block_k;
    else if (g_block_k == 1) p->block = 1;
    else {
        // (a shard's step is dearer than a single tableau's look-ahead step: wide blocks from 0.75 GB of
        // shard on, where they were measured -- not from the single tableau's 240 MiB)
        int w = 0;
        if (nl > 0 && p->sh[0].t) {
            const TabView &v0 = p->sh[0].t->v;
            const double sb = (double)v0.rows * (double)v0.ld * 8.0;
            if (sb >= 768.0 * 1024 * 1024 && wide_block_default(v0)) w = sb >= 8e9 ? 28 : 24;
        }
        p->block = w ? w : kMaxBlock;
    }
    if (!p->rccl) {
        HIP_TRY(hipSetDevice(p->sh[0].device));
        HIP_TRY(hipMalloc((void **)&p->l_gathered, 2 * p->world * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&p->l_bits_all, (size_t)p->world * p->rows * sizeof(long long)));
        HIP_TRY(hipMalloc((void **)&p->l_bits_sum, p->rows * sizeof(long long)));
        HIP_TRY(hipMemset(p->l_gathered, 0, 2 * p->world * sizeof(double)));
        for (CpShard &s : p->sh) {
            s.send = p->l_gathered + 2 * s.index;           // "all-gather" = everyone writes its slot
            s.gathered = p->l_gathered;
            s.bits = p->l_bits_all + (int64_t)s.index * p->rows;
            s.bits_in = p->l_bits_sum;
            HIP_TRY(hipMalloc((void **)&s.ec, sizeof(int64_t)));
        }
        // the logical shards run one after the other on ONE stream (that of the first)
        for (CpShard &s : p->sh) s.t->stream = p->sh[0].t->own_stream;
        return p->exchange == 2 ? cp_setup_p2p(p) : MI_OK;
    }
    if (!(p->multi_process && !id128 && p->exchange == 2)) RCCL_NEED();
    for (CpShard &s : p->sh) {
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipMalloc((void **)&s.send, 2 * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&s.gathered, 2 * p->world * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&s.bits, p->rows * sizeof(long long)));
        HIP_TRY(hipMalloc((void **)&s.ec, sizeof(int64_t)));
        HIP_TRY(hipHostMalloc((void **)&s.h_gathered, 2 * p->world * sizeof(double)));
        s.bits_in = s.bits;                                  // all-reduce / broadcast in place
    }
    if (!make_comms) return p->exchange == 2 ? cp_setup_p2p(p) : MI_OK;
    if (p->multi_process) {
        if (id128) {                                         // (NULL: exchange mode 2 without a communicator)
            ncclUniqueId id;
            memcpy(&id, id128, sizeof id);
            HIP_TRY(hipSetDevice(p->sh[0].device));
            RCCL_TRY(rccl().CommInitRank(&p->sh[0].comm, p->world, id, rank));
        }
    } else {
        std::vector<ncclComm_t> comms((size_t)nl);
        std::vector<int> devs((size_t)nl);
        for (int i = 0; i < nl; ++i) devs[(size_t)i] = p->sh[(size_t)i].device;
        RCCL_TRY(rccl().CommInitAll(comms.data(), nl, devs.data()));
        for (int i = 0; i < nl; ++i) p->sh[(size_t)i].comm = comms[(size_t)i];
    }
    return p->exchange == 2 ? cp_setup_p2p(p) : MI_OK;
}

// ---- one pivot, as the three local steps of shard s with the exchanges between them
int cp_price(mi355x_colpart *p, CpShard &s)
{
    return mi355x_shard_price(s.t, p->is_max, s.col_begin, s.send);
}
int cp_contribute(mi355x_colpart *p, CpShard &s, double f)
{
    if (p->block > 1)
        return mi355x_shard_la_contribute(s.t, p->j, s.gathered, p->world, s.col_begin, f,
                                          (int64_t *)s.bits, s.ec);
    return mi355x_shard_contribute(s.t, s.gathered, p->world, s.col_begin, f, (int64_t *)s.bits, s.ec);
}
int cp_pivot(mi355x_colpart *p, CpShard &s, double f)
{
    if (p->block > 1) return mi355x_shard_la_pivot(s.t, p->j, (const int64_t *)s.bits_in, s.ec, f);
    return mi355x_shard_pivot(s.t, (const int64_t *)s.bits_in, s.ec, f);
}

// The rank whose (key, global column) pair wins the pricing -- vi_min's rule on the host: an empty
// pair (column -1) loses against anything, a NaN-in-column-0 marker (-2) or no candidate at all
// means nobody enters a column, and any root will do (everybody contributes zeros).
int cp_winner_rank(const double *g, int world)
{
    int best = -1;
    for (int k = 0; k < world; ++k) {
        const double v = g[2 * k], c = g[2 * k + 1];
        if (c < 0.0) continue;
        if (best < 0 || v < g[2 * best] || (v == g[2 * best] && c < g[2 * best + 1])) best = k;
    }
    return best < 0 ? 0 : best;
}

// Exchange mode 2, blocked shards: one pivot of shard s as its three fused phases --
//   0  pricing kernel, which also pushes this shard's pair into every shard's buffer
//   1  contribution kernel: waits for all pairs, chains, and (the owner) pushes the column
//   2  the look-ahead step: its split form waits for the column itself; the one-workgroup form of
//      small shards takes it from the (unfused) wait kernel
// On ONE stream (logical shards) phase k of every shard is enqueued before phase k + 1 of any.
int cp_fused_p2p_step(mi355x_colpart *p, CpShard &s, double f, int j, unsigned epoch, int phase)
{
    P2pArgs x;
    x.peers = s.d_peers; x.mine = s.xch; x.lay = p->lay; x.rank = s.index; x.epoch = epoch; x.max_spins = p->p2p_spins;
    if (phase == 0) return shard_price_x(s.t, p->is_max, s.col_begin, s.send, x);
    if (phase == 1) return shard_la_contribute_x(s.t, j, s.gathered, p->world, s.col_begin, f, (int64_t *)s.bits, s.ec, x);
    if (shard_la_split(s.t->v)) return shard_la_pivot_x(s.t, j, (const int64_t *)s.bits_in, s.ec, f, x);
    int rc = cp_p2p_column(p, s, epoch, false, true);
    if (rc != MI_OK) return rc;
    return mi355x_shard_la_pivot(s.t, j, (const int64_t *)s.bits_in, s.ec, f);
}

// Exchange mode 2, blocked: the step of shard s as TWO launches (k_shard_p2p_step + k_shard_la_scale)
// where a consumer and the producer it waits for may be the same kernel on different shards -- a
// shard that has its device (or at least its stream) to itself, or the only shard there is.
// Returns > 0: done; 0: this shard / state needs the separate launches; < 0: an error.
int cp_try_merged_step(mi355x_colpart *p, CpShard &s, double f, int j, unsigned epoch)
{
    mi355x_tab *t = s.t;
    const int np = (p->p2p_merged && t->n_part > 0 && t->part_is_max == (p->is_max ? 1 : 0)) ? t->n_part : 0;
    if (!(np > 0 && t->v.blk && j < kWideBlock)) return 0;
    P2pArgs x;
    x.peers = s.d_peers; x.mine = s.xch; x.lay = p->lay; x.rank = s.index; x.epoch = epoch; x.max_spins = p->p2p_spins;
    int rc = use_device(t);
    if (rc == MI_OK) rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    t->shard_is_max = p->is_max ? 1 : 0;
    t->v.col_bias = t->v.p2l ? 0 : s.col_begin;
    const int left = launch_shard_p2p_step(t->v, j, np, p->world, s.col_begin, f, t->shard_is_max, s.ec, t->stream, x);
    if (left > 0) {
        if (j + 1 > t->shard_steps) t->shard_steps = j + 1;     // (what mi355x_shard_la_pivot records)
        t->n_part = left;
        t->part_is_max = t->shard_is_max;
        HIP_TRY(hipGetLastError());
    }
    return left;
}

// ---- exchange mode 2, blocked: the look-ahead of a whole block as ONE persistent launch per device ------
// (k_shard_la_block, kernels_shard_block.inc).  One launch covers the device-local shards: ONE where a shard
// has its GPU to itself (one process per GPU; one process with a GPU per shard), all logical shards of a
// one-GPU box together -- the workgroups of one launch are co-resident by construction as long as there are
// no more of them than CUs (each takes a CU's LDS), which is what lets shards that WAIT for each other inside
// a kernel share a device at all.  Every launch is a whole block (k <= p->block steps) followed by the
// shard's sweep under the launch's stamp: p->j stays 0 on this path.
constexpr unsigned kCpLaEpochStep = 2 * kLaBlockMax + 2;

int cp_cu_count(int device)
{
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

// may the next blocks of this handle go through k_shard_la_block?
bool cp_la_block_live(mi355x_colpart *p)
{
    if (p->exchange != 2 || !p->p2p_merged || p->block < 2 || p->block > kLaBlockMax || p->la_block_mode == 1 || p->la_lost ||
        p->world > 64 || p->sh.empty())
        return false;
    int total = 0;
    for (CpShard &s : p->sh) {
        const int nw = shard_la_block_workgroups(s.t->v);
        if (nw == 0 || !s.d_launch) return false;
        if (p->block > kMaxBlock && !s.t->v.bk_smask2) return false;
        total += nw;
    }
    // shards that share a device go in ONE launch: all its workgroups must be resident together
    if (!p->rccl && p->sh.size() > 1 && total > cp_cu_count(p->sh[0].device)) return false;
    return true;
}

// (re)describe the local shards to the device: the views may have changed since the last call
int cp_upload_launch(mi355x_colpart *p, CpShard &s, ShardLaunch *dst, hipStream_t st)
{
    mi355x_tab *t = s.t;
    int rc = use_device(t);
    if (rc == MI_OK) rc = ensure_dense(t);
    if (rc != MI_OK) return rc;
    t->shard_is_max = p->is_max ? 1 : 0;
    t->v.col_bias = t->v.p2l ? 0 : s.col_begin;
    ShardLaunch h;
    memset(&h, 0, sizeof h);
    h.t = t->v;
    h.peers = s.d_peers;
    h.mine = s.xch;
    h.col_offset = s.col_begin;
    h.rank = s.index;
    if (!s.h_launch_valid || memcmp(&h, &s.h_launch, sizeof h) != 0) {
        HIP_TRY(hipMemcpyAsync(dst, &h, sizeof h, hipMemcpyHostToDevice, st));   // (pageable source: staged before the call returns)
        s.h_launch = h;
        s.h_launch_valid = true;
    }
    return MI_OK;
}

// nb blocks (the last one `tail` steps, the others p->block) of the device-local shards sh[first .. first+n)
// behind ONE launch array; epoch0 / xepoch0: the first block's epoch base / exchange tag base
int cp_run_blocks(mi355x_colpart *p, size_t first, size_t n, double f, int64_t n_pivots, unsigned epoch0, unsigned xepoch0)
{
    CpShard &s0 = p->sh[first];
    HIP_TRY(hipSetDevice(s0.device));
    hipStream_t st = s0.t->stream;
    int nw_max = 0;
    for (size_t i = 0; i < n; ++i) {
        CpShard &s = p->sh[first + i];
        const int rc = cp_upload_launch(p, s, s0.d_launch + i, st);
        if (rc != MI_OK) return rc;
        nw_max = std::max(nw_max, shard_la_block_workgroups(s.t->v));
    }
    const int hop = (p->world > 1 || p->self_hop) ? 1 : 0;
    unsigned epoch = epoch0, xepoch = xepoch0;
    for (int64_t done = 0; done < n_pivots;) {
        const int k = (int)std::min<int64_t>(p->block, n_pivots - done);
        launch_shard_la_block(s0.d_launch, (int)n, nw_max, p->lay, k, p->is_max, f, epoch, xepoch, p->p2p_spins, hop, st);
        HIP_TRY(hipGetLastError());
        for (size_t i = 0; i < n; ++i) {
            CpShard &s = p->sh[first + i];
            const int rc = shard_sweep_x(s.t, k, epoch, shard_la_block_workgroups(s.t->v));
            if (rc != MI_OK) return rc;
            s.t->la_epoch = epoch + kCpLaEpochStep;          // (a handle's record tags only ever grow)
        }
        epoch += kCpLaEpochStep;
        xepoch += (unsigned)k;
        done += k;
    }
    return MI_OK;
}

// epoch base for `nb` more launches: every local shard's records must never have seen these tags
int cp_la_epochs(mi355x_colpart *p, int64_t nb, unsigned *epoch0)
{
    unsigned e = p->la_epoch;
    for (CpShard &s : p->sh) e = std::max(e, s.t->la_epoch);
    if ((uint64_t)e + (uint64_t)nb * kCpLaEpochStep > 0x7fff0000ull) {   // 32-bit tags: start over on clean records
        for (CpShard &s : p->sh) {
            HIP_TRY(hipSetDevice(s.device));
            HIP_TRY(hipMemsetAsync(s.t->v.la_px, 0, kLaRecordBytes, s.t->stream));
            HIP_TRY(hipMemsetAsync(s.t->v.la_rx, 0, kLaRecordBytes, s.t->stream));
            s.t->la_epoch = 1;
        }
        e = 1;
    }
    *epoch0 = e;
    p->la_epoch = e + (unsigned)nb * kCpLaEpochStep;
    return MI_OK;
}

// n iterations of shard s over RCCL (its own thread in the one-process form).  j0 = step of the
// block the first iteration is; every shard runs the same sequence, so they meet in the collectives.
int cp_run_rccl(mi355x_colpart *p, CpShard &s, double f, int64_t n, int j0)
{
    HIP_TRY(hipSetDevice(s.device));
    int j = j0;
    for (int64_t i = 0; i < n; ++i) {
        const bool timed = p->timing_stride > 0 && i % p->timing_stride == 0 &&
                           (size_t)s.ev_used + 4 <= s.ev.size();
        hipEvent_t *e = timed ? &s.ev[(size_t)s.ev_used] : nullptr;
        const unsigned epoch = p->xepoch + (unsigned)i + 1u;     // (mode 2: the tag of this pivot's granules)
        if (p->exchange == 2 && p->block > 1) {
            // mode 2, blocked: the exchanges are INSIDE the step kernels -- two launches per pivot where
            // the shards' kernels run concurrently (this loop: one shard per device or process), four
            // for the first pivot after an upload and for small shards
            int rc = MI_OK;
            const int left = cp_try_merged_step(p, s, f, j, epoch);
            if (left < 0) return left;
            if (left == 0) {
                rc = cp_fused_p2p_step(p, s, f, j, epoch, 0);
                if (rc == MI_OK) rc = cp_fused_p2p_step(p, s, f, j, epoch, 1);
                if (rc == MI_OK) rc = cp_fused_p2p_step(p, s, f, j, epoch, 2);
            }
            if (rc != MI_OK) return rc;
            if (++j == p->block) {
                rc = mi355x_shard_sweep(s.t);
                if (rc != MI_OK) return rc;
                j = 0;
            }
            continue;
        }
        int rc = mi355x_shard_price(s.t, p->is_max, s.col_begin, s.send);
        if (rc != MI_OK) return rc;
        if (timed) HIP_TRY(hipEventRecord(e[0], s.t->stream));
        if (p->exchange == 2) { if ((rc = cp_p2p_push_pair(p, s, epoch)) != MI_OK) return rc; }
        else RCCL_TRY(rccl().AllGather(s.send, s.gathered, 2, ncclDouble, s.comm, s.t->stream));
        if (timed) HIP_TRY(hipEventRecord(e[1], s.t->stream));
        if (p->block > 1) rc = mi355x_shard_la_contribute(s.t, j, s.gathered, p->world, s.col_begin, f, (int64_t *)s.bits, s.ec);
        else              rc = mi355x_shard_contribute(s.t, s.gathered, p->world, s.col_begin, f, (int64_t *)s.bits, s.ec);
        if (rc != MI_OK) return rc;
        int root = -1;
        if (p->exchange == 1) {
            // exchange B as a rooted broadcast: the root is the rank whose local pricing winner is
            // the global one (lexicographic (key, column) minimum over the all-gathered pairs -- the
            // decision every shard takes on the device).  The host has to look: one stream
            // synchronisation per pivot, the price of a root RCCL wants as a host argument.
            HIP_TRY(hipMemcpyAsync(s.h_gathered, s.gathered, 2 * p->world * sizeof(double),
                                   hipMemcpyDeviceToHost, s.t->stream));
            HIP_TRY(hipStreamSynchronize(s.t->stream));
            root = cp_winner_rank(s.h_gathered, p->world);
        }
        if (timed) HIP_TRY(hipEventRecord(e[2], s.t->stream));
        if (p->exchange == 2) { if ((rc = cp_p2p_column(p, s, epoch, true, true)) != MI_OK) return rc; }
        else if (root >= 0)
            RCCL_TRY(rccl().Broadcast(s.bits, s.bits, (size_t)p->rows, ncclInt64, root, s.comm, s.t->stream));
        else
            RCCL_TRY(rccl().AllReduce(s.bits, s.bits, (size_t)p->rows, ncclInt64, ncclSum, s.comm, s.t->stream));
        if (timed) { HIP_TRY(hipEventRecord(e[3], s.t->stream)); s.ev_used += 4; }
        if (p->block > 1) rc = mi355x_shard_la_pivot(s.t, j, (const int64_t *)s.bits, s.ec, f);
        else              rc = mi355x_shard_pivot(s.t, (const int64_t *)s.bits, s.ec, f);
        if (rc != MI_OK) return rc;
        if (p->block > 1 && ++j == p->block) {
            rc = mi355x_shard_sweep(s.t);
            if (rc != MI_OK) return rc;
            j = 0;
        }
    }
    return MI_OK;
}

// A rank failed between two collectives: the other ranks' streams hold collectives that will never
// complete.  Abort every local communicator (ncclCommAbort tears the kernels down) and mark the
// shards, so that neither this call's caller nor the destroy path waits on those streams.
void cp_abort(mi355x_colpart *p)
{
    if (!p->rccl) return;
    const std::string keep = g_err;
    // (exchange mode 2 without a communicator has nothing to abort, but granules of the failed run
    // were already pushed under tags a later run would reuse: the handle is dead either way)
    for (CpShard &s : p->sh) {
        if (s.comm && rccl().ok) { (void)hipSetDevice(s.device); (void)rccl().CommAbort(s.comm); s.comm = nullptr; }
        s.aborted = true;
    }
    p->dead = true;
    g_err = keep;
}

// enqueue n iterations on every local shard; no host synchronisation
int cp_run(mi355x_colpart *p, double f, int64_t n)
{
    if (p->dead) return fail(MI_RCCL_ERROR, "this handle's communicators were aborted after an earlier failure");
    p->unit_dense = false;                                   // (a pivot on an inf / NaN column writes NaNs into basic columns)
    if (p->exchange == 2 && !p->p2p_connected)
        return fail(MI_BAD_ARG, "exchange mode 2: the ranks' buffers are not connected yet (mi355x_colpart_p2p_connect)");
    if (n <= 0) return MI_OK;
    if (p->la_lost && p->la_rearm_in > 0 && p->j == 0) {        // (counted in pivots: la_rearm_in blocks of p->block)
        p->la_rearm_in -= std::min<int64_t>(p->la_rearm_in, (n + p->block - 1) / p->block);
        if (p->la_rearm_in == 0) p->la_lost = false;
    }
    if (p->j == 0 && cp_la_block_live(p)) {
        // whole blocks through k_shard_la_block: one launch array per device
        const int64_t nb = (n + p->block - 1) / p->block;
        unsigned epoch0 = 0;
        int rc = cp_la_epochs(p, nb, &epoch0);
        if (rc != MI_OK) return rc;
        const unsigned xepoch0 = p->xepoch;
        if (!p->rccl || p->sh.size() == 1) {
            rc = cp_run_blocks(p, 0, p->sh.size(), f, n, epoch0, xepoch0);
            if (rc != MI_OK) { if (p->rccl) cp_abort(p); return rc; }
        } else {
            p->thread_rc.assign(p->sh.size(), MI_OK);
            std::vector<std::string> errs(p->sh.size());
            std::vector<std::thread> th;
            for (size_t i = 0; i < p->sh.size(); ++i)
                th.emplace_back([p, f, n, i, epoch0, xepoch0, &errs]() {
                    p->thread_rc[i] = cp_run_blocks(p, i, 1, f, n, epoch0, xepoch0);
                    if (p->thread_rc[i] != MI_OK) errs[i] = g_err;
                });
            for (auto &x : th) x.join();
            for (size_t i = 0; i < p->sh.size(); ++i)
                if (p->thread_rc[i] != MI_OK) { cp_abort(p); g_err = errs[i]; return p->thread_rc[i]; }
        }
        p->xepoch += (unsigned)n;
        p->la_blocks += nb;
        return MI_OK;
    }
    if (p->rccl) {
        const int j0 = p->j;
        if (p->sh.size() == 1) {
            int rc = cp_run_rccl(p, p->sh[0], f, n, j0);
            if (rc != MI_OK) { cp_abort(p); return rc; }
        } else {
            // one host thread per shard: the shards' launches are enqueued in parallel and every
            // thread issues its own rank's collectives (the standard one-process multi-GPU form)
            p->thread_rc.assign(p->sh.size(), MI_OK);
            std::vector<std::string> errs(p->sh.size());
            std::vector<std::thread> th;
            for (size_t i = 0; i < p->sh.size(); ++i)
                th.emplace_back([p, f, n, j0, i, &errs]() {
                    p->thread_rc[i] = cp_run_rccl(p, p->sh[i], f, n, j0);
                    if (p->thread_rc[i] != MI_OK) errs[i] = g_err;       // g_err is thread-local
                });
            for (auto &x : th) x.join();
            for (size_t i = 0; i < p->sh.size(); ++i)
                if (p->thread_rc[i] != MI_OK) {
                    // the other ranks have enqueued collectives that can never complete now
                    cp_abort(p);
                    g_err = errs[i];
                    return p->thread_rc[i];
                }
        }
        if (p->block > 1) p->j = (int)((j0 + n) % p->block);
        p->xepoch += (unsigned)n;
        return MI_OK;
    }
    // logical shards on one device, one stream: step by step over all of them
    HIP_TRY(hipSetDevice(p->sh[0].device));
    hipStream_t st = p->sh[0].t->stream;
    for (int64_t i = 0; i < n; ++i) {
        int rc;
        const unsigned epoch = ++p->xepoch;
        if (p->exchange == 2 && p->block > 1) {
            // ONE shard in all: nobody to wait for, so the two-launch step is safe on this stream too
            const int left = p->world == 1 ? cp_try_merged_step(p, p->sh[0], f, p->j, epoch) : 0;
            if (left < 0) return left;
            if (left == 0)
                for (int phase = 0; phase < 3; ++phase)
                    for (CpShard &s : p->sh) if ((rc = cp_fused_p2p_step(p, s, f, p->j, epoch, phase)) != MI_OK) return rc;
            if (++p->j == p->block) {
                for (CpShard &s : p->sh) if ((rc = mi355x_shard_sweep(s.t)) != MI_OK) return rc;
                p->j = 0;
            }
            continue;
        }
        for (CpShard &s : p->sh) if ((rc = cp_price(p, s)) != MI_OK) return rc;
        if (p->exchange == 2) {
            // the P2P protocol on one device and ONE stream: all producers of an exchange are
            // enqueued before its consumers, so no consumer ever waits (same kernels, same buffers)
            for (CpShard &s : p->sh) if ((rc = cp_p2p_push_wait_pairs_split(p, s, epoch, true)) != MI_OK) return rc;
            for (CpShard &s : p->sh) if ((rc = cp_p2p_push_wait_pairs_split(p, s, epoch, false)) != MI_OK) return rc;
        }
        for (CpShard &s : p->sh) if ((rc = cp_contribute(p, s, f)) != MI_OK) return rc;
        if (p->exchange == 2) {
            for (CpShard &s : p->sh) if ((rc = cp_p2p_column(p, s, epoch, true, false)) != MI_OK) return rc;
            for (CpShard &s : p->sh) if ((rc = cp_p2p_column(p, s, epoch, false, true)) != MI_OK) return rc;
        } else {
            int blocks = (int)((p->rows + 255) / 256);
            if (blocks > 256) blocks = 256;
            hipLaunchKernelGGL(k_local_sum, dim3(blocks), dim3(256), 0, st, p->l_bits_all, p->l_bits_sum, p->rows, p->world);
        }
        for (CpShard &s : p->sh) if ((rc = cp_pivot(p, s, f)) != MI_OK) return rc;
        if (p->block > 1 && ++p->j == p->block) {
            for (CpShard &s : p->sh) if ((rc = mi355x_shard_sweep(s.t)) != MI_OK) return rc;
            p->j = 0;
        }
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// apply the pending pivots of an unfinished block (the tableau is whole whenever the host looks)
int cp_flush(mi355x_colpart *p)
{
    if (p->block > 1 && p->j > 0) {
        for (CpShard &s : p->sh) {
            int rc = mi355x_shard_sweep(s.t);
            if (rc != MI_OK) return rc;
        }
        p->j = 0;
    }
    return MI_OK;
}

// k_shard_la_block lost an exchange on some local shard (status kSyncLost: its workgroups were not all
// resident together, or a peer's granules never came).  The sweeps behind the launch applied what every
// workgroup of their shard completed; the bookkeeping of a pivot beyond that is taken back per shard
// (k_shard_la_rollback), the handle goes on with the two-launch step (no co-residency needed) and tries the
// persistent form again after la_rearm_in clean blocks -- provided the shards still AGREE on the pivot count
// (the caller checks that for the shards of this process; ranks of the one-process-per-GPU form cannot see
// each other and only go on after the one loss that leaves every rank with nothing committed: the launch's
// first exchange -- the co-residency check -- which precedes a shard's first push).
int cp_recover_lost_block(mi355x_colpart *p)
{
    p->la_lost = true;
    p->la_rearm_in = (int64_t)1024 << (2 * std::min(p->la_losses, 8));
    p->la_losses++;
    for (CpShard &s : p->sh) {
        mi355x_tab *t = s.t;
        HIP_TRY(hipSetDevice(s.device));
        int64_t pend_before = 0, pend_after = 0;
        if (p->multi_process)
            HIP_TRY(hipMemcpyAsync(&pend_before, &t->v.blk->n_pending, sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
        launch_shard_la_rollback(t->v, shard_la_block_workgroups(t->v), t->stream);
        launch_ctl_resume(t->v, t->stream, kSyncLost);
        HIP_TRY(hipGetLastError());
        if (p->multi_process) {
            HIP_TRY(hipMemcpyAsync(&pend_after, &t->v.blk->n_pending, sizeof(int64_t), hipMemcpyDeviceToHost, t->stream));
            HIP_TRY(hipStreamSynchronize(t->stream));
            if (pend_before != 0 || pend_after != 0)
                return fail(MI_RCCL_ERROR, "shard %d lost an exchange inside a block (%lld of its pivots selected, %lld applied): "
                                           "the ranks may disagree on the pivot count", s.index, (long long)pend_before, (long long)pend_after);
        }
        t->n_part = 0;
    }
    return MI_OK;
}

int cp_status(mi355x_colpart *p, int64_t *n_pivots)
{
    int rc = cp_flush(p);
    if (rc != MI_OK) return rc;
    {   // a lost exchange of the persistent block launch (never auto-recovered by mi355x_tab_sync's single-tableau path)
        bool lost = false;
        for (CpShard &s : p->sh) {
            if ((rc = use_device(s.t)) != MI_OK || (rc = read_ctl(s.t)) != MI_OK) return rc;
            lost = lost || s.t->h_ctl->status == kSyncLost;
        }
        if (lost && (rc = cp_recover_lost_block(p)) != MI_OK) return rc;
    }
    int st0 = 0;
    int64_t n0 = 0;
    for (size_t i = 0; i < p->sh.size(); ++i) {
        int64_t n = 0;
        const int st = mi355x_tab_sync(p->sh[i].t, &n);
        if (st < 0) return st;
        if (st == kExchangeLost)
            return fail(MI_RCCL_ERROR, "P2P exchange: a peer's data never arrived at shard %d (after %lld pivots)",
                        p->sh[i].index, (long long)n);
        if (i == 0) { st0 = st; n0 = n; }
        else if (st != st0 || n != n0)
            return fail(MI_HIP_ERROR, "shards disagree: (%d, %lld) vs (%d, %lld)", st0, (long long)n0, st, (long long)n);
    }
    if (n_pivots) *n_pivots = n0;
    return st0;
}

// devices for `world` shards of one process: one each when enough are visible, else all logical on 0.
// MI355X_COLPART_FORCE_RCCL=1 (test hook): a single shard also goes through its RCCL communicator
// (all-gather / all-reduce over one rank), so the collective code path runs on a one-GPU box.
bool cp_one_device_each(int world)
{
    if (world == 1) { const char *e = getenv("MI355X_COLPART_FORCE_RCCL"); return e && e[0] == '1'; }
    return device_count_checked() >= world;
}

}  // namespace

extern "C" {

int mi355x_rccl_unique_id(void *id128)
{
    if (!id128) return fail(MI_BAD_ARG, "id128 is NULL");
    RCCL_NEED();
    ncclUniqueId id;
    RCCL_TRY(rccl().GetUniqueId(&id));
    static_assert(sizeof id == 128, "ncclUniqueId is 128 bytes");
    memcpy(id128, &id, sizeof id);
    return MI_OK;
}

static int cp_create_synthetic(mi355x_colpart **out, int64_t n_vars, int64_t n_cons, uint64_t seed,
                               int world, int rank, int device, const void *id128)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (world < 1 || n_vars < world || n_cons < 1) return fail(MI_BAD_ARG, "need 1 <= shards <= n_vars and n_cons >= 1");
    const bool mp = rank >= 0;
    if (mp && (rank >= world || (!id128 && g_cp_exchange != 2 && g_cp_exchange != 3)))
        return fail(MI_BAD_ARG, "bad rank / id (a NULL id is accepted in exchange mode 2 only: no communicator, "
                                "the host connects the ranks with mi355x_colpart_p2p_handle / _p2p_connect)");
    if (device_count_checked() <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    mi355x_colpart *p = new (std::nothrow) mi355x_colpart;
    if (!p) return fail(MI_NO_MEMORY, "host allocation failed");
    p->world = world;
    p->multi_process = mp;
    // (world == 1 in the one-process-per-GPU form: device-local exchanges, unless the test hook
    // MI355X_COLPART_FORCE_RCCL=1 asks for the one-rank ncclCommInitRank communicator)
    p->rccl = mp ? (world > 1 || cp_one_device_each(1)) : cp_one_device_each(world);
    p->exchange = g_cp_exchange == 3 ? 2 : g_cp_exchange;
    p->p2p_merged = g_cp_exchange != 3;
    // (a lone shard without a communicator exchanges with nobody: it takes the self-push form, whose
    // step is two launches instead of five)
    if (g_cp_exchange == 0 && p->world == 1 && !p->rccl) p->exchange = 2;
    p->compact = true;
    p->rows = n_cons + 1;
    p->var_count = n_vars + n_cons;
    const int first = mp ? rank : 0, last = mp ? rank + 1 : world;
    for (int r = first; r < last; ++r) {
        CpShard s;
        s.index = r;
        s.device = mp ? device : (p->rccl ? r : 0);
        cp_partition(n_vars, world, r, &s.col_begin, &s.col_end);      // compact: the structural columns
        int rc = mi355x_tab_create_synthetic(&s.t, n_vars, n_cons, seed, s.col_begin, s.col_end, s.device);
        if (rc == MI_OK) {
            std::vector<int64_t> cols((size_t)(s.col_end - s.col_begin));
            for (size_t k = 0; k < cols.size(); ++k) cols[k] = s.col_begin + (int64_t)k;
            rc = mi355x_shard_set_compact(s.t, p->var_count, cols.data());
        }
        p->sh.push_back(s);
        if (rc != MI_OK) { cp_free(p); return rc; }
    }
    int rc = cp_finish_setup(p, id128, rank);
    if (rc != MI_OK) { cp_free(p); return rc; }
    *out = p;
    return MI_OK;
}

int mi355x_colpart_create_synthetic(mi355x_colpart **out, int64_t n_vars, int64_t n_cons, uint64_t seed,
                                    int n_devices)
{
    return cp_create_synthetic(out, n_vars, n_cons, seed, n_devices, -1, 0, nullptr);
}

int mi355x_colpart_create_synthetic_rank(mi355x_colpart **out, int64_t n_vars, int64_t n_cons, uint64_t seed,
                                         int world, int rank, int device, const void *id128)
{
    if (rank < 0) return fail(MI_BAD_ARG, "rank < 0");
    return cp_create_synthetic(out, n_vars, n_cons, seed, world, rank, device, id128);
}

int mi355x_colpart_create(mi355x_colpart **out, int64_t rows, int64_t cols, const double *hm,
                          const int64_t *hb, int n_devices)
{
    return mi355x_colpart_create_on(out, rows, cols, hm, hb, n_devices, nullptr);
}

static int cp_create_from_host(mi355x_colpart **out, int64_t rows, int64_t cols, const double *hm,
                               const int64_t *hb, int n_devices, const int *device_ids, bool force_dense,
                               bool make_comms, int force_exchange = -1, int force_rccl = -1);

int mi355x_colpart_create_on(mi355x_colpart **out, int64_t rows, int64_t cols, const double *hm,
                             const int64_t *hb, int n_devices, const int *device_ids)
{
    return cp_create_from_host(out, rows, cols, hm, hb, n_devices, device_ids, false, true);
}

// force_dense: dense shards (every logical column distributed) whatever the basis looks like; make_comms == false:
// the communicators are handed over from another handle; force_exchange / force_rccl >= 0: as that handle's
static int cp_create_from_host(mi355x_colpart **out, int64_t rows, int64_t cols, const double *hm,
                               const int64_t *hb, int n_devices, const int *device_ids, bool force_dense,
                               bool make_comms, int force_exchange, int force_rccl)
{
    if (!out) return fail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    const int64_t m = rows - 1, vc = cols - 1;
    if (!hm || !hb || m < 1 || vc < 1 || n_devices < 1) return fail(MI_BAD_ARG, "bad arguments");
    const int ndev = device_count_checked();
    if (ndev <= 0) return fail(MI_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device_ids && force_rccl != 0) {                         // (force_rccl == 0: logical shards, all on device_ids[0])
        for (int i = 0; i < n_devices; ++i) {
            if (device_ids[i] < 0 || device_ids[i] >= ndev)
                return fail(MI_BAD_ARG, "device %d out of range [0,%d)", device_ids[i], ndev);
            for (int k = 0; k < i; ++k)
                if (device_ids[k] == device_ids[i]) return fail(MI_BAD_ARG, "device %d listed twice", device_ids[i]);
        }
    }
    // compact shards when the basis is a set of exact unit columns (+0.0 in the objective row)
    std::vector<char> basic((size_t)vc, 0);
    bool compact = !force_dense;
    for (int64_t i = 0; i < m && compact; ++i) {
        const int64_t b = hb[i];
        if (b < 0 || b >= vc || basic[(size_t)b]) { compact = false; break; }
        basic[(size_t)b] = 1;
        for (int64_t r = 0; r < rows && compact; ++r) {
            double v = hm[r * cols + b];
            uint64_t bits;
            memcpy(&bits, &v, 8);
            if (bits != (r == i ? 0x3FF0000000000000ull : 0ull)) compact = false;
        }
    }
    std::vector<int64_t> dist;                                   // the columns that are distributed
    for (int64_t c = 0; c < vc; ++c)
        if (!compact || !basic[(size_t)c]) dist.push_back(c);
    if (dist.empty()) return fail(MI_BAD_ARG, "no column to distribute");
    if ((int64_t)dist.size() < n_devices) n_devices = (int)dist.size();   // a shard needs a column: fewer shards (mi355x_colpart_info says how many)
    mi355x_colpart *p = new (std::nothrow) mi355x_colpart;
    if (!p) return fail(MI_NO_MEMORY, "host allocation failed");
    p->world = n_devices;
    p->rccl = force_rccl >= 0 ? force_rccl != 0 : cp_one_device_each(n_devices);
    p->exchange = g_cp_exchange == 3 ? 2 : g_cp_exchange;
    p->p2p_merged = g_cp_exchange != 3;
    // (a lone shard without a communicator exchanges with nobody: it takes the self-push form, whose
    // step is two launches instead of five)
    if (g_cp_exchange == 0 && p->world == 1 && !p->rccl) p->exchange = 2;
    if (force_exchange >= 0) p->exchange = force_exchange;
    p->compact = compact;
    p->rows = rows;
    p->var_count = vc;
    std::vector<double> loc;
    for (int r = 0; r < n_devices; ++r) {
        CpShard s;
        s.index = r;
        // one shard per listed device (default 0 .. n-1); logical shards all live on the first
        s.device = device_ids ? device_ids[p->rccl ? r : 0] : (p->rccl ? r : 0);
        int64_t b, e;
        cp_partition((int64_t)dist.size(), n_devices, r, &b, &e);
        const int64_t nloc = e - b;
        s.col_begin = dist[(size_t)b];                           // dense shards: a contiguous block of columns
        s.col_end = s.col_begin + nloc;
        loc.assign((size_t)(rows * (nloc + 1)), 0.0);
        for (int64_t rr = 0; rr < rows; ++rr) {
            for (int64_t k = 0; k < nloc; ++k) loc[(size_t)(rr * (nloc + 1) + k)] = hm[rr * cols + dist[(size_t)(b + k)]];
            loc[(size_t)(rr * (nloc + 1) + nloc)] = hm[rr * cols + vc];   // own copy of the RHS column
        }
        int rc = mi355x_tab_create(&s.t, rows, nloc + 1, loc.data(), hb, s.device);
        if (rc == MI_OK && compact) rc = mi355x_shard_set_compact(s.t, vc, dist.data() + b);
        p->sh.push_back(s);
        if (rc != MI_OK) { cp_free(p); return rc; }
    }
    int rc = cp_finish_setup(p, nullptr, -1, make_comms);
    if (rc != MI_OK) { cp_free(p); return rc; }
    *out = p;
    return MI_OK;
}

int mi355x_colpart_p2p_handle(mi355x_colpart *p, void *handle64)
{
    if (!p || !handle64) return fail(MI_BAD_ARG, "NULL argument");
    if (p->exchange != 2 || !p->multi_process || p->sh.empty() || !p->sh[0].xch)
        return fail(MI_BAD_ARG, "not a one-process-per-GPU handle in exchange mode 2");
    HIP_TRY(hipSetDevice(p->sh[0].device));
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, p->sh[0].xch));
    memcpy(handle64, &h, 64);
    return MI_OK;
}

int mi355x_colpart_p2p_connect(mi355x_colpart *p, const void *handles)
{
    if (!p || !handles) return fail(MI_BAD_ARG, "NULL argument");
    if (p->exchange != 2 || !p->multi_process || p->sh.empty() || !p->sh[0].xch)
        return fail(MI_BAD_ARG, "not a one-process-per-GPU handle in exchange mode 2");
    if (p->p2p_connected) return MI_OK;
    return cp_p2p_connect(p, static_cast<const char *>(handles));
}

int mi355x_colpart_info(const mi355x_colpart *p, int *n_shards, int *n_devices_used, int *uses_rccl)
{
    if (!p) return fail(MI_BAD_ARG, "handle is NULL");
    if (n_shards) *n_shards = p->world;
    if (n_devices_used) *n_devices_used = p->rccl ? p->world : 1;
    if (uses_rccl) *uses_rccl = p->rccl ? 1 : 0;
    return MI_OK;
}

int mi355x_colpart_solve_async(mi355x_colpart *p, int is_max, double f, int64_t n_pivots, int reset)
{
    if (!p) return fail(MI_BAD_ARG, "handle is NULL");
    if (n_pivots < 0) return fail(MI_BAD_ARG, "n_pivots < 0");
    p->is_max = is_max ? 1 : 0;
    if (reset) {
        int rc = cp_flush(p);
        if (rc != MI_OK) return rc;
        for (CpShard &s : p->sh)
            if ((rc = mi355x_tab_reset(s.t, 0)) != MI_OK) return rc;
    }
    return cp_run(p, f, n_pivots);
}

// pivots per sweep of a shard's slice on this handle (1 = per-pivot updates)
int mi355x_colpart_block_size(const mi355x_colpart *p) { return p ? p->block : 0; }

// measurement aid: n doubles of local shard `shard`'s scratch rhs buffer (the per-phase clocks of a
// -DMI355X_LA_TIMING build of k_shard_la_block); clear != 0 zeroes it afterwards
int mi355x_colpart_debug_rhs(mi355x_colpart *p, int shard, double *out, int64_t n, int clear)
{
    if (!p || !out || shard < 0 || shard >= (int)p->sh.size()) return fail(MI_BAD_ARG, "bad argument");
    HIP_TRY(hipSetDevice(p->sh[(size_t)shard].device));
    HIP_TRY(hipStreamSynchronize(p->sh[(size_t)shard].t->stream));
    return mi355x_debug_rhs(p->sh[(size_t)shard].t, out, n, clear) == 0 ? MI_OK : fail(MI_HIP_ERROR, "copy failed");
}

// test / measurement aid: clean two-launch blocks before a demoted handle tries the persistent block launch again
int mi355x_colpart_debug_set_la_rearm(mi355x_colpart *p, int64_t blocks)
{
    if (!p) return fail(MI_BAD_ARG, "handle is NULL");
    p->la_rearm_in = blocks;
    return MI_OK;
}

// out4: blocks enqueued through the persistent block launch (k_shard_la_block), exchanges it lost, whether the
// handle is demoted to the two-launch step right now, whether the next block would take the persistent form
int mi355x_colpart_la_stats(mi355x_colpart *p, int64_t *out4)
{
    if (!p || !out4) return fail(MI_BAD_ARG, "NULL argument");
    out4[0] = p->la_blocks; out4[1] = p->la_losses; out4[2] = p->la_lost ? 1 : 0; out4[3] = (p->j == 0 && cp_la_block_live(p)) ? 1 : 0;
    return MI_OK;
}

int mi355x_colpart_exchange_timing_enable(mi355x_colpart *p, int stride, int max_samples)
{
    if (!p || stride < 0 || max_samples < 0 || max_samples > 4096) return fail(MI_BAD_ARG, "bad exchange-timing arguments");
    p->timing_stride = stride;
    for (CpShard &s : p->sh) {
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipStreamSynchronize(s.t->stream));
        s.ev_used = 0;
        while (s.ev.size() < (size_t)max_samples * 4) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            s.ev.push_back(e);
        }
    }
    return MI_OK;
}

int mi355x_colpart_exchange_timing_read(mi355x_colpart *p, int64_t *n_samples, double *allgather_us, double *allreduce_us)
{
    if (!p) return fail(MI_BAD_ARG, "handle is NULL");
    int64_t n = 0;
    double ag = 0.0, ar = 0.0;
    for (CpShard &s : p->sh) {                       // averages over the local shards' samples
        HIP_TRY(hipSetDevice(s.device));
        HIP_TRY(hipStreamSynchronize(s.t->stream));
        for (int k = 0; k + 4 <= s.ev_used; k += 4) {
            float a = 0.f, b = 0.f;
            HIP_TRY(hipEventElapsedTime(&a, s.ev[(size_t)k], s.ev[(size_t)k + 1]));
            HIP_TRY(hipEventElapsedTime(&b, s.ev[(size_t)k + 2], s.ev[(size_t)k + 3]));
            ag += a * 1e3;
            ar += b * 1e3;
            ++n;
        }
        s.ev_used = 0;
    }
    if (n_samples) *n_samples = n;
    if (allgather_us) *allgather_us = n ? ag / n : 0.0;
    if (allreduce_us) *allreduce_us = n ? ar / n : 0.0;
    return MI_OK;
}

int mi355x_colpart_sync(mi355x_colpart *p, int64_t *n_pivots)
{
    if (!p) return fail(MI_BAD_ARG, "handle is NULL");
    return cp_status(p, n_pivots);
}

}  // extern "C"
namespace { int cp_make_dense(mi355x_colpart *art, bool unit_columns_stay); }
extern "C" {

int mi355x_colpart_solve(mi355x_colpart *p, int is_max, double f, int64_t max_pivots, int64_t *n_pivots)
{
    if (!p) return fail(MI_BAD_ARG, "handle is NULL");
    if (max_pivots < 0) return fail(MI_BAD_ARG, "max_pivots < 0");
    FlagCancelScope cancel_scope(p->cancel);
    p->is_max = is_max ? 1 : 0;
    int rc = cp_flush(p);
    if (rc != MI_OK) return rc;
    for (CpShard &s : p->sh)
        if ((rc = mi355x_tab_reset(s.t, max_pivots)) != MI_OK) return rc;
    // blind enqueue in chunks (an iteration after termination is a no-op on the device), one
    // status read-back per chunk -- the same decision on every shard / rank
    int64_t chunk = 64;
    for (;;) {
        // (whole blocks: the persistent block launch starts a new block with every launch)
        const int64_t bk = p->block > 1 ? p->block : 1;
        rc = cp_run(p, f, (chunk + bk - 1) / bk * bk);
        if (rc != MI_OK) return rc;
        const int st = cp_status(p, n_pivots);
        if (st == MI_NONFINITE && p->compact && !p->multi_process && (int)p->sh.size() == p->world) {
            // The entering column holds an inf / NaN (the pivot was NOT applied): the reference would turn the
            // basic columns into NaNs (x - inf * 0), which only a tableau that stores them can hold.  From here
            // on the tableau lives on DENSE shards -- every logical column distributed -- and the pivot is
            // redone there (round 6; until then the handle stopped with MI_NONFINITE and the host fell back to
            // one device).  What dense shards still cannot follow -- a NaN quotient in the ratio test, whose
            // outcome depends on the reference's scan order -- ends as MI_NONFINITE as before.
            if ((rc = cp_make_dense(p, /*unit_columns_stay=*/false)) != MI_OK) return rc;   // (the redone pivot writes NaNs into them)
            for (CpShard &s : p->sh) {
                HIP_TRY(hipSetDevice(s.device));
                launch_ctl_resume(s.t->v, s.t->stream, MI_NONFINITE);
                HIP_TRY(hipGetLastError());
            }
            continue;
        }
        if (st != MI_RUNNING) return st;
        // (cp_status has applied the pending pivots of an open block: the tableau is whole)
        if (p->cancel.exchange(0, std::memory_order_acq_rel)) return MI_CANCELLED;
        if (chunk < 256) chunk *= 2;
    }
}

/* 1: compact shards (non-basic columns only), 0: dense shards (every logical column distributed: the basis was not
 * a set of unit columns, or the solve met what compact shards cannot hold -- a non-finite entering column, a
 * drive-out pivot on a negative element, a non-finite objective coefficient on a basic column) */
int mi355x_colpart_is_compact(const mi355x_colpart *p) { return p ? (p->compact ? 1 : 0) : -1; }

int mi355x_colpart_cancel(mi355x_colpart *p)
{
    if (!p) return fail(MI_BAD_ARG, "handle is NULL");
    // one process per GPU: the ranks would have to take the decision at the same chunk, or the
    // collectives of the others never complete -- bound such solves with max_pivots instead
    if (p->multi_process)
        return fail(MI_UNSUPPORTED, "cancel is not available on a one-process-per-GPU handle: solve in max_pivots chunks");
    p->cancel.store(1, std::memory_order_release);
    return MI_OK;
}

}  // extern "C"

namespace {

// fn(shard) on every local shard: one after the other, except over RCCL with several shards in
// this process, where every shard's collectives must be issued from its own thread
template <class F> int cp_each_shard(mi355x_colpart *p, F fn)
{
    if (!p->rccl || p->sh.size() == 1) {
        for (CpShard &s : p->sh) {
            const int rc = fn(s);
            if (rc != MI_OK) return rc;
        }
        return MI_OK;
    }
    std::vector<int> rcs(p->sh.size(), MI_OK);
    std::vector<std::string> errs(p->sh.size());
    std::vector<std::thread> th;
    for (size_t i = 0; i < p->sh.size(); ++i)
        th.emplace_back([&, i]() { rcs[i] = fn(p->sh[i]); if (rcs[i] != MI_OK) errs[i] = g_err; });
    for (auto &x : th) x.join();
    for (size_t i = 0; i < p->sh.size(); ++i)
        if (rcs[i] != MI_OK) { cp_abort(p); g_err = errs[i]; return rcs[i]; }
    return MI_OK;
}

// n-pivot-row with a column AND row the caller chose (src/simplex.lisp:434), on every shard: the
// owner contributes the column, exchange B delivers it, every shard normalises its slice of the
// row and updates its slice (per-pivot kernels; no pending block may be open)
int cp_forced_pivot(mi355x_colpart *p, int64_t ec, int64_t cr)
{
    if (p->dead) return fail(MI_RCCL_ERROR, "this handle's communicators were aborted after an earlier failure");
    auto contribute = [&](CpShard &s) -> int {
        mi355x_tab *t = s.t;
        HIP_TRY(hipSetDevice(s.device));
        t->v.col_bias = t->v.p2l ? 0 : s.col_begin;
        launch_shard_forced_contribute(t->v, ec, s.col_begin, (int64_t *)s.bits, s.ec, t->stream);
        HIP_TRY(hipGetLastError());
        return MI_OK;
    };
    auto pivot = [&](CpShard &s) -> int {
        mi355x_tab *t = s.t;
        HIP_TRY(hipSetDevice(s.device));
        launch_shard_prepare(t->v, reinterpret_cast<const double *>(s.bits_in), s.ec, 1024.0, t->stream, cr);
        (void)launch_update(t->v, 1.0, 0, t->stream);
        t->n_part = 0;
        HIP_TRY(hipGetLastError());
        return MI_OK;
    };
    const unsigned epoch = ++p->xepoch;
    if (!p->rccl) {
        int rc;
        for (CpShard &s : p->sh) if ((rc = contribute(s)) != MI_OK) return rc;
        if (p->exchange == 2) {
            for (CpShard &s : p->sh) if ((rc = cp_p2p_column(p, s, epoch, true, false)) != MI_OK) return rc;
            for (CpShard &s : p->sh) if ((rc = cp_p2p_column(p, s, epoch, false, true)) != MI_OK) return rc;
        } else {
            int blocks = (int)((p->rows + 255) / 256);
            if (blocks > 256) blocks = 256;
            hipLaunchKernelGGL(k_local_sum, dim3(blocks), dim3(256), 0, p->sh[0].t->stream, p->l_bits_all, p->l_bits_sum,
                               p->rows, p->world);
        }
        for (CpShard &s : p->sh) if ((rc = pivot(s)) != MI_OK) return rc;
        return MI_OK;
    }
    return cp_each_shard(p, [&](CpShard &s) -> int {
        int rc = contribute(s);
        if (rc != MI_OK) return rc;
        if (p->exchange == 2) { if ((rc = cp_p2p_column(p, s, epoch, true, true)) != MI_OK) return rc; }
        else RCCL_TRY(rccl().AllReduce(s.bits, s.bits, (size_t)p->rows, ncclInt64, ncclSum, s.comm, s.t->stream));
        return pivot(s);
    });
}

}  // namespace

namespace {

// src/simplex.lisp:447 on the basic columns alone: the scale of step i is the objective entry of basis[i] AS
// REDUCED BY THE STEPS BEFORE IT.  o[k] = objective entry of basis[k]; B[i][k] = entry of row i in column
// basis[k] (B == nullptr: the basic columns are exact unit columns, B is the identity with +0 elsewhere).  One
// workgroup, a barrier per step -- m steps of m / 1024 operations per thread; only what CAN make a later scale
// differ from the original coefficient goes through here (an entry of B above the diagonal in a row whose scale is
// not zero; an inf / NaN scale times a zero), the objective row itself is then re-eliminated column-parallel with
// these scales (k_handover_objective_columns).
__global__ __launch_bounds__(1024) void k_handover_scales_seq(const double *B, int64_t m, double *o, double *scales)
{
    for (int64_t i = 0; i < m; ++i) {
        const double sc = o[i];
        __syncthreads();                                   // everyone has read the scale
        if (threadIdx.x == 0) scales[i] = sc;
        if (sc != 0.0)                                     // (/= 0 scale)                        simplex.lisp:448
            for (int64_t k = threadIdx.x; k < m; k += blockDim.x) {
                const double e = B ? B[i * m + k] : (k == i ? 1.0 : 0.0);
                const double prod = sc * e;
                o[k] = o[k] - prod;
            }
        __syncthreads();                                   // o updated before the next scale
    }
}

// the scales of the hand-over's re-elimination, as the sequential loop reads them: through k_handover_scales_seq on
// `device` with the basic block B_host (m x m, row-major).  B_host == nullptr is the caller's word that the basic
// columns are unit vectors with +-0 elsewhere AND every coefficient is finite: then every product scale * (+-0) is a
// zero, no later scale can change, and the scales are the original objective coefficients (host-side shortcut).
int cp_handover_scales(int device, hipStream_t st, int64_t m, const int64_t *basis, const double *main_obj,
                       const double *B_host, std::vector<double> &scales)
{
    scales.resize((size_t)std::max<int64_t>(m, 1));
    for (int64_t i = 0; i < m; ++i) scales[(size_t)i] = main_obj[basis[i]];
    if (!B_host || m < 1) return MI_OK;
    HIP_TRY(hipSetDevice(device));
    double *d_o = nullptr, *d_s = nullptr, *d_B = nullptr;
    hipError_t e = hipMalloc((void **)&d_o, m * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&d_s, m * sizeof(double));
    if (e == hipSuccess && B_host) e = hipMalloc((void **)&d_B, (size_t)m * m * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(d_o, scales.data(), m * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && B_host) e = hipMemcpyAsync(d_B, B_host, (size_t)m * m * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_handover_scales_seq, dim3(1), dim3(1024), 0, st, d_B, m, d_o, d_s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(scales.data(), d_s, m * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(d_o); (void)hipFree(d_s); (void)hipFree(d_B);
    if (e != hipSuccess) return fail(MI_HIP_ERROR, "hand-over scales failed: %s", hipGetErrorString(e));
    return MI_OK;
}

// Degenerate artificials still basic after phase 1: pivot them out (src/simplex.lisp:419-434), from row
// `first_row` on.  Compact shards cannot take a pivot on a NEGATIVE element (it turns the +0 entries the basic
// columns hold in the pivot row into -0.0, and they store no basic column): *stopped_at = that row, nothing
// done for it, MI_OK -- the caller moves the tableau to dense shards and calls again.
int cp_drive_out(mi355x_colpart *art, int64_t num_vars, std::vector<int64_t> &basis, int64_t first_row, int64_t *n1,
                 bool *reset_done, int64_t *stopped_at)
{
    const int64_t m = art->rows - 1;
    *stopped_at = -1;
    std::vector<double> rowbuf;
    std::vector<int64_t> gcols;
    std::vector<char> is_basic;
    int rc;
    for (int64_t i = first_row; i < m; ++i) {
        if (basis[(size_t)i] < num_vars) continue;
        // the RHS entry of row i (every shard holds the RHS column)
        {
            CpShard &s0 = art->sh[0];
            HIP_TRY(hipSetDevice(s0.device));
            double rhs_i = 0.0;
            HIP_TRY(hipMemcpyAsync(&rhs_i, s0.t->v.M + i * s0.t->v.ld + (s0.t->v.cols - 1), sizeof(double),
                                   hipMemcpyDeviceToHost, s0.t->stream));
            HIP_TRY(hipStreamSynchronize(s0.t->stream));
            if (rhs_i != 0.0) return MI_ART_NONZERO;
        }
        // first non-basic column of the main problem with a non-zero entry in row i (compact shards: only
        // stored columns can qualify; dense shards store the basic columns too: skipped explicitly, :427-429)
        if (!art->compact) {
            is_basic.assign((size_t)art->var_count, 0);
            for (int64_t k = 0; k < m; ++k)
                if (basis[(size_t)k] >= 0 && basis[(size_t)k] < art->var_count) is_basic[(size_t)basis[(size_t)k]] = 1;
        }
        int64_t new_col = -1;
        double new_val = 0.0;
        for (CpShard &s : art->sh) {
            const int64_t nloc = s.t->v.cols - 1;
            gcols.resize((size_t)nloc);
            rowbuf.resize((size_t)nloc);
            if (art->compact) { if ((rc = mi355x_shard_columns(s.t, gcols.data())) != MI_OK) return rc; }
            else for (int64_t k = 0; k < nloc; ++k) gcols[(size_t)k] = s.col_begin + k;
            HIP_TRY(hipSetDevice(s.device));
            HIP_TRY(hipMemcpyAsync(rowbuf.data(), s.t->v.M + i * s.t->v.ld, nloc * sizeof(double),
                                   hipMemcpyDeviceToHost, s.t->stream));
            HIP_TRY(hipStreamSynchronize(s.t->stream));
            for (int64_t k = 0; k < nloc; ++k) {
                const int64_t g = gcols[(size_t)k];
                if (g >= 0 && g < num_vars && rowbuf[(size_t)k] != 0.0 && (new_col < 0 || g < new_col) &&
                    (art->compact || !is_basic[(size_t)g])) {
                    new_col = g;
                    new_val = rowbuf[(size_t)k];
                }
            }
        }
        if (new_col < 0) return MI_ART_STUCK;
        if (new_val < 0.0 && art->compact) { *stopped_at = i; return MI_OK; }
        if (!*reset_done) {                                   // phase 1 left every shard's status at OPTIMAL
            for (CpShard &s : art->sh)
                if ((rc = mi355x_tab_reset(s.t, 0)) != MI_OK) return rc;
            *reset_done = true;
        }
        rc = cp_forced_pivot(art, new_col, i);
        if (rc != MI_OK) return rc;
        basis[(size_t)i] = new_col;
        ++*n1;
    }
    return MI_OK;
}

// what `p` holds -> `q` (the handle keeps its address: callers go on using it); q is emptied
void cp_take_over(mi355x_colpart *p, mi355x_colpart *q)
{
    std::swap(p->sh, q->sh);
    std::swap(p->l_gathered, q->l_gathered);
    std::swap(p->l_bits_all, q->l_bits_all);
    std::swap(p->l_bits_sum, q->l_bits_sum);
    p->compact = q->compact; p->block = q->block; p->j = q->j; p->lay = q->lay; p->xepoch = q->xepoch;
    p->p2p_connected = q->p2p_connected; p->la_epoch = q->la_epoch;   // (la_lost / la_rearm_in: the handle's own history stays)
    p->la_block_mode = q->la_block_mode; p->self_hop = q->self_hop; p->p2p_spins = q->p2p_spins;
}

// The artificial tableau on DENSE shards (every logical column distributed, basic ones included) in place of its
// compact shards: what a -0.0 in a basic column, or a NaN in the objective row of one, needs in order to exist.
// The tableau goes through the host once (data movement only: the assembly mi355x_colpart_download does anyway).
int cp_make_dense(mi355x_colpart *art, bool unit_columns_stay)
{
    const int64_t rows = art->rows, cols = art->var_count + 1, m = rows - 1;
    std::vector<double> hm((size_t)rows * cols);
    std::vector<int64_t> hb((size_t)std::max<int64_t>(m, 1));
    int rc = mi355x_colpart_download(art, hm.data(), hb.data(), nullptr, nullptr);
    if (rc != MI_OK) return rc;
    std::vector<int> devs;
    for (CpShard &s : art->sh) devs.push_back(s.device);
    mi355x_colpart *ad = nullptr;
    rc = cp_create_from_host(&ad, rows, cols, hm.data(), hb.data(), art->world, art->rccl ? devs.data() : &devs[0],
                             /*force_dense=*/true, /*make_comms=*/false, art->exchange, art->rccl ? 1 : 0);
    if (rc != MI_OK) return rc;
    if (ad->world != art->world) { cp_free(ad); return fail(MI_UNSUPPORTED, "dense shards: fewer columns than shards"); }
    // the pivot count and the trace go on where the compact shards stopped
    auto carry_over = [&]() -> int {
        for (size_t i = 0; i < art->sh.size(); ++i) {
            mi355x_tab *from = art->sh[i].t, *to = ad->sh[i].t;
            HIP_TRY(hipSetDevice(ad->sh[i].device));
            HIP_TRY(hipStreamSynchronize(from->stream));
            HIP_TRY(hipMemcpyAsync(to->v.ctl, from->v.ctl, sizeof(Ctl), hipMemcpyDeviceToDevice, to->stream));
            Ctl c;
            HIP_TRY(hipMemcpyAsync(&c, from->v.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, to->stream));
            HIP_TRY(hipStreamSynchronize(to->stream));
            const int64_t tn = std::min<int64_t>(c.trace_n, kTraceCap);
            if (tn > 0 && from->v.trace_ec && to->v.trace_ec) {
                HIP_TRY(hipMemcpyAsync(to->v.trace_ec, from->v.trace_ec, tn * sizeof(int64_t), hipMemcpyDeviceToDevice, to->stream));
                HIP_TRY(hipMemcpyAsync(to->v.trace_cr, from->v.trace_cr, tn * sizeof(int64_t), hipMemcpyDeviceToDevice, to->stream));
                HIP_TRY(hipStreamSynchronize(to->stream));
            }
        }
        return MI_OK;
    };
    if ((rc = carry_over()) != MI_OK) { cp_free(ad); return rc; }   // (the compact shards and their communicators are untouched)
    for (size_t i = 0; i < art->sh.size(); ++i) { ad->sh[i].comm = art->sh[i].comm; art->sh[i].comm = nullptr; }
    cp_take_over(art, ad);
    cp_free(ad);                                              // (now holds the compact shards)
    art->unit_dense = unit_columns_stay;
    return MI_OK;
}

// Hand-over from DENSE artificial shards (src/simplex.lisp:437-451): the main tableau's rows are the artificial
// tableau's (columns of the main problem + RHS), its objective row the main problem's own re-eliminated over the
// basic rows with the scales the sequential loop would read.  Staged through the host (data movement: rows
// copied, columns redistributed over the shards); the re-elimination runs on the devices, column-parallel.
int cp_dense_handover(mi355x_colpart *art, int64_t main_cols, const double *main_obj, const std::vector<int64_t> &basis,
                      mi355x_colpart **main_out)
{
    const int64_t rows = art->rows, m = rows - 1, acols = art->var_count + 1, num_vars = main_cols - 1;
    std::vector<double> ha((size_t)rows * acols);
    int rc = mi355x_colpart_download(art, ha.data(), nullptr, nullptr, nullptr);
    if (rc != MI_OK) return rc;
    std::vector<double> hm((size_t)rows * main_cols);
    for (int64_t r = 0; r < m; ++r) {                          // :437-441
        std::copy(ha.begin() + r * acols, ha.begin() + r * acols + num_vars, hm.begin() + r * main_cols);
        hm[(size_t)(r * main_cols + num_vars)] = ha[(size_t)(r * acols + art->var_count)];
    }
    std::copy(main_obj, main_obj + main_cols, hm.begin() + m * main_cols);
    // The basic block (row i, column basis[k]) for the scales.  A tableau that was dense when the handle was created
    // may hold anything there: an entry above the diagonal changes a later scale (:447), so the sequential loop runs
    // on B.  Only shards that cp_make_dense filled from compact ones (unit columns, +-0 elsewhere: drive-out pivots
    // keep that) may take the original coefficients -- and only while all of them are finite.
    std::vector<double> B, scales;
    bool finite = true;
    for (int64_t i = 0; i < m; ++i) finite = finite && std::fabs(main_obj[basis[(size_t)i]]) <= 1.7976931348623157e308;
    const bool shortcut = art->unit_dense && finite;
    if (!shortcut) {
        B.resize((size_t)m * m);
        for (int64_t i = 0; i < m; ++i)
            for (int64_t k = 0; k < m; ++k) B[(size_t)(i * m + k)] = hm[(size_t)(i * main_cols + basis[(size_t)k])];
    }
    rc = cp_handover_scales(art->sh[0].device, art->sh[0].t->stream, m, basis.data(), main_obj, shortcut ? nullptr : B.data(), scales);
    if (rc != MI_OK) return rc;
    std::vector<int> devs;
    for (CpShard &s : art->sh) devs.push_back(s.device);
    mi355x_colpart *mp = nullptr;
    rc = cp_create_from_host(&mp, rows, main_cols, hm.data(), basis.data(), art->world, art->rccl ? devs.data() : &devs[0],
                             /*force_dense=*/true, /*make_comms=*/false, art->exchange, art->rccl ? 1 : 0);
    if (rc != MI_OK) return rc;
    if (art->rccl && mp->world != art->world) { cp_free(mp); return fail(MI_UNSUPPORTED, "dense main shards: fewer columns than communicators"); }
    for (CpShard &s : mp->sh) {                               // :444-451, every shard on its own columns (and its RHS copy)
        mi355x_tab *t = s.t;
        hipError_t e = hipSetDevice(s.device);
        if (e == hipSuccess && m > 0) e = hipMemcpyAsync(t->v.col, scales.data(), m * sizeof(double), hipMemcpyHostToDevice, t->stream);
        if (e == hipSuccess) {
            launch_handover_objective_columns(t->v, t->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
        if (e != hipSuccess) { cp_free(mp); return fail(MI_HIP_ERROR, "dense hand-over failed: %s", hipGetErrorString(e)); }
        t->n_part = 0;
    }
    *main_out = mp;
    return MI_OK;
}

}  // namespace

extern "C" {

int mi355x_colpart_solve_two_phase(mi355x_colpart *art, int64_t main_cols, const double *main_obj,
                                   int main_is_max, double f, int64_t *n_pivots, mi355x_colpart **main_out)
{
    if (main_out) *main_out = nullptr;
    if (n_pivots) { n_pivots[0] = 0; n_pivots[1] = 0; }
    if (!art || !main_obj || !main_out) return fail(MI_BAD_ARG, "NULL argument");
    const int64_t rows = art->rows, m = rows - 1, num_art_vars = art->var_count, num_vars = main_cols - 1;
    if (num_vars < 1 || num_vars > num_art_vars)
        return fail(MI_BAD_ARG, "main tableau has %lld columns, the artificial one %lld", (long long)main_cols,
                    (long long)(num_art_vars + 1));
    if (art->multi_process || (int)art->sh.size() != art->world)
        return fail(MI_UNSUPPORTED, "the two-phase hand-over needs every shard in this process");
    int64_t n1 = 0, n2 = 0;
    int rc = mi355x_colpart_solve(art, /*is_max=*/0, f, 0, &n1);                  // simplex.lisp:403
    if (n_pivots) n_pivots[0] = n1;
    if (rc != MI_OPTIMAL) return rc;
    std::vector<int64_t> basis((size_t)std::max<int64_t>(m, 1));
    std::vector<double> last_col((size_t)rows);
    rc = mi355x_colpart_download(art, nullptr, basis.data(), nullptr, last_col.data());
    if (rc != MI_OK) return rc;
    // (a caller's basis may hold anything; from here on main_obj, the rows and is_basic are indexed with it)
    for (int64_t i = 0; i < m; ++i)
        if (basis[(size_t)i] < 0 || basis[(size_t)i] >= num_art_vars)
            return fail(MI_BAD_ARG, "basis entry %lld of row %lld is outside [0, %lld)", (long long)basis[(size_t)i],
                        (long long)i, (long long)num_art_vars);
    // (fp= 0 objective factor)                                                    simplex.lisp:405-407
    const double diff = 0.0 - last_col[(size_t)m];
    if (!((diff < 0.0 ? -diff : diff) <= f * kClEpsilon)) return MI_INFEASIBLE;
    // degenerate artificials still basic: pivot them out                        simplex.lisp:419-434
    // A NEGATIVE pivot element turns the +0 entries the basic columns hold in the pivot row into -0.0 (+0 /
    // negative; the ratio test only ever picks positive elements, a drive-out pivot takes whatever is there),
    // and compact shards store no basic column: from that pivot on the tableau lives on DENSE shards -- every
    // logical column distributed, phase 2 included (round 6; until then such a problem was declined).
    bool reset_done = false;
    int64_t stopped = -1;
    rc = cp_drive_out(art, num_vars, basis, 0, &n1, &reset_done, &stopped);
    if (rc != MI_OK) return rc;
    if (stopped >= 0) {
        if (reset_done) {                                     // the drive-out pivots so far: any trouble among them?
            int64_t np = 0;
            const int st = cp_status(art, &np);
            if (st != MI_RUNNING) return st < 0 ? st : (st == MI_NONFINITE ? MI_NONFINITE : fail(MI_HIP_ERROR, "drive-out pivot failed (status %d)", st));
        }
        if ((rc = cp_make_dense(art, /*unit_columns_stay=*/true)) != MI_OK) return rc;
        reset_done = false;                                   // (the dense shards' first pivot sets them running)
        rc = cp_drive_out(art, num_vars, basis, stopped, &n1, &reset_done, &stopped);
        if (rc != MI_OK) return rc;
    }
    if (n_pivots) n_pivots[0] = n1;
    if (reset_done) {                                         // a non-finite column in a drive-out pivot
        int64_t np = 0;
        const int st = cp_status(art, &np);
        if (st != MI_RUNNING) return st < 0 ? st : (st == MI_NONFINITE ? MI_NONFINITE : fail(MI_HIP_ERROR, "drive-out pivot failed (status %d)", st));
    }
    // ---- hand-over (simplex.lisp:437-451)
    // The re-elimination reads every scale from the objective row AS REDUCED SO FAR (:447).  While every scale is
    // finite that is the original coefficient (earlier steps subtract scale * (+-0) from it, and a zero of either
    // sign is skipped by the (/= 0 scale) test); an inf / NaN coefficient on a basic column turns the objective
    // entries of the OTHER basic columns into NaNs (inf * 0), which only a tableau that stores its basic
    // columns can hold: dense shards again (round 6), with the scales from the sequential loop on the basic block.
    // That argument needs unit basic columns: a tableau that was dense at creation always takes the sequential loop
    // (cp_dense_handover).
    bool finite = true;
    for (int64_t i = 0; i < m; ++i) finite = finite && std::fabs(main_obj[basis[(size_t)i]]) <= 1.7976931348623157e308;
    if (!finite && art->compact && (rc = cp_make_dense(art, /*unit_columns_stay=*/true)) != MI_OK) return rc;
    mi355x_colpart *mp = nullptr;
    if (!art->compact) {
        rc = cp_dense_handover(art, main_cols, main_obj, basis, &mp);
        if (rc != MI_OK) return rc;
    } else {
    // compact shards: the main tableau's shards are the artificial shards' main-problem columns, gathered slot by
    // slot on each device; the objective row is the main tableau's own, re-eliminated over the basic rows
    mp = new (std::nothrow) mi355x_colpart;
    if (!mp) return fail(MI_NO_MEMORY, "host allocation failed");
    mp->world = art->world;
    mp->rccl = art->rccl;
    mp->compact = true;
    mp->rows = rows;
    mp->var_count = num_vars;
    mp->exchange = art->exchange;
    mp->xepoch = 0;                                           // (its own buffers, zeroed: tags start over)
    std::vector<double> scales((size_t)std::max<int64_t>(m, 1));
    for (int64_t i = 0; i < m; ++i) scales[(size_t)i] = main_obj[basis[(size_t)i]];
    std::vector<int64_t> keep, newcols, gcols;
    std::vector<double> obj0;
    for (CpShard &as : art->sh) {
        const int64_t nloc = as.t->v.cols - 1;
        gcols.resize((size_t)nloc);
        rc = mi355x_shard_columns(as.t, gcols.data());
        if (rc != MI_OK) { cp_free(mp); return rc; }
        keep.clear(); newcols.clear(); obj0.clear();
        for (int64_t k = 0; k < nloc; ++k)
            if (gcols[(size_t)k] >= 0 && gcols[(size_t)k] < num_vars) {
                keep.push_back(k); newcols.push_back(gcols[(size_t)k]); obj0.push_back(main_obj[gcols[(size_t)k]]);
            }
        if (keep.empty()) {                                   // nothing but artificial columns here: keep ONE slot as a
            keep.push_back(0); newcols.push_back(-1); obj0.push_back(0.0);   // dead slot (a shard stores a column)
        }
        obj0.push_back(main_obj[num_vars]);
        const int64_t nk = (int64_t)keep.size();
        CpShard ns;
        ns.index = as.index;
        ns.device = as.device;
        ns.col_begin = 0; ns.col_end = nk;
        rc = alloc_tab(&ns.t, rows, nk + 1, ns.device);
        mp->sh.push_back(ns);
        if (rc != MI_OK) { cp_free(mp); return rc; }
        mi355x_tab *nt = mp->sh.back().t;
        int64_t *d_keep = nullptr;
        double *d_obj0 = nullptr, *d_scales = nullptr;
        hipError_t e = hipMalloc((void **)&d_keep, nk * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&d_obj0, (nk + 1) * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&d_scales, std::max<int64_t>(m, 1) * sizeof(double));
        hipStream_t st = as.t->stream;                        // behind everything phase 1 enqueued on this shard
        if (e == hipSuccess) e = hipMemcpyAsync(d_keep, keep.data(), nk * sizeof(int64_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_obj0, obj0.data(), (nk + 1) * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && m > 0) e = hipMemcpyAsync(d_scales, scales.data(), m * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(nt->stream);          // alloc_tab's memsets
        if (e == hipSuccess) e = hipMemsetAsync(nt->v.M, 0, (size_t)rows * nt->v.ld * sizeof(double), st);   // padding columns
        if (e == hipSuccess) {
            launch_shard_handover(as.t->v, nt->v, d_keep, d_obj0, d_scales, st);
            launch_ctl_reset(nt->v, 0, 1, st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(d_keep); (void)hipFree(d_obj0); (void)hipFree(d_scales);
        if (e != hipSuccess) { cp_free(mp); return fail(MI_HIP_ERROR, "hand-over failed: %s", hipGetErrorString(e)); }
        rc = mi355x_shard_set_compact(nt, num_vars, newcols.data());
        if (rc != MI_OK) { cp_free(mp); return rc; }
    }
    rc = cp_finish_setup(mp, nullptr, -1, /*make_comms=*/false);
    if (rc != MI_OK) { cp_free(mp); return rc; }
    }
    // the communicators move to the main tableau: the artificial one can still be read, not solved
    for (size_t i = 0; i < art->sh.size() && i < mp->sh.size(); ++i) { mp->sh[i].comm = art->sh[i].comm; art->sh[i].comm = nullptr; }
    art->dead = art->rccl;
    *main_out = mp;
    rc = mi355x_colpart_solve(mp, main_is_max, f, 0, &n2);                       // simplex.lisp:452
    if (n_pivots) n_pivots[1] = n2;
    return rc;
}

int mi355x_colpart_trace(mi355x_colpart *p, int64_t *ecs, int64_t *crs, int64_t cap, int64_t *n)
{
    if (!p) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = cp_flush(p);
    if (rc != MI_OK) return rc;
    return mi355x_tab_trace(p->sh[0].t, ecs, crs, cap, n);
}

int mi355x_colpart_download(mi355x_colpart *p, double *hm, int64_t *hb, double *last_row, double *last_col)
{
    if (!p) return fail(MI_BAD_ARG, "handle is NULL");
    int rc = cp_flush(p);
    if (rc != MI_OK) return rc;
    const int64_t rows = p->rows, vc = p->var_count, cols = vc + 1, m = rows - 1;
    const bool whole = (int)p->sh.size() == p->world;
    if ((hm || last_row) && !whole)
        return fail(MI_UNSUPPORTED, "the logical tableau / objective row need every shard in this process");
    std::vector<int64_t> basis((size_t)std::max<int64_t>(m, 1));
    std::vector<double> loc;
    std::vector<int64_t> gcols;
    if (hm) std::fill(hm, hm + rows * cols, 0.0);
    if (last_row) std::fill(last_row, last_row + cols, 0.0);
    for (size_t si = 0; si < p->sh.size(); ++si) {
        CpShard &s = p->sh[si];
        const int64_t nloc = s.t->v.cols - 1;
        const bool first = si == 0;
        if (hm || last_row) {
            gcols.resize((size_t)nloc);
            if (p->compact) { if ((rc = mi355x_shard_columns(s.t, gcols.data())) != MI_OK) return rc; }
            else for (int64_t k = 0; k < nloc; ++k) gcols[(size_t)k] = s.col_begin + k;
        }
        if (hm) {
            loc.resize((size_t)(rows * (nloc + 1)));
            rc = mi355x_tab_download(s.t, loc.data(), first ? basis.data() : nullptr, nullptr, nullptr);
            if (rc != MI_OK) return rc;
            for (int64_t r = 0; r < rows; ++r) {
                for (int64_t k = 0; k < nloc; ++k)
                    if (gcols[(size_t)k] >= 0) hm[r * cols + gcols[(size_t)k]] = loc[(size_t)(r * (nloc + 1) + k)];   // (< 0: a dead slot)
                if (first) hm[r * cols + vc] = loc[(size_t)(r * (nloc + 1) + nloc)];
            }
            if (last_row) for (int64_t k = 0; k < nloc; ++k)
                if (gcols[(size_t)k] >= 0) last_row[gcols[(size_t)k]] = loc[(size_t)(m * (nloc + 1) + k)];
            if (last_row && first) last_row[vc] = loc[(size_t)(m * (nloc + 1) + nloc)];
        } else if (last_row) {
            loc.resize((size_t)(nloc + 1));
            rc = mi355x_tab_download(s.t, nullptr, first ? basis.data() : nullptr, loc.data(), nullptr);
            if (rc != MI_OK) return rc;
            for (int64_t k = 0; k < nloc; ++k)
                if (gcols[(size_t)k] >= 0) last_row[gcols[(size_t)k]] = loc[(size_t)k];
            if (first) last_row[vc] = loc[(size_t)nloc];
        } else if (first && (hb || last_col)) {
            rc = mi355x_tab_download(s.t, nullptr, basis.data(), nullptr, nullptr);
            if (rc != MI_OK) return rc;
        }
    }
    if (hm && p->compact)                                        // basic columns are stored nowhere: unit vectors
        for (int64_t i = 0; i < m; ++i) hm[i * cols + basis[(size_t)i]] = 1.0;
    if (hb) std::copy(basis.begin(), basis.begin() + m, hb);
    if (last_col) {
        rc = mi355x_tab_download(p->sh[0].t, nullptr, nullptr, nullptr, last_col);   // every shard holds the RHS column
        if (rc != MI_OK) return rc;
    }
    return MI_OK;
}

void mi355x_colpart_destroy(mi355x_colpart *p) { cp_free(p); }

}  // extern "C"
