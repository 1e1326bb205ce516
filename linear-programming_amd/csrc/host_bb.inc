// host_bb.inc -- branch-and-bound (src/simplex.lisp:462-542) as a resumable job: part of the
// host_problem.cpp translation unit (it uses build(), the problem and the solution structs).
//
// The search is the reference's, node for node: a depth-first walk over an explicit stack of
// entries (lists of extra rows, newest first), each entry popped, built with
// constraints = entry ++ problem-constraints and solved, the first integer variable of the
// caller's order whose value is not integral branched on, `<=` child on top.  What differs is only
// WHEN a node's LP is solved: ahead of time, up to `width` nodes in one mi355x_simplex_solver_many
// job (same-shape node LPs become one multi-device batch).  That is exact because
//   - every entry the reference pushes is eventually popped and solved (it never drops entries),
//   - a node's LP result -- and so which children it would create -- depends only on its own rows,
//   - pruning is monotone: the incumbent only improves, a node prunable now stays prunable,
// so the replay below sees the same results in the same order for every width.
#include <atomic>
#include <cmath>
#include <limits>

namespace {

struct BBNode {
    int64_t parent = -1;                      // node id of the parent (-1: the root)
    int64_t var = -1;                         // the branching row that made this node: var <= / >= bound
    int     sense = 0;                        // 0 `<=`, 1 `>=`
    double  bound = 0.0;
    int     depth = 0;
    bool    solved = false;
    int     status = MI_RUNNING;              // the node LP's outcome
    double  obj = 0.0;
    int64_t viol = -1;                        // first non-integral integer variable (caller's order), -1 none
    double  viol_val = 0.0;
    int64_t child[2] = {-1, -1};              // `<=` and `>=` children, made when first needed
    int64_t trace_index = -1;                 // position among the processed nodes
    std::unique_ptr<mi355x_solution> sol;     // kept while the node could still become the incumbent
};

}  // namespace

struct mi355x_bb {
    mi355x_problem base;
    std::vector<int64_t> int_order;
    double f = 1024.0, int_f = 0.0;
    int64_t width = 1;
    int n_devices = 1;
    std::vector<int> device_ids;              // empty: 0 .. n_devices-1
    std::vector<BBNode> nodes;
    std::vector<int64_t> stack;               // node ids, back() = top
    int64_t incumbent = -1;                   // node id
    bool done = false;
    int status = MI_RUNNING;
    std::atomic<int> cancel{0};
    int64_t n_solved = 0, max_depth = 0;
    struct TraceRow { int64_t parent, var; int32_t sense; double bound; int32_t outcome; double obj; };
    std::vector<TraceRow> trace;
    // device assembly: the base problem's general-form tableau on the devices (made at the first round)
    mi355x_bb_base *dbase = nullptr;
    std::vector<Mapping> gmap;                // var-mapping of every node (bounds only decide it)
    int64_t base_art = 0;                     // artificial rows of the base general form
    int64_t grows = 0, gcols = 0;             // its shape
    // the round in flight (kept across step calls: each call advances it by a bounded number of pivots)
    mi355x_solve_many *round = nullptr;
    std::vector<int64_t> round_ids;
    ~mi355x_bb()
    {
        mi355x_simplex_solver_many_abandon(round);
        mi355x_bb_base_destroy_(dbase);
    }
};

namespace {

// the reference's comparator (:515): `<` for max, `>` for min
bool bb_better(const mi355x_bb &j, double incumbent, double value)
{
    return j.base.is_max ? (incumbent < value) : (incumbent > value);
}

// integerp of the f64 reading (see the header): exact unless int_f > 0, then fp= v (round v) int_f
bool bb_integral(const mi355x_bb &j, double v)
{
    if (j.int_f > 0.0) {
        const double d = v - std::nearbyint(v);
        return (d < 0.0 ? -d : d) <= j.int_f * mi355x_epsilon();
    }
    return v == std::floor(v);
}

bool bb_prunable(const mi355x_bb &j, const BBNode &n)
{
    return n.viol >= 0 && j.incumbent >= 0 && !bb_better(j, j.nodes[(size_t)j.incumbent].obj, n.obj);
}

int64_t bb_child(mi355x_bb &j, int64_t id, int which)
{
    if (j.nodes[(size_t)id].child[which] >= 0) return j.nodes[(size_t)id].child[which];
    const BBNode &p = j.nodes[(size_t)id];
    BBNode c;                                                              // gen-entries, :465-472
    c.parent = id; c.var = p.viol; c.sense = which;
    c.bound = which == 0 ? std::floor(p.viol_val) : std::ceil(p.viol_val);
    c.depth = p.depth + 1;
    j.nodes.push_back(std::move(c));
    const int64_t cid = (int64_t)j.nodes.size() - 1;
    j.nodes[(size_t)id].child[which] = cid;
    return cid;
}

// the node's problem: constraints = entry (newest row first) ++ problem-constraints (:489-500)
void bb_node_problem(const mi355x_bb &j, int64_t id, mi355x_problem &out)
{
    out.is_max = j.base.is_max; out.n_vars = j.base.n_vars;
    out.obj_var = j.base.obj_var; out.obj_coef = j.base.obj_coef;
    out.bounds = j.base.bounds;
    out.is_integer.assign((size_t)j.base.n_vars, 0);                      // a node is an LP
    out.constraints.clear();
    for (int64_t k = id; j.nodes[(size_t)k].parent >= 0; k = j.nodes[(size_t)k].parent) {
        const BBNode &n = j.nodes[(size_t)k];
        Constraint c;
        c.op = n.sense; c.var = {n.var}; c.coef = {1.0}; c.rhs = n.bound;
        out.constraints.push_back(std::move(c));
    }
    out.constraints.insert(out.constraints.end(), j.base.constraints.begin(), j.base.constraints.end());
}

// the speculation policy (cost only, never results): a depth-first walk from the top of the stack,
// into the children of solved, non-integral, not yet prunable nodes, `<=` child first
void bb_collect(mi355x_bb &j, int64_t id, std::vector<int64_t> &out)
{
    if ((int64_t)out.size() >= j.width) return;
    if (!j.nodes[(size_t)id].solved) { out.push_back(id); return; }
    const BBNode &n = j.nodes[(size_t)id];
    if (n.status != MI_OPTIMAL || n.viol < 0 || bb_prunable(j, n)) return;
    const int64_t le = bb_child(j, id, 0);
    bb_collect(j, le, out);
    const int64_t ge = bb_child(j, id, 1);
    bb_collect(j, ge, out);
}

// the base problem's general form on the devices, once: what launch_node_assemble turns into node tableaux
int bb_prepare_base(mi355x_bb &j)
{
    if (j.dbase) return MI_OK;
    const Built g = build(j.base, /*general=*/true);
    const HostTableau &t = g.main_tab;
    const int64_t nv = j.base.n_vars;
    std::vector<int32_t> kind((size_t)nv);
    std::vector<int64_t> col((size_t)nv);
    std::vector<double> off((size_t)nv);
    for (int64_t v = 0; v < nv; ++v) { kind[v] = g.map[v].kind; col[v] = g.map[v].col; off[v] = g.map[v].offset; }
    j.gmap = g.map;
    j.grows = t.rows; j.gcols = t.cols;
    j.base_art = 0;
    for (int64_t bb : t.basis) j.base_art += bb == t.cols ? 1 : 0;
    return mi355x_bb_base_create_(&j.dbase, t.rows, t.cols, t.M.data(), g.flip.data(), t.basis.data(), g.ncv, g.nb, nv,
                                  kind.data(), col.data(), off.data());
}

// does node row (var, sense, bound) end up artificial?  (the sign test of k_bb_rows, same arithmetic)
bool bb_row_artificial(const mi355x_bb &j, int64_t var, int sense, double bound)
{
    const Mapping &mp = j.gmap[(size_t)var];
    double rhs = bound;
    if (mp.kind != kSigned) rhs = rhs - 1.0 * mp.offset;
    return mi355x::row_word_artificial(mi355x::row_word(rhs < 0.0, sense));
}

// start a speculation round: the collected nodes' LPs as ONE mi355x_simplex_solver_many job whose
// units are built here -- the root (depth 0: the problem itself, the no-constraint special case
// included) as an ordinary solver job, every other node in a batch of its shape (depth, artificial
// rows) assembled on the devices by launch_node_assemble
int bb_round_begin(mi355x_bb &j)
{
    std::vector<int64_t> ids;
    for (size_t s = j.stack.size(); s-- > 0 && (int64_t)ids.size() < j.width;)
        bb_collect(j, j.stack[s], ids);
    int rc = bb_prepare_base(j);
    if (rc != MI_OK) return rc;
    const size_t n = ids.size();
    std::unique_ptr<mi355x_solve_many> job(new (std::nothrow) mi355x_solve_many);
    if (!job) return hfail(MI_NO_MEMORY, "host allocation failed");
    job->n = (int64_t)n; job->f = j.f;
    job->status.assign(n, MI_RUNNING);
    job->sol.resize(n);
    std::map<std::pair<int64_t, int64_t>, std::vector<size_t>> groups;    // (depth, artificial rows) -> members
    for (size_t q = 0; q < n; ++q) {
        const BBNode &nd = j.nodes[(size_t)ids[q]];
        if (nd.depth == 0) {
            ManyUnit u;
            u.members.push_back((int64_t)q);
            mi355x_problem root;
            bb_node_problem(j, ids[q], root);                               // the problem, as an LP
            rc = mi355x_simplex_solver_begin(&root, j.f, j.device_ids.empty() ? 0 : j.device_ids[0], &u.single);
            if (rc == MI_UNBOUNDED) { job->status[q] = MI_UNBOUNDED; u.phase = 3; }   // :170, :174
            else if (rc != MI_OK) return rc;
            job->units.push_back(std::move(u));
            continue;
        }
        int64_t art = j.base_art;
        for (int64_t k = ids[q]; j.nodes[(size_t)k].parent >= 0; k = j.nodes[(size_t)k].parent)
            art += bb_row_artificial(j, j.nodes[(size_t)k].var, j.nodes[(size_t)k].sense, j.nodes[(size_t)k].bound);
        groups[{nd.depth, art}].push_back(q);
    }
    for (auto &g : groups) {
        const int64_t d = g.first.first, n_art = g.first.second, gn = (int64_t)g.second.size();
        std::vector<int64_t> var((size_t)(gn * d));
        std::vector<int32_t> sense((size_t)(gn * d));
        std::vector<double> bound((size_t)(gn * d));
        for (int64_t i = 0; i < gn; ++i) {
            int64_t k = ids[g.second[(size_t)i]];
            for (int64_t r = 0; r < d; ++r, k = j.nodes[(size_t)k].parent) {    // newest row first
                const BBNode &nk = j.nodes[(size_t)k];
                var[(size_t)(i * d + r)] = nk.var; sense[(size_t)(i * d + r)] = nk.sense; bound[(size_t)(i * d + r)] = nk.bound;
            }
        }
        ManyUnit u;
        u.is_max = j.base.is_max ? 1 : 0;
        for (size_t q : g.second) u.members.push_back((int64_t)q);
        rc = mi355x_bb_assemble_(j.dbase, gn, d, var.data(), sense.data(), bound.data(), n_art, j.n_devices,
                                 j.device_ids.empty() ? nullptr : j.device_ids.data(), &u.main_mb, &u.art_mb);
        if (rc != MI_OK) return rc;
        u.phase = n_art ? 1 : 2;
        u.st1.assign((size_t)gn, MI_RUNNING); u.between.assign((size_t)gn, MI_OK);
        u.np1.assign((size_t)gn, 0); u.np2.assign((size_t)gn, 0);
        job->units.push_back(std::move(u));                                 // (the job owns the batches now)
        const int64_t rows = j.grows + d, cols = j.gcols + d;
        for (size_t q : g.second) {
            std::unique_ptr<mi355x_solution> sl(new (std::nothrow) mi355x_solution);
            if (!sl) return hfail(MI_NO_MEMORY, "host allocation failed");
            sl->rows = rows; sl->cols = cols; sl->map = j.gmap;
            sl->last_row.resize((size_t)cols); sl->last_col.resize((size_t)rows);
            sl->basis.resize((size_t)(rows - 1));
            job->sol[q] = std::move(sl);
        }
    }
    j.round = job.release();
    j.round_ids = ids;
    return MI_OK;
}

// advance the round in flight by at most kRoundChunks x 4096 pivots per node LP and phase; MI_OK when
// every node of it has its result, MI_MAX_PIVOTS when the call's budget is used up, MI_CANCELLED
constexpr int kRoundChunks = 16;
int bb_round_advance(mi355x_bb &j)
{
    const size_t n = j.round_ids.size();
    std::vector<int32_t> st(n);
    int rc = MI_MAX_PIVOTS;
    for (int c = 0; c < kRoundChunks && rc == MI_MAX_PIVOTS; ++c) {
        if (j.cancel.exchange(0)) return MI_CANCELLED;       // (the round stays, a later step carries on)
        rc = mi355x_simplex_solver_many_step(j.round, 4096, st.data());
    }
    if (rc == MI_MAX_PIVOTS) return MI_MAX_PIVOTS;
    mi355x_solve_many *job = j.round;
    j.round = nullptr;
    if (rc != MI_OK) { mi355x_simplex_solver_many_abandon(job); return rc; }
    std::vector<mi355x_solution *> sols(n, nullptr);
    rc = mi355x_simplex_solver_many_finish(job, st.data(), sols.data());
    std::vector<std::unique_ptr<mi355x_solution>> owned(n);
    for (size_t q = 0; q < n; ++q) owned[q].reset(sols[q]);
    if (rc != MI_OK) return rc;
    for (size_t q = 0; q < n; ++q) {
        if (st[q] < 0) return st[q];           // a device error in this node's group
        BBNode &nd = j.nodes[(size_t)j.round_ids[q]];
        nd.solved = true; nd.status = st[q];
        ++j.n_solved;
        if (st[q] != MI_OPTIMAL) continue;
        mi355x_solution_objective_value(owned[q].get(), &nd.obj);
        for (int64_t v : j.int_order) {        // violated-integer-constraint, :474-479
            double x = 0.0;
            mi355x_solution_variable(owned[q].get(), v, &x);
            if (!bb_integral(j, x)) { nd.viol = v; nd.viol_val = x; break; }
        }
        if (nd.viol < 0) nd.sol = std::move(owned[q]);   // a candidate incumbent
    }
    return MI_OK;
}

}  // namespace

extern "C" {

int mi355x_simplex_solver_bb_begin(const mi355x_problem *p, const int64_t *int_order, int64_t n_int,
                                   double fp_tolerance, double int_tolerance, int64_t width, int n_devices,
                                   const int *device_ids, mi355x_bb **out)
{
    if (!out) return hfail(MI_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (!p) return hfail(MI_BAD_ARG, "problem is NULL");
    if (n_int < 0 || (n_int > 0 && !int_order)) return hfail(MI_BAD_ARG, "bad integer-variable order");
    for (int64_t k = 0; k < n_int; ++k)
        if (int_order[k] < 0 || int_order[k] >= p->n_vars) return hfail(MI_BAD_ARG, "integer variable index out of range");
    if (!(fp_tolerance >= 0.0) || !(int_tolerance >= 0.0) || std::isinf(int_tolerance))
        return hfail(MI_BAD_ARG, "tolerances must be finite and >= 0");
    if (width < 1 || n_devices < 1) return hfail(MI_BAD_ARG, "width and n_devices must be >= 1");
    if (device_ids)
        for (int d = 0; d < n_devices; ++d) if (device_ids[d] < 0) return hfail(MI_BAD_ARG, "bad device id");
    if (mi355x_device_count() < 1) return hfail(MI_NO_DEVICE, "no HIP device (gfx950) visible: there is no CPU fallback");
    std::unique_ptr<mi355x_bb> job(new (std::nothrow) mi355x_bb);
    if (!job) return hfail(MI_NO_MEMORY, "host allocation failed");
    job->base = *p;
    job->int_order.assign(int_order, int_order + n_int);
    job->f = fp_tolerance; job->int_f = int_tolerance;
    job->width = width; job->n_devices = n_devices;
    if (device_ids) job->device_ids.assign(device_ids, device_ids + n_devices);
    job->nodes.emplace_back();                                             // the root entry ()
    job->stack.push_back(0);
    *out = job.release();
    return MI_OK;
}

int mi355x_simplex_solver_bb_step(mi355x_bb *job, int64_t max_nodes, int64_t *n_nodes)
{
    if (n_nodes) *n_nodes = 0;
    if (!job) return hfail(MI_BAD_ARG, "job is NULL");
    if (max_nodes < 0) return hfail(MI_BAD_ARG, "max_nodes < 0");
    if (job->done) return job->status;
    mi355x_bb &j = *job;
    int64_t processed = 0;
    auto finished = [&](int rc) { j.done = true; j.status = rc; if (n_nodes) *n_nodes = processed; return rc; };
    auto paused = [&](int rc) { if (n_nodes) *n_nodes = processed; return rc; };
    while (!j.stack.empty()) {                                             // :517-539
        if (max_nodes && processed >= max_nodes) return paused(MI_MAX_PIVOTS);
        if (j.cancel.exchange(0)) return paused(MI_CANCELLED);
        const int64_t id = j.stack.back();
        if (!j.nodes[(size_t)id].solved) {
            int rc = j.round ? MI_OK : bb_round_begin(j);
            if (rc == MI_OK) rc = bb_round_advance(j);
            if (rc == MI_CANCELLED || rc == MI_MAX_PIVOTS) return paused(rc);   // bounded: back to the caller
            if (rc != MI_OK) return finished(rc);
            continue;
        }
        j.stack.pop_back();
        BBNode &n = j.nodes[(size_t)id];
        n.trace_index = (int64_t)j.trace.size();
        j.max_depth = std::max<int64_t>(j.max_depth, n.depth);
        ++processed;
        mi355x_bb::TraceRow row{n.parent >= 0 ? j.nodes[(size_t)n.parent].trace_index : -1, n.var, n.sense, n.bound,
                                MI_BB_FAILED, std::numeric_limits<double>::quiet_NaN()};
        if (n.status == MI_INFEASIBLE) {                                   // build-and-solve -> :infeasible
            row.outcome = MI_BB_INFEASIBLE;
            j.trace.push_back(row);
            continue;
        }
        if (n.status != MI_OPTIMAL) {                                      // any other condition ends the solve
            j.trace.push_back(row);
            return finished(n.status);
        }
        row.obj = n.obj;
        if (bb_prunable(j, n)) {
            row.outcome = MI_BB_PRUNED;
        } else if (n.viol >= 0) {                                          // (append (gen-entries tab entry) stack)
            row.outcome = MI_BB_BRANCHED;
            const int64_t ge = bb_child(j, id, 1), le = bb_child(j, id, 0);
            j.stack.push_back(ge);
            j.stack.push_back(le);
        } else if (j.incumbent < 0 || bb_better(j, j.nodes[(size_t)j.incumbent].obj, n.obj)) {
            row.outcome = MI_BB_INCUMBENT;
            if (j.incumbent >= 0) j.nodes[(size_t)j.incumbent].sol.reset();
            j.incumbent = id;
        } else {
            row.outcome = MI_BB_NOT_BETTER;
        }
        if (j.incumbent != id) j.nodes[(size_t)id].sol.reset();
        j.trace.push_back(row);
    }
    return finished(j.incumbent >= 0 ? MI_OPTIMAL : MI_INFEASIBLE);        // :540-542
}

int mi355x_simplex_solver_bb_cancel(mi355x_bb *job)
{
    if (!job) return hfail(MI_BAD_ARG, "job is NULL");
    job->cancel.store(1);
    return MI_OK;
}

int mi355x_simplex_solver_bb_finish(mi355x_bb *job, mi355x_solution **out)
{
    if (out) *out = nullptr;
    if (!job) return hfail(MI_BAD_ARG, "job is NULL");
    std::unique_ptr<mi355x_bb> owner(job);                                 // consumed whatever happens
    if (!out) return hfail(MI_BAD_ARG, "out is NULL");
    if (!job->done || job->status != MI_OPTIMAL)
        return hfail(MI_BAD_ARG, "the search has not ended with MI_OPTIMAL: there is no solution to read");
    *out = job->nodes[(size_t)job->incumbent].sol.release();
    return MI_OPTIMAL;
}

void mi355x_simplex_solver_bb_abandon(mi355x_bb *job) { delete job; }

int mi355x_simplex_solver_bb_stats(const mi355x_bb *job, int64_t *n_processed, int64_t *n_solved, int64_t *max_depth)
{
    if (!job) return hfail(MI_BAD_ARG, "job is NULL");
    if (n_processed) *n_processed = (int64_t)job->trace.size();
    if (n_solved) *n_solved = job->n_solved;
    if (max_depth) *max_depth = job->max_depth;
    return MI_OK;
}

int mi355x_simplex_solver_bb_trace(const mi355x_bb *job, int64_t *parent, int64_t *var, int32_t *sense, double *bound,
                                   int32_t *outcome, double *objective, int64_t cap, int64_t *n)
{
    if (!job || cap < 0) return hfail(MI_BAD_ARG, "bad arguments");
    const int64_t k = std::min<int64_t>(cap, (int64_t)job->trace.size());
    for (int64_t i = 0; i < k; ++i) {
        const mi355x_bb::TraceRow &r = job->trace[(size_t)i];
        if (parent) parent[i] = r.parent;
        if (var) var[i] = r.var;
        if (sense) sense[i] = r.sense;
        if (bound) bound[i] = r.bound;
        if (outcome) outcome[i] = r.outcome;
        if (objective) objective[i] = r.obj;
    }
    if (n) *n = (int64_t)job->trace.size();
    return MI_OK;
}

// test hook (mi355x_simplex_tune.h): n_nodes nodes of one depth assembled on `device` by launch_node_assemble and
// downloaded (tight rows x cols / rows x art_cols per node, NULL arrays: the shapes only)
int mi355x_bb_debug_assemble(const mi355x_problem *p, int64_t n_nodes, int64_t depth, const int64_t *var,
                             const int32_t *sense, const double *bound, int device, int64_t *rows, int64_t *cols,
                             int64_t *art_cols, double *main_out, int64_t *main_basis, double *art_out, int64_t *art_basis)
{
    if (!p || n_nodes < 1 || depth < 1 || !var || !sense || !bound) return hfail(MI_BAD_ARG, "bad arguments");
    for (int64_t i = 0; i < n_nodes * depth; ++i)
        if (var[i] < 0 || var[i] >= p->n_vars || sense[i] < 0 || sense[i] > 1) return hfail(MI_BAD_ARG, "bad node row");
    if (mi355x_device_count() < 1) return hfail(MI_NO_DEVICE, "no HIP device (gfx950) visible: there is no CPU fallback");
    mi355x_bb j;
    j.base = *p;
    int rc = bb_prepare_base(j);
    if (rc != MI_OK) return rc;
    int64_t n_art = -1;
    for (int64_t q = 0; q < n_nodes; ++q) {
        int64_t a = j.base_art;
        for (int64_t r = 0; r < depth; ++r)
            a += bb_row_artificial(j, var[q * depth + r], sense[q * depth + r], bound[q * depth + r]);
        if (n_art >= 0 && a != n_art) return hfail(MI_BAD_ARG, "the nodes have different numbers of artificial rows");
        n_art = a;
    }
    const int64_t R = j.grows + depth, C = j.gcols + depth;
    if (rows) *rows = R;
    if (cols) *cols = C;
    if (art_cols) *art_cols = n_art ? C + n_art : 0;
    if (!main_out && !main_basis && !art_out && !art_basis) return MI_OK;
    mi355x_multibatch *mb = nullptr, *ab = nullptr;
    rc = mi355x_bb_assemble_(j.dbase, n_nodes, depth, var, sense, bound, n_art, 1, &device, &mb, &ab);
    for (int64_t q = 0; rc == MI_OK && q < n_nodes; ++q) {
        rc = mi355x_multibatch_download(mb, q, main_out ? main_out + q * R * C : nullptr,
                                        main_basis ? main_basis + q * (R - 1) : nullptr, nullptr, nullptr);
        if (rc == MI_OK && ab)
            rc = mi355x_multibatch_download(ab, q, art_out ? art_out + q * R * (C + n_art) : nullptr,
                                            art_basis ? art_basis + q * (R - 1) : nullptr, nullptr, nullptr);
    }
    mi355x_multibatch_destroy(mb);
    mi355x_multibatch_destroy(ab);
    return rc;
}

}  // extern "C"
