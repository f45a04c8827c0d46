// bfs.hip — Rodinia BFS as device task kinds of the work-stealing scheduler.
//
// The reference (test/performance-regression/full-apps/rodinia/bfs/bfs.cpp; the
// algorithm as bfs.ref.cpp:135-183 states it) runs every level as two sweeps
// over all vertices, the first relaxing the edges of the vertices in
// h_graph_mask, the second moving h_updating_graph_mask into the mask and
// h_graph_visited, with a wait after each: O(V depth) work and two joins per
// level. Both forms here run in one launch:
//
//   level (HCLIB_HIP_BFS_LEVEL)
//     The reference's schedule over the frontier alone. `order` holds the
//     reached vertices in claiming order, so level L is a range of it. The
//     LEVEL template {LEVEL, L, off_L, n_L} has the level's vertices as its
//     children: child k reads v = order[off_L + k] and returns the VERTEX
//     template {VERTEX, v, starting[v], L} with degree[v] children, the edges
//     of v. Edge k claims id = edges[start + k] with one compare-and-swap of
//     cost[id] from -1 to L + 1; the winner appends id to `order` through one
//     64-bit add on `packed` (the reached count above bit 40, the sum of the
//     reached vertices' degrees below), whose old count is its slot.
//     A level closes without any wait. Every item a lane runs, vertex or
//     edge, adds 1 to the lane's pending count; when a wave's ring runs empty
//     its drain adds the wave's sum to the monotonic `done` (an agent release
//     before, an acquire after). The items of levels 0 .. L number target_L =
//     (vertices in them) + (their degrees summed), and items of level L + 1
//     do not exist before L is closed, so exactly one add lands on target_L,
//     after every item of the level has run and been flushed. That wave's
//     renew (hx_sched.h) reads `packed`, records where level L + 1 ends,
//     stores target_{L+1} and returns the next LEVEL template, or 0 where the
//     level is empty: the launch then ends through `outstanding` as always.
//     order, packed, done and target only grow; nothing is reset and nothing
//     spins: a miscount would end the launch early, it could not hang it.
//   async (HCLIB_HIP_BFS_ASYNC)
//     No levels, no order, no renew. The VERTEX template {VERTEX, v, start, d}
//     says that v was given cost d. Its items are out of date, and return
//     without relaxing, when cost[v] is below d by now. Otherwise edge k
//     lowers cost[id] with an unsigned atomic minimum (-1 is the largest
//     value) to d + 1, and a strict lowering returns id's VERTEX template.
//     Unit weights: the fixed point is the same cost array bit for bit.
//
// Visibility across XCDs (their L2s are not coherent with each other): cost
// and packed are touched by agent atomics only; order entries are sc1 stores
// (st_sc1_u32) made visible by the storing wave's release before its add on
// done, and read with agent loads; target and level are agent stores of the
// closing wave, read after an acquire. starting, degree and edges are
// read-only and take plain loads.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hx_bfs_plan.h"
#include "hx_client.h"

namespace hx {

constexpr uint32_t kBfsTagLevel = 0, kBfsTagVertex = 1, kBfsTagRoot = 2;

struct BfsCtx {
    unsigned long long *ctl;  // packed, done, target, level (hx_bfs_plan.h)
    int32_t *cost;
    const int32_t *starting, *degree, *edges;
    uint32_t *order, *lvl_off;  // level form
    uint32_t source;
};

struct BfsAcc {
    unsigned long long items = 0, relaxed = 0, stale = 0;
    uint32_t pending = 0;  // items run since the wave's last flush (level form)
    uint32_t closed = 0;   // wave-uniform: this wave's last flush closed the open level
    __device__ void totals(unsigned long long (&c)[8], unsigned long long (&)[4]) {
        c[0] = wave_sum(items);
        c[1] = wave_sum(relaxed);
        c[2] = wave_sum(stale);
    }
};

struct BfsLevelKind {
    static constexpr int kTmplWords = 6;
    static constexpr int kWords = 8;
    static constexpr bool kPure = false;
    static constexpr bool kBoundedChildren = true;  // n_nodes and every degree < 2^24 (bfs_plan)
    using Ctx = BfsCtx;
    using Acc = BfsAcc;

    // level 0: the source, which the host put into order[0]
    __device__ static int roots(const Ctx &, Acc &, uint32_t *tmpl) {
        tmpl[0] = kBfsTagLevel;
        tmpl[1] = tmpl[2] = tmpl[4] = tmpl[5] = 0;
        tmpl[3] = 1;
        return 1;
    }

    // One add on `packed` per claiming lane. One per batch (the winners ranked
    // with a ballot, the first adding for all) measured the same on 2^20
    // vertices: 3.92 against 3.94 ms, ten launches each spread over 0.09 and
    // 0.12 ms (profiles/r22/bfs_packed_add_ab.json), so the plain form stays.
    __device__ static int process(const Ctx &c, Acc &acc, const uint32_t *t, uint32_t k, uint32_t *child, uint32_t *,
                                  bool) {
        acc.items += 1;
        acc.pending += 1;
        if (t[0] == kBfsTagLevel) {
            const uint32_t v = ld_agent(&c.order[t[2] + k]);
            child[0] = kBfsTagVertex;
            child[1] = v;
            child[2] = (uint32_t)c.starting[v];
            child[3] = t[1];
            child[4] = child[5] = 0;
            return c.degree[v];
        }
        const int32_t id = c.edges[t[2] + k];
        const int32_t next = (int32_t)t[3] + 1;
        acc.relaxed += 1;
        // cost[id] leaves -1 once and for good: a value read as set is set
        if (ld_agent(&c.cost[id]) == -1 && cas_agent(&c.cost[id], (int32_t)-1, next)) {
            const unsigned long long old =
                add_agent(&c.ctl[0], (1ull << kBfsCountShift) + (unsigned long long)(uint32_t)c.degree[id]);
            st_sc1_u32(&c.order[(uint32_t)(old >> kBfsCountShift)], (uint32_t)id);
        }
        return 0;
    }

    // the ring ran empty: the items run since the last flush are counted
    // (whole wave, uniform control flow)
    __device__ static void drain(const Ctx &c, Acc &acc, uint32_t *) {
        const uint32_t s = wave_sum(acc.pending);
        acc.pending = 0;
        acc.closed = 0;
        if (s == 0) return;
        // this wave's order entries and claims are visible before its count is
        release_agent();
        const bool first = lane_id() == 0;
        unsigned long long now = 0;
        if (first) now = add_agent(&c.ctl[1], (unsigned long long)s) + s;
        // what the waves that counted before this one wrote, and the target
        acquire_agent();
        uint32_t hit = 0;
        if (first) hit = now == ld_agent(&c.ctl[2]) ? 1u : 0u;
        acc.closed = (uint32_t)__builtin_amdgcn_readfirstlane((int)hit);
    }

    // the wave whose flush closed level L opens level L + 1
    __device__ static int renew(const Ctx &c, Acc &acc, uint32_t *tmpl) {
        if (!acc.closed) return 0;
        acc.closed = 0;
        const unsigned long long packed = ld_agent(&c.ctl[0]);
        const uint32_t reached = (uint32_t)(packed >> kBfsCountShift);
        const unsigned long long degsum = packed & ((1ull << kBfsCountShift) - 1);
        const uint32_t L = (uint32_t)ld_agent(&c.ctl[3]);
        const uint32_t off = ld_agent(&c.lvl_off[L + 1]);
        const uint32_t n = reached - off;
        if (lane_id() == 0) {
            st_agent(&c.lvl_off[L + 2], reached);
            if (n) {
                st_agent(&c.ctl[2], (unsigned long long)reached + degsum);
                st_agent(&c.ctl[3], (unsigned long long)(L + 1));
            }
        }
        // the stores have left before the template can reach another wave
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tmpl[0] = kBfsTagLevel;
        tmpl[1] = L + 1;
        tmpl[2] = off;
        tmpl[3] = n;
        tmpl[4] = tmpl[5] = 0;
        return (int)n;
    }
};

struct BfsAsyncKind {
    static constexpr int kTmplWords = 6;
    static constexpr int kWords = 8;
    static constexpr bool kPure = false;
    static constexpr bool kBoundedChildren = true;
    using Ctx = BfsCtx;
    using Acc = BfsAcc;

    // one item that stands for the host's cost[source] = 0
    __device__ static int roots(const Ctx &, Acc &, uint32_t *tmpl) {
        tmpl[0] = kBfsTagRoot;
        tmpl[1] = tmpl[2] = tmpl[3] = tmpl[4] = tmpl[5] = 0;
        return 1;
    }

    __device__ static int process(const Ctx &c, Acc &acc, const uint32_t *t, uint32_t k, uint32_t *child, uint32_t *,
                                  bool) {
        acc.items += 1;
        uint32_t id, d;
        if (t[0] == kBfsTagRoot) {
            id = c.source;
            d = 0;
        } else {
            if ((uint32_t)ld_agent(&c.cost[t[1]]) < t[3]) {  // v has a shorter path by now: its items follow
                acc.stale += 1;
                return 0;
            }
            id = (uint32_t)c.edges[t[2] + k];
            d = t[3] + 1;
            acc.relaxed += 1;
            const uint32_t old = __hip_atomic_fetch_min((uint32_t *)&c.cost[id], d, __ATOMIC_RELAXED, HX_AGENT);
            if (old <= d) return 0;
        }
        child[0] = kBfsTagVertex;
        child[1] = id;
        child[2] = (uint32_t)c.starting[id];
        child[3] = d;
        child[4] = child[5] = 0;
        return c.degree[id];
    }
};

constexpr int kBfsCap = 1024;  // ring items per wave

template <class K>
__global__ __launch_bounds__(64) void k_bfs(BfsCtx ctx, PoolView pool, SchedGlobals *g, SchedConfig cfg) {
    __shared__ WaveStack<K, kBfsCap> st;
    run_worker<K, kBfsCap>(ctx, pool, g, cfg, st, blockIdx.x == 0);
}

}  // namespace hx

using namespace hx;

namespace {

int bfs_check(const char *who, const int32_t *starting, const int32_t *degree, int n_nodes, const int32_t *edges,
              int n_edges, int source, int form, BfsPlan &p) {
    std::string err;
    if (bfs_plan(starting, degree, n_nodes, edges, n_edges, source, form, p, err)) {
        set_error("%s: %s", who, err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    return HCLIB_HIP_OK;
}

}  // namespace

extern "C" int hclib_hip_bfs_bounds(const int32_t *starting, const int32_t *degree, int n_nodes, const int32_t *edges,
                                    int n_edges, int source, int form, uint64_t out[2]) {
    if (!out) {
        set_error("hclib_hip_bfs_bounds: out is NULL");
        return HCLIB_HIP_EINVAL;
    }
    BfsPlan p;
    HX_TRY(bfs_check("hclib_hip_bfs_bounds", starting, degree, n_nodes, edges, n_edges, source, form, p));
    out[0] = p.bytes;
    out[1] = p.items;
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_bfs_read_input(const char *path, int32_t *starting, int32_t *degree, int32_t *edges,
                                        int64_t counts[3]) {
    std::string err;
    if (bfs_read_input(path, starting, degree, edges, counts, err)) {
        set_error("hclib_hip_bfs_read_input: %s", err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_bfs(const int32_t *starting, const int32_t *degree, int n_nodes, const int32_t *edges,
                             int n_edges, int source, int form, int32_t *cost, hclib_hip_bfs_result_t *result,
                             uint64_t *frontier, int32_t *order) {
    const char *who = "hclib_hip_bfs";
    if (!cost || !result) {
        set_error("%s: cost or result is NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    BfsPlan p;
    HX_TRY(bfs_check(who, starting, degree, n_nodes, edges, n_edges, source, form, p));
    const bool level = form == kBfsLevel;
    if (order && !level) {
        set_error("%s: the async form keeps no order", who);
        return HCLIB_HIP_EINVAL;
    }
    HX_TRY(ensure_device());
    Module &m = mod();
    const int grid = sched_grid(3);
    DevBuf buf;
    HX_TRY(buf.alloc(p.bytes, who));
    char *d = buf.p;
    BfsCtx ctx;
    ctx.ctl = (unsigned long long *)d;
    ctx.cost = (int32_t *)(d + p.off_cost);
    ctx.starting = (const int32_t *)(d + p.off_starting);
    ctx.degree = (const int32_t *)(d + p.off_degree);
    ctx.edges = (const int32_t *)(d + p.off_edges);
    ctx.order = level ? (uint32_t *)(d + p.off_order) : nullptr;
    ctx.lvl_off = level ? (uint32_t *)(d + p.off_lvl) : nullptr;
    ctx.source = (uint32_t)source;
    const size_t nb = 4 * (size_t)n_nodes;
    // h_cost = -1 but for the source (bfs.ref.cpp:128-131); order and lvl_off
    // start as -1 / 0 so that what the launch did not write reads as unset
    HX_HIP(hipMemsetAsync(ctx.cost, 0xff, nb, m.stream));
    HX_TRY(upload_async((void *)ctx.starting, starting, nb, m.stream));
    HX_TRY(upload_async((void *)ctx.degree, degree, nb, m.stream));
    if (n_edges) HX_TRY(upload_async((void *)ctx.edges, edges, 4 * (size_t)n_edges, m.stream));
    const unsigned long long deg0 = (unsigned long long)degree[source];
    unsigned long long ctl[32] = {};
    ctl[0] = (1ull << kBfsCountShift) + deg0;  // the source is reached
    ctl[2] = 1 + deg0;                         // level 0: one vertex item and its edges
    HX_TRY(upload_async(ctx.ctl, ctl, sizeof(ctl), m.stream));
    const int32_t zero = 0;
    HX_TRY(upload_async(ctx.cost + source, &zero, 4, m.stream));
    if (level) {
        HX_HIP(hipMemsetAsync(ctx.order, 0xff, nb, m.stream));
        HX_HIP(hipMemsetAsync(ctx.lvl_off, 0, 4 * ((size_t)n_nodes + 2), m.stream));
        const uint32_t head[2] = {0, 1}, src = (uint32_t)source;
        HX_TRY(upload_async(ctx.lvl_off, head, sizeof(head), m.stream));
        HX_TRY(upload_async(ctx.order, &src, 4, m.stream));
    }
    PoolView pool;
    HX_TRY(sched_pool(64, (uint32_t)env_int("HCLIB_HIP_BFS_CHUNK", 32), 8, &pool));
    const SchedConfig cfg = sched_config_unseeded("BFS", grid);
    HX_TRY(reset_sched(pool, 1u, false, (uint32_t)grid));
    void (*const kern)(BfsCtx, PoolView, SchedGlobals *, SchedConfig) =
        level ? k_bfs<BfsLevelKind> : k_bfs<BfsAsyncKind>;
    SchedGlobals gl;
    float ms = 0;
    HX_TRY(launch_sched((const void *)kern, grid, 64, who, [&] {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, m.stream, ctx, pool, m.globals, cfg);
    }, &gl, &ms, "hipLaunchKernelGGL(k_bfs)"));
    HX_HIP(hipMemcpy(cost, ctx.cost, nb, hipMemcpyDeviceToHost));
    // the frontier sizes: from the level offsets where the launch kept them
    // (and checked against cost below), else counted from cost
    std::vector<uint64_t> fr;
    uint64_t reached = 0;
    for (int v = 0; v < n_nodes; ++v) {
        if (cost[v] < 0) continue;
        ++reached;
        if ((size_t)cost[v] >= fr.size()) fr.resize((size_t)cost[v] + 1, 0);
        ++fr[(size_t)cost[v]];
    }
    if (level) {
        unsigned long long end[4] = {};
        HX_HIP(hipMemcpy(end, ctx.ctl, sizeof(end), hipMemcpyDeviceToHost));
        std::vector<uint32_t> off((size_t)n_nodes + 2);
        HX_HIP(hipMemcpy(off.data(), ctx.lvl_off, 4 * off.size(), hipMemcpyDeviceToHost));
        // the device's own account must be the one cost gives: a level that
        // closed early or late shows here, whatever cost looks like
        bool same = end[3] + 1 == fr.size() && (end[0] >> kBfsCountShift) == reached && end[1] == end[2];
        for (size_t l = 0; same && l < fr.size(); ++l) same = (uint64_t)off[l + 1] - off[l] == fr[l];
        if (!same) {
            set_error("%s: the level offsets the launch recorded do not match its cost array (levels %llu / %zu, "
                      "reached %llu / %llu, done %llu of %llu)", who, end[3] + 1, fr.size(), end[0] >> kBfsCountShift,
                      (unsigned long long)reached, end[1], end[2]);
            return HCLIB_HIP_EDEVICE;
        }
        if (order) HX_HIP(hipMemcpy(order, ctx.order, nb, hipMemcpyDeviceToHost));
    }
    if (frontier)
        for (int l = 0; l < n_nodes; ++l) frontier[l] = (size_t)l < fr.size() ? fr[(size_t)l] : 0;
    result->levels = fr.size();
    result->reached = reached;
    result->relaxed = gl.counters[1];
    result->items = gl.counters[0];
    result->chunks_pushed = gl.counters[kCtrPushed];
    result->chunks_stolen = gl.counters[kCtrStolen];
    result->kernel_ms = ms;
    result->busy_frac = busy_frac(gl);
    return HCLIB_HIP_OK;
}
