// nqueens.hip — N-Queens as device task kinds of the work-stealing scheduler.
//
// The reference ships the program in two forms, and both run here:
//
//   BOTS (test/performance-regression/full-apps/bots/nqueens/nqueens.c:125-182)
//     a call nqueens(n, j, a) with j < n opens a finish, spawns one task per
//     column i of row j, and sums csols[] behind the end_finish; a task copies
//     the board, places a[j] = i and, if ok(), is the call nqueens(n, j + 1).
//     Here a call opens a finish scope (hx_finish.h) under its caller's scope,
//     its column tasks are the scope's tasks, and `*solutions += csols[i]` is
//     the scope's sum climbing through finish_check_out with PassSum; the root
//     value is the count.
//   flat (test/performance-regression/full-apps/nqueens.cpp:41-60, test/misc)
//     one outer finish, an async only for a placement that passes ok(), one
//     atomic counter. Here a pure kind: no scopes, solutions counted per lane
//     in Acc and summed at the wave's exit (the privatised form of the one
//     __sync_fetch_and_add).
//
// A board prefix of j queens is three column masks (occupied columns, the two
// diagonals shifted one per row) in the 6-word template, so ok() for column k
// is one AND against the free mask and the child's state three ORs and
// shifts: no board array, no allocation. Child k of a template is the k-th
// set bit of its free mask (BOTS with every placement spawned: column k).
//
// Task depth d (the BOTS manual cutoff, nqueens_ser of nqueens.ref.c:99-123):
// a call with j >= d is finished by its lane alone, a depth-first search over
// the masks whose per-row candidate masks live in a per-lane LDS stack.
#include <stdio.h>
#include <string.h>

#include <mutex>

#include "hx_client.h"
#include "../../include/hclib_hip/hx_finish.h"

namespace hx {

constexpr int kNqMaxN = 20;
constexpr uint32_t kNqRootRow = 0xffffffffu;  // template word 3 of the root: its one child is the empty board

struct NqCtx {
    uint32_t n, full;  // full = the n column bits
    uint32_t m;        // calls with j < m spawn tasks, a call with j >= m is one lane's serial search (1..n)
    int all;           // BOTS: conflicting placements travel as items too (the reference's n asyncs per call)
    int local;         // scopes in the wave's LDS while they stay inside it (as FibCtx::local)
    int blocks;        // HBM scope ids taken kScopeBlock at a time per wave
    unsigned long long *hist;  // n + 1 words (the histogram instantiations), or null
    FinishArena fin;
};

// the wave's LDS finish scopes and its block of HBM scope ids (as fib.hip)
constexpr int kNqLocalScopes = 256;
__shared__ LocalScopes<kNqLocalScopes> s_nq_scopes;
__shared__ uint32_t s_nq_blk[2];
// the serial search's candidate masks, one column of the array per lane
__shared__ uint32_t s_nq_stack[kNqMaxN][64];
// the wave's share of the per-depth histogram, handed over when it goes idle
__shared__ unsigned long long s_nq_hist[kNqMaxN + 1];

template <bool HIST>
__device__ __forceinline__ void nq_hist_add(uint32_t j, uint32_t v) {
    if constexpr (HIST)
        __hip_atomic_fetch_add(&s_nq_hist[j], (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// (whole wave, uniform control flow: the drain hook)
__device__ __forceinline__ void nq_hist_flush(const NqCtx &c) {
    const int lane = lane_id();
    if (c.hist && lane <= (int)c.n) {
        const unsigned long long v = s_nq_hist[lane];
        if (v) {
            add_agent(&c.hist[lane], v);
            s_nq_hist[lane] = 0;
        }
    }
    asm volatile("" ::: "memory");
}

// the k-th set bit of m (0 if m has no more than k)
__device__ __forceinline__ uint32_t nq_kth_bit(uint32_t m, uint32_t k) {
    for (uint32_t i = 0; i < k && m; ++i) m &= m - 1;
    return m & (0u - m);
}

// The board a lane's item stands for: child k of template t.
struct NqBoard {
    uint32_t cols, ld, rd, j;
    bool conflict;  // the placement fails ok() (only where conflicting placements are items)
};
__device__ __forceinline__ NqBoard nq_child(const NqCtx &c, const uint32_t *t, uint32_t k, bool all) {
    NqBoard b;
    if (t[3] == kNqRootRow) {
        b.cols = b.ld = b.rd = b.j = 0;
        b.conflict = false;
        return b;
    }
    const uint32_t free = c.full & ~(t[0] | t[1] | t[2]);
    const uint32_t bit = nq_kth_bit(all ? c.full : free, k);
    b.conflict = (bit & free) == 0;
    b.cols = t[0] | bit;
    b.ld = ((t[1] | bit) << 1) & c.full;
    b.rd = (t[2] | bit) >> 1;
    b.j = t[3] + 1;
    return b;
}

// nqueens_ser from a prefix of `row` < n queens: the number of solutions below
// it. Depth first over the masks; level s of the lane's LDS stack holds the
// candidates of row + s that are still to try, the lowest being the one
// placed. The diagonals are kept in 64 bits so that a placement is undone by
// the opposite shift (no bit of either is lost in n <= 20 rows).
template <bool HIST>
__device__ __forceinline__ unsigned long long nq_serial(const NqCtx &c, uint32_t cols, uint32_t ld, uint32_t rd,
                                                        uint32_t row) {
    const int lane = lane_id();
    unsigned long long L = ld, R = (unsigned long long)rd << 32, count = 0;
    uint32_t sp = 0;
    uint32_t avail = c.full & ~(cols | ld | rd);
    while (true) {
        if (row + sp + 1 == c.n) {  // the last row: every free column completes a board
            const uint32_t s = (uint32_t)__popc(avail);
            count += s;
            if (s) nq_hist_add<HIST>(c.n, s);
            avail = 0;
        }
        if (avail == 0) {
            if (sp == 0) break;
            --sp;
            avail = s_nq_stack[sp][lane];
            const uint32_t bit = avail & (0u - avail);
            cols ^= bit;
            L = (L >> 1) & ~(unsigned long long)bit;
            R = (R << 1) & ~((unsigned long long)bit << 32);
            avail &= avail - 1;
            continue;
        }
        const uint32_t bit = avail & (0u - avail);
        s_nq_stack[sp][lane] = avail;
        cols |= bit;
        L = (L | bit) << 1;
        R = (R | ((unsigned long long)bit << 32)) >> 1;
        ++sp;
        nq_hist_add<HIST>(row + sp, 1u);
        avail = c.full & ~(cols | (uint32_t)L | (uint32_t)(R >> 32));
    }
    return count;
}

struct NqAcc {
    unsigned long long items = 0, joins = 0, calls = 0, sols = 0;
    FinishInFlight q;  // BOTS, LDS scopes: this lane's HBM check-out step in flight
    __device__ void totals(unsigned long long (&c)[8], unsigned long long (&)[4]) {
        c[0] = wave_sum(items);
        c[1] = wave_sum(joins);
        c[2] = wave_sum(calls);
        c[3] = wave_sum(sols);
    }
};

template <bool HIST>
struct NqBotsKind {
    // template = {columns, left diagonal, right diagonal, j, the call's scope, 0}
    // of the call nqueens(n, j, a): its children are the tasks of row j
    static constexpr int kTmplWords = 6;
    static constexpr int kWords = 8;
    static constexpr bool kPure = false;           // scopes are opened / checked out
    static constexpr bool kBoundedChildren = true;  // at most n
    using Ctx = NqCtx;
    using Acc = NqAcc;

    __device__ static int roots(const Ctx &, Acc &, uint32_t *tmpl) {
        tmpl[0] = tmpl[1] = tmpl[2] = tmpl[5] = 0;
        tmpl[3] = kNqRootRow;
        tmpl[4] = kScopeRoot;
        return 1;
    }

    __device__ static int process(const Ctx &c, Acc &acc, const uint32_t *t, uint32_t k, uint32_t *child,
                                  uint32_t *err, bool) {
        // the HBM check-out this lane issued a batch ago: its result is in
        if (c.local) acc.joins += finish_resolve(c.fin, acc.q, PassSum());
        const NqBoard b = nq_child(c, t, k, c.all != 0);
        acc.items += 1;
        // a conflicting placement leaves csols[i] = 0, a full board is 1, a call
        // at the task depth is its lane's serial count, a call above it spawns
        unsigned long long value = 0;
        uint32_t cnt = 0;
        if (!b.conflict) {
            nq_hist_add<HIST>(b.j, 1u);
            if (b.j == c.n) {
                value = 1;
            } else if (b.j >= c.m) {
                value = nq_serial<HIST>(c, b.cols, b.ld, b.rd, b.j);
            } else {
                acc.calls += 1;
                cnt = c.all ? c.n : (uint32_t)__popc(c.full & ~(b.cols | b.ld | b.rd));
            }
        }
        // start_finish; n asyncs (the parent settles the conflicting ones: the
        // scope counts the free columns only; none free: the finish closes at
        // once on a sum of zero, and no scope is opened for it)
        const bool spawn = cnt != 0;
        const uint32_t s = c.local ? finish_open_local(c.fin, s_nq_scopes, spawn, t[4], cnt, 0, err,
                                                       c.blocks ? s_nq_blk : nullptr)
                                   : finish_open(c.fin, spawn, t[4], cnt, 0, err, c.blocks ? s_nq_blk : nullptr);
        if (spawn) {
            if (s == kScopeRoot) return 0;  // arena error (reported)
            child[0] = b.cols;
            child[1] = b.ld;
            child[2] = b.rd;
            child[3] = b.j;
            child[4] = s;
            child[5] = 0;
            return (int)cnt;
        }
        acc.joins += c.local ? finish_check_out_local(c.fin, s_nq_scopes, t[4], value, PassSum(), &acc.q)
                             : finish_check_out(c.fin, t[4], value, PassSum());
        return 0;
    }

    // the ring ran empty: the check-outs still in flight, to their ends
    __device__ static void drain(const Ctx &c, Acc &acc, uint32_t *) {
        if (c.local) acc.joins += finish_drain(c.fin, acc.q, PassSum());
        if constexpr (HIST) nq_hist_flush(c);
    }

    // an item leaving the wave names an HBM scope (its LDS scope promoted)
    __device__ static void export_item(const Ctx &c, uint32_t *w, bool valid, uint32_t *err) {
        if (!c.local) return;
        const uint32_t s = finish_promote(c.fin, s_nq_scopes, valid ? w[4] : kScopeRoot, err);
        if (valid) w[4] = s;
    }
};

template <bool HIST>
struct NqFlatKind {
    // template = {columns, left diagonal, right diagonal, j, 0, 0} of
    // nqueens_kernel(A, j, n): its children are the placements that pass ok()
    static constexpr int kTmplWords = 6;
    static constexpr int kWords = 8;
    static constexpr bool kPure = true;
    static constexpr bool kBoundedChildren = true;
    using Ctx = NqCtx;
    using Acc = NqAcc;

    __device__ static int roots(const Ctx &, Acc &, uint32_t *tmpl) {
        tmpl[0] = tmpl[1] = tmpl[2] = tmpl[4] = tmpl[5] = 0;
        tmpl[3] = kNqRootRow;
        return 1;
    }

    // (pure: every lane runs; a lane without an item holds whatever its ring
    // slot held, so nothing it computes is kept and its loops do not run)
    __device__ static int process(const Ctx &c, Acc &acc, const uint32_t *t, uint32_t k, uint32_t *child, uint32_t *,
                                  bool valid) {
        const NqBoard b = nq_child(c, t, valid ? k : 0u, false);
        acc.items += valid ? 1u : 0u;
        if (valid) nq_hist_add<HIST>(b.j, 1u);
        const bool done = b.j >= c.n, serial = !done && b.j >= c.m;
        if (valid && done) acc.sols += 1;
        if (valid && serial) acc.sols += nq_serial<HIST>(c, b.cols, b.ld, b.rd, b.j);
        child[0] = b.cols;
        child[1] = b.ld;
        child[2] = b.rd;
        child[3] = b.j;
        child[4] = 0;
        child[5] = 0;
        return (valid && !done && !serial) ? (int)__popc(c.full & ~(b.cols | b.ld | b.rd)) : 0;
    }

    __device__ static void drain(const Ctx &c, Acc &, uint32_t *) {
        if constexpr (HIST) nq_hist_flush(c);
    }
};

constexpr int kNqCap = 1024;  // ring items per wave

template <class K>
__global__ __launch_bounds__(64) void k_nqueens(NqCtx ctx, PoolView pool, SchedGlobals *g, SchedConfig cfg) {
    __shared__ WaveStack<K, kNqCap> st;
    if constexpr (!K::kPure) {
        if (ctx.local) s_nq_scopes.init();
        if (threadIdx.x < 2) s_nq_blk[threadIdx.x] = 0;
    }
    if (ctx.hist && threadIdx.x <= kNqMaxN) s_nq_hist[threadIdx.x] = 0;
    __syncthreads();
    run_worker<K, kNqCap>(ctx, pool, g, cfg, st, blockIdx.x == 0);
}

}  // namespace hx

using namespace hx;

namespace {

// ids the arena keeps beyond the scopes themselves: each wave's last partly
// used id block and the root. A constant, so that hclib_hip_nqueens_bounds
// (which knows no grid) and the launch accept exactly the same calls
constexpr unsigned long long kNqIdReserve = 1ull << 24;
constexpr unsigned long long kNqScopeLimit = 0xfffffff0ull - kNqIdReserve;

// Counts the valid prefixes below the prefix (cols, ld, rd) of j queens down
// to length `top` (j < top), those of length `top` by their parents' free
// masks. False as soon as the count passes `limit`.
bool nq_walk(uint32_t full, uint32_t cols, uint32_t ld, uint32_t rd, int j, int top, unsigned long long limit,
             unsigned long long &cnt) {
    uint32_t avail = full & ~(cols | ld | rd);
    if (j + 1 == top) {
        cnt += (unsigned)__builtin_popcount(avail);
        return cnt <= limit;
    }
    if (j + 2 == top) {  // the last two levels without a call each
        unsigned long long c = (unsigned)__builtin_popcount(avail);
        while (avail) {
            const uint32_t bit = avail & (0u - avail);
            avail ^= bit;
            c += (unsigned)__builtin_popcount(full & ~((cols | bit) | ((ld | bit) << 1) | ((rd | bit) >> 1)));
        }
        cnt += c;
        return cnt <= limit;
    }
    while (avail) {
        const uint32_t bit = avail & (0u - avail);
        avail ^= bit;
        if (++cnt > limit) return false;
        if (!nq_walk(full, cols | bit, ((ld | bit) << 1) & full, (rd | bit) >> 1, j + 1, top, limit, cnt)) return false;
    }
    return true;
}

// The same from the empty board, the mirror image of every prefix counted
// with it: the first queen takes the left half of its row only (and, n odd,
// the middle column, whose subtree is its own mirror image). Exact, and false
// as soon as the count passes `limit`.
bool nq_count(int n, int top, unsigned long long limit, unsigned long long &cnt) {
    const uint32_t full = (1u << n) - 1u;
    cnt = 1;  // the empty prefix
    if (top < 1) return true;
    for (int i = 0; i < (n + 1) / 2; ++i) {
        const uint32_t bit = 1u << i;
        const unsigned long long w = (2 * i + 1 == n) ? 1 : 2;
        if (limit - cnt < w) return false;
        unsigned long long sub = 1;  // the prefix of this one queen
        const bool fits = top == 1 || nq_walk(full, bit, (bit << 1) & full, bit >> 1, 1, top, (limit - cnt) / w, sub);
        if (!fits) return false;
        cnt += w * sub;
    }
    return true;
}

struct NqPlan {
    uint32_t m;                        // the effective task depth, 1..n
    unsigned long long tasks, scopes;  // by the reference's definitions
};

// the argument checks and the counts both entry points share
int nq_plan(const char *who, int n, int form, int task_depth, bool count, NqPlan *p) {
    if (n < 1 || n > kNqMaxN) {
        set_error("%s: n = %d must be in [1, %d]", who, n, kNqMaxN);
        return HCLIB_HIP_EINVAL;
    }
    if (form != HCLIB_HIP_NQUEENS_BOTS && form != HCLIB_HIP_NQUEENS_FLAT) {
        set_error("%s: form %d is neither HCLIB_HIP_NQUEENS_BOTS nor HCLIB_HIP_NQUEENS_FLAT", who, form);
        return HCLIB_HIP_EINVAL;
    }
    if (task_depth < 0) {
        set_error("%s: task_depth = %d must not be negative", who, task_depth);
        return HCLIB_HIP_EINVAL;
    }
    p->m = (task_depth == 0 || task_depth > n) ? (uint32_t)n : (uint32_t)task_depth;
    p->tasks = p->scopes = 0;
    if (!count) return HCLIB_HIP_OK;
    // P(n, j) = valid prefixes of length j. BOTS: one scope per call with
    // j < m, n tasks per scope. Flat: one task per valid prefix of length 1..m
    const bool bots = form == HCLIB_HIP_NQUEENS_BOTS;
    const int top = bots ? (int)p->m - 1 : (int)p->m;
    // the last count is kept: repeated launches of one size, or the helper and
    // then the launch, walk the prefixes once
    static std::mutex mu;
    static int last_n = 0, last_top = 0;
    static bool last_bots = false, last_fits = false;
    static unsigned long long last_cnt = 0;
    std::lock_guard<std::mutex> lock(mu);
    if (!(last_n == n && last_top == top && last_bots == bots)) {
        const unsigned long long limit = bots ? kNqScopeLimit : ~0ull >> 2;
        last_fits = nq_count(n, top, limit, last_cnt);
        last_n = n;
        last_top = top;
        last_bots = bots;
    }
    const unsigned long long cnt = last_cnt;
    if (!last_fits) {
        set_error("%s: n = %d at task depth %u opens more finish scopes than the arena can address (%llu)", who, n,
                  p->m, kNqScopeLimit);
        return HCLIB_HIP_EINVAL;
    }
    if (bots) {
        p->scopes = cnt;
        p->tasks = cnt * (unsigned long long)n;
    } else {
        p->tasks = cnt - 1;
    }
    return HCLIB_HIP_OK;
}

}  // namespace

extern "C" int hclib_hip_nqueens_bounds(int n, int form, int task_depth, uint64_t out[2]) {
    if (!out) {
        set_error("hclib_hip_nqueens_bounds: out is NULL");
        return HCLIB_HIP_EINVAL;
    }
    NqPlan p;
    HX_TRY(nq_plan("hclib_hip_nqueens_bounds", n, form, task_depth, true, &p));
    out[0] = p.tasks;
    out[1] = p.scopes;
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_nqueens(int n, int form, int task_depth, hclib_hip_nqueens_result_t *result,
                                 uint64_t *hist) {
    if (!result) {
        set_error("hclib_hip_nqueens: result is NULL");
        return HCLIB_HIP_EINVAL;
    }
    NqPlan p;
    // the BOTS arena holds every scope once: the exact count (the flat form
    // has no arena, and its count would be the whole search on the host)
    const bool bots = form == HCLIB_HIP_NQUEENS_BOTS;
    HX_TRY(nq_plan("hclib_hip_nqueens", n, form, task_depth, bots, &p));
    HX_TRY(ensure_device());
    Module &m = mod();
    const int grid = sched_grid(3);
    const int blocks = env_int("HCLIB_HIP_NQUEENS_BLOCKS", 1);
    if (bots && 1ull + (unsigned long long)grid * kScopeBlock > kNqIdReserve) {
        set_error("hclib_hip_nqueens: %d workers need more scope id blocks than the arena reserves", grid);
        return HCLIB_HIP_EINVAL;
    }
    const unsigned long long ids = bots ? p.scopes + 1 + (blocks ? (unsigned long long)grid * kScopeBlock : 0ull) : 1ull;
    const size_t jb = (sizeof(FinishScope) * (size_t)ids + 255) & ~(size_t)255;
    const size_t hb = hist ? 256 : 0;  // behind the arena's counters: n + 1 words
    DevBuf buf;
    HX_TRY(buf.alloc(jb + 256 + hb, "hclib_hip_nqueens"));
    char *dmem = buf.p;
    NqCtx ctx;
    ctx.n = (uint32_t)n;
    ctx.full = (1u << n) - 1u;
    ctx.m = p.m;
    ctx.all = env_int("HCLIB_HIP_NQUEENS_SPAWN_ALL", 0);
    ctx.local = env_int("HCLIB_HIP_NQUEENS_LOCAL", 1);
    ctx.blocks = blocks;
    ctx.fin.scopes = (FinishScope *)dmem;
    ctx.fin.next = (uint32_t *)(dmem + jb);
    ctx.fin.cap = (uint32_t)ids;
    ctx.fin.root_value = (unsigned long long *)(ctx.fin.next + 16);
    ctx.hist = hist ? (unsigned long long *)(dmem + jb + 256) : nullptr;
    HX_HIP(hipMemsetAsync(ctx.fin.next, 0, 256 + hb, m.stream));
    PoolView pool;
    HX_TRY(sched_pool(64, (uint32_t)env_int("HCLIB_HIP_NQUEENS_CHUNK", 32), 8, &pool));
    const SchedConfig cfg = sched_config_unseeded("NQUEENS", grid);
    HX_TRY(reset_sched(pool, 1u, false, (uint32_t)grid));
    void (*const kern)(NqCtx, PoolView, SchedGlobals *, SchedConfig) =
        bots ? (hist ? k_nqueens<NqBotsKind<true>> : k_nqueens<NqBotsKind<false>>)
             : (hist ? k_nqueens<NqFlatKind<true>> : k_nqueens<NqFlatKind<false>>);
    SchedGlobals gl;
    float ms = 0;
    HX_TRY(launch_sched((const void *)kern, grid, 64, "hclib_hip_nqueens", [&] {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, m.stream, ctx, pool, m.globals, cfg);
    }, &gl, &ms, "hipLaunchKernelGGL(k_nqueens)"));
    unsigned long long v = 0, h[kNqMaxN + 1] = {};
    if (bots) HX_HIP(hipMemcpy(&v, ctx.fin.root_value, 8, hipMemcpyDeviceToHost));
    if (hist) HX_HIP(hipMemcpy(h, ctx.hist, 8 * (size_t)(n + 1), hipMemcpyDeviceToHost));
    if (env_int("HCLIB_HIP_NQUEENS_DEBUG", 0)) {
        uint32_t used = 0;  // scopes that lived in HBM (opened there or promoted from LDS)
        if (hipMemcpy(&used, ctx.fin.next, 4, hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "nqueens(%d): %u of %llu scope ids taken in HBM (local %d)\n", n, used, p.scopes, ctx.local);
    }
    result->solutions = bots ? v : gl.counters[3];
    result->items = gl.counters[0];
    result->joins = gl.counters[1];
    // the reference's counts: n asyncs per spawning call and one finish each
    // (BOTS); one async per placement that passed ok() (flat: every item but
    // the root)
    result->scopes = bots ? gl.counters[2] : 0;
    result->tasks = bots ? gl.counters[2] * (unsigned long long)n : gl.counters[0] - 1;
    result->chunks_pushed = gl.counters[kCtrPushed];
    result->chunks_stolen = gl.counters[kCtrStolen];
    result->kernel_ms = ms;
    result->busy_frac = busy_frac(gl);
    if (hist)
        for (int i = 0; i <= n; ++i) hist[i] = h[i];
    return HCLIB_HIP_OK;
}
