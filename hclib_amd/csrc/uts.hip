// uts.hip — UTS tree search as a device task kind of the megakernel.
//
// One lane-item = one rng_spawn (test/uts/rng/brg_sha1.c:68-83): the child
// state is a single SHA-1 block compression of parent[20] || i, computed in
// registers. A task entry is a non-leaf node with children left to spawn
// (leaves are counted and never stored). numChildren (test/uts/uts.c:225-274)
// runs on integer threshold tables that the host derives from the
// reference's own libm formula (uts.c:171-222), so the device needs no libm
// and stays bit-exact: n = #{k in 1..100 : thr[depth][k] <= rand}.
// Counting follows UTS.cpp: a node counts when it is generated (each node is
// popped exactly once in the reference), leaves when numChildren <= 0,
// depth = max height.
#include <string.h>

#include <type_traits>
#include <vector>

#include "hx_client.h"
#include "uts_sha1.h"
#include "hx_uts_plan.h"

namespace hx {

// rng_spawn (the device SHA-1, one and several interleaved chains): uts_sha1.h

// --------------------------------------------------------- depth rules
// rule.x: 0 = constant rule.y children; 1 = BIN: rand < rule.y ? m : 0;
//         2 = GEO: threshold table rule.z (128 words, entries 1..100)
// (the host builds them as UtsRule, hx_uts_host.h; the device reads int4)
static_assert(sizeof(UtsRule) == sizeof(int4) && offsetof(UtsRule, x) == offsetof(int4, x) &&
                  offsetof(UtsRule, y) == offsetof(int4, y) && offsetof(UtsRule, z) == offsetof(int4, z) &&
                  offsetof(UtsRule, w) == offsetof(int4, w),
              "UtsRule is uploaded as int4");
static_assert(kUtsSeedMaxLevels == kSeedMaxLevels, "the plan's level bound is the seeding's");
struct UtsCtx {
    uint32_t root[5];
    int root_nc;
    int nrules;
    int stationary;
    int gran;
    int m;
    int shard, nshards, split;
    int hist_levels;
    int lds_tables;  // rules/thr fit the per-wave LDS cache
    uint32_t bin_thr;  // BIN trees: a node has m children iff rand < bin_thr (every depth >= 1)
    int nthr;        // words in thr
    int geo_depth;   // kUtsGeoFixed: depths 1..geo_depth-1 use table 0, deeper nodes are leaves
    // kUtsGeoFixed: table 0's bucket bytes (kUtsBuckets, see uts_nc): per
    // 2^21-wide bucket of rand, the thresholds at or below its start (| 0x80
    // when more than two thresholds fall inside it)
    const uint32_t *nb;
    const int4 *rules;
    const uint32_t *thr;
    unsigned long long *hist;
    const uint32_t *chain;  // FEAT 3 (diagnostic): chain[d] = child index of the traced chain's depth-d node
};

// LDS copies of the rule tables (file scope, so every access is a ds_read:
// a generic pointer to them would compile to flat loads whose waits also
// drain the in-flight global loads).
__shared__ int4 s_rules[kUtsLdsRules];
__shared__ uint32_t s_thr[kUtsLdsThr];

template <int MODE>
__device__ __forceinline__ int uts_nc(const UtsCtx &c, int d, uint32_t r, uint32_t *err) {
    if (MODE == kUtsBin) return r < c.bin_thr ? c.m : 0;
    if (MODE == kUtsGeoFixed) {
        if (d >= c.geo_depth) return 0;
        // bucket of rand: the thresholds at or below its start (n_lo), and
        // the next two compared — exact whenever at most two thresholds fall
        // inside the bucket (thresholds are sorted): n = #{k : thr[k] <= r}.
        // 6-8 VALU and two LDS reads per node instead of 16 compares (and a
        // binary search in 3 of 4 batches at b = 4, where P(n > 16) is 2.3 %)
        const uint32_t e = ((const uint8_t *)(s_thr + 128))[r >> kUtsBucketShift];
        const uint32_t nlo = e & 0x7fu;
        uint32_t n = nlo + (s_thr[nlo + 1] <= r ? 1u : 0u) + (s_thr[nlo + 2] <= r ? 1u : 0u);
        if (e & 0x80u) {
            // a dense bucket (thresholds past ~23 at b = 4, P ~ 0.6 % per
            // node): binary search of the LDS table above n_lo
            int lo = (int)nlo, hi = 100;
            for (int s = 0; s < 7; ++s) {
                int mid = (lo + hi + 1) >> 1;
                if (lo < hi) {
                    if (s_thr[mid] <= r) lo = mid;
                    else hi = mid - 1;
                }
            }
            n = (uint32_t)lo;
        }
        return (int)n;
    }
    constexpr bool LDS = MODE == kUtsRulesLds;
    int ri = d;
    if (d >= c.nrules) {
        if (!c.stationary) {
            dev_error(err, kErrDepthTable);
            return 0;
        }
        ri = c.nrules - 1;
    }
    const int4 rule = LDS ? s_rules[ri] : c.rules[ri];
    if (rule.x == 0) return rule.y;
    if (rule.x == 1) return r < (uint32_t)rule.y ? c.m : 0;
    const int tb = rule.z * 128;
    int lo = 0, hi = 100;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        int mid = (lo + hi + 1) >> 1;
        if (lo < hi) {
            const uint32_t t = LDS ? s_thr[tb + mid] : c.thr[tb + mid];
            if (t <= r) lo = mid;
            else hi = mid - 1;
        }
    }
    return lo;
}

// ring items per wave (CAP) and the pieces a task's children are pushed as:
// BIN trees 1024 / 8 (m <= 8 children keep every batch uniform: the register
// carry); GEO trees 512 by default (16 KiB: 8 waves per CU resident), 256 / 1
// (8 KiB) and 1024 / 8 as measured alternatives (HCLIB_HIP_UTS_RING). On 512
// rings a fixed-shape GEO tree pushes a task's children as ONE range item
// (the residual splits in halves as it is popped): fewer ring writes and a
// one-iteration push loop, T1XL 49.7 -> 37.6 ms, T1L 4.48 -> 4.04, against
// 5 pieces (45.0 / 4.17 at 3, 42.3 / 4.43 at 2); rule-table trees keep 5
// (T4 0.88 -> 2.35 ms at 1, T2 1.37 -> 1.65): profiles/r02/pieces_ab.log
template <int MODE, int CAP>
constexpr int uts_pieces() {
    return CAP >= 1024 ? 8 : (CAP >= 512 ? (MODE == kUtsGeoFixed ? 1 : 5) : 1);
}

// FEAT = 0: plain search; 1: sharded (nshards > 1) and/or per-level histogram;
// 2: diagnostic trace (HCLIB_HIP_UTS_TRACE=1): per depth, the earliest
// s_memrealtime (100 MHz) at which any wave reached it, recorded by a wave
// only when its own deepest depth grows (the level_hist array receives
// these times instead of counts); 3: chain stamps (HCLIB_HIP_UTS_TRACE=2,
// BIN trees): one given root-to-leaf chain (HCLIB_HIP_UTS_CHAIN, a file from
// scripts/critpath/uts_chain.c) is followed through the search — its nodes
// carry a flag in the height word's top bit — and level_hist[4d], [4d+1]
// receive when its depth-d node ran and where (worker, narrow loop or not,
// batch fill, dual batch), [4d+2], [4d+3] when it was given away and taken
// if it changed hands (trace_item)
template <int MODE, int FEAT, int CAP = (MODE == kUtsBin ? 1024 : 512)>
struct UtsKind {
    // template = the node {state[5], height}; an item = its children [k, kend)
    static constexpr int kTmplWords = 6;
    static constexpr int kPieces = uts_pieces<MODE, CAP>();
    static constexpr int kWords = 8;
    // every side effect (histogram atomics, trace stamps) is guarded by
    // `counted` / lane 0, so invalid lanes may run the body: branch-free
    // batches for every variant
    static constexpr bool kPure = true;
    static constexpr bool kBoundedChildren = true;  // <= 100 (the root goes through roots())
    using Ctx = UtsCtx;
    // BIN trees: a node has m children or none (the narrow loop's fast path;
    // hx_sched.h KindFixedChildren). Sharded BIN searches drop foreign nodes
    // (0 children) at the split: still none-or-m.
    static constexpr bool kFixedChildren = MODE == kUtsBin;
    __device__ static uint32_t fixed_children(const Ctx &c) { return c.m > 0 ? (uint32_t)c.m : 0u; }
    struct Acc {
        // per lane: at most one node per batch, so 32 bits last 4G batches
        uint32_t nodes = 0, leaves = 0;
        uint32_t maxd = 0;
        uint32_t trace_seen = 0;  // FEAT 2: the deepest depth this wave has stamped
        uint32_t mode = 0;        // FEAT 2: 1 while the scheduler runs the narrow loop (hx_sched.h)
        uint32_t wid = 0;         // FEAT 2: this worker's id (hx_sched.h acc_set_wid)
        // the wave's totals go into its exit record (hx_sched.h Kind concept)
        __device__ void totals(unsigned long long (&c)[8], unsigned long long (&m)[4]) {
            c[0] = wave_sum((unsigned long long)nodes);
            c[1] = wave_sum((unsigned long long)leaves);
            m[0] = (unsigned long long)wave_max(maxd);
        }
    };

    // cross-GPU sharing (GLOBAL launches): a task may move to another rank
    // once its children lie below the shard split (the levels above it are
    // expanded by every rank and counted by shard 0)
    __device__ static bool movable(const Ctx &c, const uint32_t *tmpl) {
        return c.nshards <= 1 || (int)tmpl[5] >= c.split;
    }

    __device__ static int roots(const Ctx &c, Acc &acc, uint32_t *tmpl) {
        // the root node (height 0) is counted once, by shard 0
        if (lane_id() == 0 && c.shard == 0) {
            acc.nodes += 1;
            if (c.root_nc <= 0) acc.leaves += 1;
            if (c.hist && c.hist_levels > 0) atomicAdd(&c.hist[0], 1ull);
        }
        for (int k = 0; k < 5; ++k) tmpl[k] = c.root[k];
        tmpl[5] = FEAT == 3 ? 0x80000000u : 0u;  // FEAT 3: the root heads the traced chain
        return c.root_nc;
    }

    // everything after the spawn: counting, numChildren, the child template
    // (F: the FEAT whose side paths run; the shard filter from F = 1 on)
    template <int F = FEAT>
    __device__ static __forceinline__ int finish(const Ctx &c, Acc &acc, const uint32_t *t, const uint32_t *ch,
                                                 uint32_t *child, uint32_t *err, bool valid) {
        const int h1 = (int)(F == 3 ? t[5] & 0x7fffffffu : t[5]) + 1;
        bool counted = valid;
        // (the worker loop filters only where the seeding cannot reach the
        // split; a wave-uniform branch around this was no faster: the FEAT
        // = 1 body's cost is its code generation, profiles/r06/shard_big_a.log)
        if (F && c.nshards > 1) {
            if (h1 == c.split && (ch[0] % (uint32_t)c.nshards) != (uint32_t)c.shard) return 0;
            if (h1 < c.split && c.shard != 0) counted = false;
        }
        // an invalid lane's template is stale ring bytes: look it up at depth 1
        // so it can neither index past the rule table nor raise kErrDepthTable
        int nc = uts_nc<MODE>(c, valid ? h1 : 1, ch[4] & 0x7fffffffu, err);
        // branch-free counting (invalid lanes of a pure batch count nothing)
        acc.nodes += counted ? 1u : 0u;
        acc.leaves += (counted && nc <= 0) ? 1u : 0u;
        acc.maxd = (counted && (uint32_t)h1 > acc.maxd) ? (uint32_t)h1 : acc.maxd;
        if (F == 1 && counted && c.hist && h1 < c.hist_levels) atomicAdd(&c.hist[h1], 1ull);
        if (F == 2 && c.hist) {
            const uint32_t dm = wave_max(counted ? (uint32_t)h1 : 0u);
            if (dm > acc.trace_seen) {
                acc.trace_seen = dm;
                // stamp = time (low 46 bits: 8 days of 100 MHz ticks, so a box up
                // longer does not push every stamp past the 0xff.. fill) << 17 |
                // worker (16 bits) << 1 | reached in the narrow loop (1) or not
                if (lane_id() == 0 && (int)dm < c.hist_levels)
                    __hip_atomic_fetch_min(&c.hist[dm],
                                           ((__builtin_amdgcn_s_memrealtime() & 0x3fffffffffffull) << 17) |
                                               ((unsigned long long)(acc.wid & 0xffffu) << 1) | acc.mode,
                                           __ATOMIC_RELAXED, HX_AGENT);
            }
        }
        if (!valid) nc = 0;
        child[0] = ch[0];
        child[1] = ch[1];
        child[2] = ch[2];
        child[3] = ch[3];
        child[4] = ch[4];
        child[5] = (uint32_t)h1;
        return nc;
    }

    // FEAT 3: the traced chain's next child index, loaded before the SHA-1
    // by lanes whose node is on the chain (its latency hides behind it)
    __device__ static __forceinline__ uint32_t chain_next(const Ctx &c, const uint32_t *t, bool valid) {
        uint32_t kc = 0xffffffffu;
        if (FEAT == 3 && valid && (t[5] >> 31)) kc = c.chain[(t[5] & 0x7fffffffu) + 1u];
        return kc;
    }
    __device__ static __forceinline__ void chain_stamp(const Ctx &c, const Acc &acc, uint32_t *child, bool on,
                                                       bool valid, uint32_t dual) {
        if constexpr (FEAT == 3) {
            const uint32_t fill = (uint32_t)__builtin_popcountll(__ballot(valid));
            if (on) {
                const uint32_t d = child[5];
                child[5] = d | 0x80000000u;
                c.hist[4 * d] = __builtin_amdgcn_s_memrealtime();
                c.hist[4 * d + 1] = (unsigned long long)((acc.wid & 0xffffu) | (acc.mode << 16) | (dual << 17) |
                                                         (fill << 20));
            }
        }
    }

    // FEAT 3: an item {template, k, kend} holding the traced chain's next
    // node changes hands (hx_sched.h kind_trace_item): level_hist[4d + 2] =
    // when it was given away, [4d + 3] = when it was taken (bit 63: through
    // a sibling's LDS inbox rather than the HBM deques)
    __device__ static void trace_item(const Ctx &c, const uint32_t *w, bool valid, uint32_t ev, bool via_inbox) {
        if constexpr (FEAT == 3) {
            if (valid && (w[5] >> 31)) {
                const uint32_t d = (w[5] & 0x7fffffffu) + 1u;
                const uint32_t kc = c.chain[d];
                if (kc >= w[kWords - 2] && kc < w[kWords - 1])
                    c.hist[4 * d + ev] = __builtin_amdgcn_s_memrealtime() | (via_inbox ? 1ull << 63 : 0ull);
            }
        }
    }

    __device__ static int process(const Ctx &c, Acc &acc, const uint32_t *t, uint32_t k,
                                  uint32_t *child, uint32_t *err, bool valid) {
        uint32_t ch[5];
        const uint32_t kc = chain_next(c, t, valid);
        rng_spawn_dev(t, k, ch);
        for (int g = 1; g < c.gran; ++g) rng_spawn_dev(t, k, ch);  // -g: repeated spawns
        const int nc = finish(c, acc, t, ch, child, err, valid);
        chain_stamp(c, acc, child, k == kc, valid, 0u);
        return nc;
    }

    // the fixed-size narrow loop's form (hx_sched.h narrow_loop_fixed; FEAT 0,
    // where a node counts iff its lane is valid): finish<0> without the node
    // and leaf counts, which the loop sums per level as wave-uniform values
    // (nodes = the carry, leaves = the carry less the spawning lanes)
    // Returns whether the node spawns (its m children; the loop runs only
    // with m > 0, so the test is the threshold alone)
    static constexpr bool kBulkCount = FEAT == 0;
    __device__ static __forceinline__ bool process_bulk(const Ctx &c, Acc &acc, const uint32_t *t, uint32_t k,
                                                        uint32_t *child, uint32_t *err, bool valid) {
        static_assert(MODE == kUtsBin, "the fixed-size narrow loop runs BIN trees");
        uint32_t ch[5];
        rng_spawn_dev(t, k, ch);
        for (int g = 1; g < c.gran; ++g) rng_spawn_dev(t, k, ch);
        const int h1 = (int)t[5] + 1;
        acc.maxd = (valid && (uint32_t)h1 > acc.maxd) ? (uint32_t)h1 : acc.maxd;
        for (int i = 0; i < 5; ++i) child[i] = ch[i];
        child[5] = (uint32_t)h1;
        return valid && (ch[4] & 0x7fffffffu) < c.bin_thr;
    }
    // (lane 0 holds a wave's bulk counts: at most the tree's nodes, < 2^32
    // for every published tree)
    __device__ static void count_bulk(Acc &acc, uint32_t nodes, uint32_t leaves) {
        if (lane_id() == 0) {
            acc.nodes += nodes;
            acc.leaves += leaves;
        }
    }

    // the breadth-first seeding's slots (hx_sched.h seed_levels) run with the
    // shard filter and the top levels' counting rule whatever FEAT is: a
    // seeded shard's levels reach past its split depth (the host launches
    // FEAT = 0 only then), so its work-stealing loop, the plain kernel of a
    // whole-tree search, never meets a node at or above the split
    __device__ static int seed_process(const Ctx &c, Acc &acc, const uint32_t *t, uint32_t k, uint32_t *child,
                                       uint32_t *err, bool valid) {
        uint32_t ch[5];
        rng_spawn_dev(t, k, ch);
        for (int g = 1; g < c.gran; ++g) rng_spawn_dev(t, k, ch);
        return finish<FEAT == 0 ? 1 : FEAT>(c, acc, t, ch, child, err, valid);
    }

    // two nodes per lane (dual batches of the megakernel, hx_sched.h): the two
    // SHA-1 chains interleaved instruction by instruction (uts_sha1.h)
    __device__ static void process2(const Ctx &c, Acc &acc, const uint32_t *tA, uint32_t kA, uint32_t *childA,
                                    int &ncA, const uint32_t *tB, uint32_t kB, uint32_t *childB, int &ncB,
                                    uint32_t *err, bool validB) {
        uint32_t chA[5], chB[5];
        const uint32_t kcA = chain_next(c, tA, true), kcB = chain_next(c, tB, validB);
        const uint32_t *pp[2] = {tA, tB};
        const uint32_t ii[2] = {kA, kB};
        uint32_t *oo[2] = {chA, chB};
        rng_spawn_n<2>(pp, ii, oo);
        for (int g = 1; g < c.gran; ++g) rng_spawn_n<2>(pp, ii, oo);  // -g: repeated spawns
        ncA = finish(c, acc, tA, chA, childA, err, true);
        ncB = finish(c, acc, tB, chB, childB, err, validB);
        chain_stamp(c, acc, childA, kA == kcA, true, 1u);
        chain_stamp(c, acc, childB, kB == kcB, validB, 1u);
    }
};

// GLOBAL: a sharded launch that shares work with the other ranks
// (hclib_hip_global_attach; hx_sched.h GlobalView). WPG: worker waves per
// workgroup, handing work to idle siblings through LDS inboxes (hx_sched.h
// Inbox) before the HBM deques. Such a workgroup (not GLOBAL) may be launched
// with 64 more threads: wave WPG is then its hand-off wave (hx_sched.h
// comm_wave), which runs no task and is no worker of the grid.
template <int MODE, int FEAT, int CAP = (MODE == kUtsBin ? 1024 : 512), bool GLOBAL = false, int WPG = 1>
__global__ __launch_bounds__(64 * uts_block_waves(WPG, GLOBAL)) void k_uts_search(UtsCtx ctx, PoolView pool,
                                                                                  SchedGlobals *g, SchedConfig cfg) {
    constexpr int kUtsCap = CAP;
    constexpr bool kComm = uts_block_waves(WPG, GLOBAL) > WPG;
    using K = UtsKind<MODE, FEAT, CAP>;
    __shared__ WaveStack<K, kUtsCap> st[WPG];
    WgBoxes<K, WPG> &bx = wg_static_boxes<K, WPG>();  // the workgroup's one static LDS object
    static_assert(sizeof(st) + sizeof(WgBoxes<K, WPG>) + (MODE == kUtsBin ? 0 : sizeof(s_rules) + sizeof(s_thr)) <= 160 * 1024,
                  "a workgroup's rings, boxes and rule tables fit a CU's LDS");
    Inbox<K> *ib = bx.ib;
    const uint32_t wave = WPG > 1 ? threadIdx.x / 64 : 0;
    const uint32_t worker = blockIdx.x * WPG + wave;
    if (WPG > 1) {
        if (threadIdx.x < WPG) {
            ib[threadIdx.x].state = 0;
            ib[threadIdx.x].idle = 0;
        }
    }
    if constexpr (WPG > 1) {
        if (threadIdx.x < kOutboxes) bx.out[threadIdx.x].state = 0;
        if (threadIdx.x < 6) bx.ctl.cnt[threadIdx.x] = 0;
        if (threadIdx.x == 0) {
            // the outbox has users only where the launch brought the wave
            bx.ctl.on = kComm && blockDim.x > 64u * WPG ? (cfg.narrow_shed >> 16) & 7u : 0u;
            bx.ctl.left = 0;
        }
    }
    if (MODE == kUtsGeoFixed) {
        // table 0 and its bucket bytes in LDS (uts_nc)
        for (int i = threadIdx.x; i < 128; i += 64 * WPG) s_thr[i] = ctx.thr[i];
        for (int i = threadIdx.x; i < kUtsBuckets / 4; i += 64 * WPG) s_thr[128 + i] = ctx.nb[i];
    }
    if (MODE == kUtsRulesLds) {
        // the per-node rule lookup becomes LDS-latency (no dependent HBM/L2 loads)
        for (int i = threadIdx.x; i < ctx.nrules; i += 64 * WPG) s_rules[i] = ctx.rules[i];
        for (int i = threadIdx.x; i < ctx.nthr; i += 64 * WPG) s_thr[i] = ctx.thr[i];
    }
    __syncthreads();
    if constexpr (kComm) {
        if (wave == (uint32_t)WPG) {
            comm_wave<K, kUtsCap, WPG>(ctx, pool, g, cfg, bx, st[0]);
            return;
        }
    }
    run_worker<K, kUtsCap, GLOBAL, WPG>(ctx, pool, g, cfg, st[wave], worker == 0, ib, wave, worker);
    if constexpr (kComm) {
        if (threadIdx.x % 64 == 0)
            __hip_atomic_fetch_add((hx_lds_u32 *)&bx.ctl.left, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// build_tables, its error (if any) reported through set_error
static int uts_tables(const hclib_hip_uts_params_t &p, UtsTables &T) {
    std::string err;
    const int rc = build_tables(p, T, err);
    if (rc != HCLIB_HIP_OK) set_error("%s", err.c_str());
    return rc;
}

}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_uts_num_children_host(const hclib_hip_uts_params_t *params, int height,
                                               const uint32_t st[5]) {
    // tables are pure functions of the parameters: cache the last set
    static hclib_hip_uts_params_t last_p;
    static UtsTables T;
    static bool have = false;
    if (!have || memcmp(&last_p, params, sizeof(last_p)) != 0) {
        have = false;
        if (uts_tables(*params, T) != HCLIB_HIP_OK) return -1;
        last_p = *params;
        have = true;
    }
    if (height == 0) return T.root_nc;
    return host_nc(*params, T, height, st[4] & 0x7fffffffu);
}

// Host check of the bucketed numChildren lookup (no GPU needed): for the
// tree's first threshold table, the bucket method against the exact count
// #{k : thr[k] <= r} at every threshold +-3, every bucket edge +-1 and
// `nrandom` splitmix values of rand. Returns the mismatches (0) or a negative
// error; *checked receives the values compared.
extern "C" int hclib_hip_uts_bucket_check(const hclib_hip_uts_params_t *params, uint64_t nrandom,
                                          uint64_t *checked) {
    if (!params) {
        set_error("hclib_hip_uts_bucket_check: NULL params");
        return HCLIB_HIP_EINVAL;
    }
    UtsTables T;
    if (uts_tables(*params, T) != HCLIB_HIP_OK) return HCLIB_HIP_EINVAL;
    if (T.thr.size() < 128) {  // no threshold table (BIN or constant rules)
        if (checked) *checked = 0;
        return 0;
    }
    const uint32_t *t0 = T.thr.data();
    uint8_t nb[kUtsBuckets];
    build_buckets(t0, nb);
    uint64_t n = 0;
    int bad = 0;
    auto one = [&](int64_t v) {
        if (v < 0 || v > 0x7fffffffll) return;
        const uint32_t r = (uint32_t)v;
        int exact = 0;
        for (int k = 1; k <= 100; ++k) exact += t0[k] <= r;
        bad += bucket_nc(t0, nb, r) != exact;
        ++n;
    };
    for (int k = 1; k <= 100; ++k)
        if (t0[k] != 0x80000000u)
            for (int d = -3; d <= 3; ++d) one((int64_t)t0[k] + d);
    for (int b = 0; b <= kUtsBuckets; ++b)
        for (int d = -1; d <= 1; ++d) one(((int64_t)b << kUtsBucketShift) + d);
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (uint64_t i = 0; i < nrandom; ++i) {
        x += 0x9e3779b97f4a7c15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        one((int64_t)((z ^ (z >> 31)) & 0x7fffffffull));
    }
    if (checked) *checked = n;
    return bad;
}

static thread_local hclib_hip_uts_launch_t g_last_launch{-1, 0, 0, 0, 0, 0, 0, 0, 0};

extern "C" int hclib_hip_uts_last_launch(hclib_hip_uts_launch_t *out) {
    if (!out) {
        set_error("hclib_hip_uts_last_launch: null output");
        return HCLIB_HIP_EINVAL;
    }
    *out = g_last_launch;
    return g_last_launch.mode < 0 ? HCLIB_HIP_EINVAL : HCLIB_HIP_OK;
}

// HCLIB_HIP_<NAME> into UtsKnobs, once per search
static UtsKnobs uts_knobs() {
    UtsKnobs k;
    k.grid = env_int("HCLIB_HIP_GRID", k.grid);
    k.waves_per_cu = env_int("HCLIB_HIP_WAVES_PER_CU", k.waves_per_cu);
    k.wpg = env_int("HCLIB_HIP_WPG", k.wpg);
    k.uts_ring = env_int("HCLIB_HIP_UTS_RING", k.uts_ring);
    k.uts_geo_fixed = env_int("HCLIB_HIP_UTS_GEO_FIXED", k.uts_geo_fixed);
    k.uts_seed = env_int("HCLIB_HIP_UTS_SEED", k.uts_seed);
    k.uts_trace = env_int("HCLIB_HIP_UTS_TRACE", k.uts_trace);
    k.uts_dual = env_int("HCLIB_HIP_UTS_DUAL", k.uts_dual);
    k.deques = env_int("HCLIB_HIP_DEQUES", k.deques);
    k.deque_cap = env_int("HCLIB_HIP_DEQUE_CAP", k.deque_cap);
    k.chunk = env_int("HCLIB_HIP_CHUNK", k.chunk);
    k.spill_hi = env_int("HCLIB_HIP_SPILL_HI", k.spill_hi);
    k.spill_lo = env_int("HCLIB_HIP_SPILL_LO", k.spill_lo);
    k.seed_per_wave = env_int("HCLIB_HIP_SEED_PER_WAVE", k.seed_per_wave);
    k.seed_per_wave_set = getenv("HCLIB_HIP_SEED_PER_WAVE") != nullptr;
    k.seed_levels = env_int("HCLIB_HIP_SEED_LEVELS", k.seed_levels);
    k.seed_solo = env_int("HCLIB_HIP_SEED_SOLO", k.seed_solo);
    k.hunger = env_int("HCLIB_HIP_HUNGER", k.hunger);
    k.spin_limit_ms = env_int("HCLIB_HIP_SPIN_LIMIT_MS", k.spin_limit_ms);
    k.stamps = env_int("HCLIB_HIP_STAMPS", k.stamps);
    k.carry = env_int("HCLIB_HIP_CARRY", k.carry);
    k.backoff = env_int("HCLIB_HIP_BACKOFF", k.backoff);
    k.defer = env_int("HCLIB_HIP_DEFER", k.defer);
    k.spills_per_batch = env_int("HCLIB_HIP_SPILLS_PER_BATCH", k.spills_per_batch);
    k.narrow_shed = env_int("HCLIB_HIP_NARROW_SHED", k.narrow_shed);
    k.narrow_shed_sibs = env_int("HCLIB_HIP_NARROW_SHED_SIBS", k.narrow_shed_sibs);
    k.uts_comm = env_int("HCLIB_HIP_UTS_COMM", k.uts_comm);
    return k;
}

// The kernel of a plan: every k_uts_search specialisation the library holds
// is a row here, and nothing else instantiates one. Null: the plan asks for
// a combination that is not built (uts_plan never does).
typedef void (*uts_kernel_t)(UtsCtx, PoolView, SchedGlobals *, SchedConfig);
static uts_kernel_t uts_kernel(int mode, int feat, int cap, bool global, int wpg) {
#define HX_UTS_KERNEL(MODE, FEAT, CAP, GLOBAL, WPG) {MODE, FEAT, CAP, GLOBAL, WPG, k_uts_search<MODE, FEAT, CAP, GLOBAL, WPG>}
    static const struct {
        int mode, feat, cap;
        bool global;
        int wpg;
        uts_kernel_t kern;
    } kernels[] = {
        // the plain and the filtering / histogram kernel of each lookup mode
        HX_UTS_KERNEL(kUtsRulesGlobal, 0, 512, false, 1), HX_UTS_KERNEL(kUtsRulesGlobal, 1, 512, false, 1),
        HX_UTS_KERNEL(kUtsRulesLds, 0, 512, false, 1), HX_UTS_KERNEL(kUtsRulesLds, 1, 512, false, 1),
        HX_UTS_KERNEL(kUtsBin, 0, 1024, false, 1), HX_UTS_KERNEL(kUtsBin, 1, 1024, false, 1),
        HX_UTS_KERNEL(kUtsGeoFixed, 0, 512, false, 1), HX_UTS_KERNEL(kUtsGeoFixed, 1, 512, false, 1),
        // diagnostics on BIN trees: chain stamps, depth trace
        HX_UTS_KERNEL(kUtsBin, 3, 1024, false, 1), HX_UTS_KERNEL(kUtsBin, 2, 1024, false, 1),
        // sharded launches that share work across ranks
        HX_UTS_KERNEL(kUtsRulesGlobal, 1, 512, true, 1), HX_UTS_KERNEL(kUtsRulesLds, 1, 512, true, 1),
        HX_UTS_KERNEL(kUtsBin, 1, 1024, true, 1), HX_UTS_KERNEL(kUtsGeoFixed, 1, 512, true, 1),
        // ring-size variants of the fixed-shape GEO search: the plain kernel only
        HX_UTS_KERNEL(kUtsGeoFixed, 0, 256, false, 1), HX_UTS_KERNEL(kUtsGeoFixed, 0, 1024, false, 1),
        // BIN trees in workgroups of 2 and 4 worker waves
        HX_UTS_KERNEL(kUtsBin, 3, 1024, false, 2), HX_UTS_KERNEL(kUtsBin, 3, 1024, false, 4),
        HX_UTS_KERNEL(kUtsBin, 1, 1024, false, 2), HX_UTS_KERNEL(kUtsBin, 0, 1024, false, 2),
        HX_UTS_KERNEL(kUtsBin, 1, 1024, false, 4), HX_UTS_KERNEL(kUtsBin, 0, 1024, false, 4),
    };
#undef HX_UTS_KERNEL
    for (const auto &k : kernels)
        if (k.mode == mode && k.feat == feat && k.cap == cap && k.global == global && k.wpg == wpg) return k.kern;
    return nullptr;
}

extern "C" int hclib_hip_uts_search(const hclib_hip_uts_params_t *params, int shard, int nshards,
                                    int split_depth, hclib_hip_uts_result_t *result,
                                    uint64_t *level_hist, int max_levels) {
    const char *who = "hclib_hip_uts_search";
    const UtsKnobs knobs = uts_knobs();
    if (!params || !result || nshards < 1 || shard < 0 || shard >= nshards || max_levels < 0 ||
        max_levels > (knobs.uts_trace == 2 ? 4 * 65536 : 65536) || (nshards > 1 && split_depth < 1)) {
        set_error("hclib_hip_uts_search: invalid arguments");
        return HCLIB_HIP_EINVAL;
    }
    {
        // (a knob the plan would refuse, refused before the tables' arena is reserved)
        std::string why;
        if (!uts_comm_valid(knobs.uts_comm, why)) {
            set_error("%s", why.c_str());
            return HCLIB_HIP_EINVAL;
        }
    }
    HX_TRY(ensure_device());
    Module &m = mod();
    // The rule / threshold tables are pure functions of the parameters and
    // cost ~1 ms of libm on the host for a GEO tree (100 threshold searches
    // per depth): the last set and its device copy are kept for the next
    // search of the same tree (every call returns with the stream drained, so
    // no launch still reads them when they are replaced). The host copy is
    // valid while the device copy's arena is: Module::uts_tables_cached goes
    // with the arena at hclib_hip_finalize
    static struct {
        hclib_hip_uts_params_t p;
        UtsTables T;
    } tab;
    const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    if (!m.uts_tables_cached || memcmp(&tab.p, params, sizeof(tab.p)) != 0) {
        m.uts_tables_cached = false;
        HX_TRY(uts_tables(*params, tab.T));
        const size_t rb = tab.T.rules.size() * sizeof(int4), tb = tab.T.thr.size() * 4;
        char *dp = nullptr;
        HX_TRY(arena_reserve(kArenaUtsTables, pad(rb) + pad(tb) + kUtsBuckets + 256, who, (void **)&dp));
        HX_HIP(hipMemcpy(dp, tab.T.rules.data(), rb, hipMemcpyHostToDevice));
        HX_HIP(hipMemcpy(dp + pad(rb), tab.T.thr.data(), tb, hipMemcpyHostToDevice));
        uint8_t nb[kUtsBuckets] = {0};
        if (tab.T.thr.size() >= 128) build_buckets(tab.T.thr.data(), nb);
        HX_HIP(hipMemcpy(dp + pad(rb) + pad(tb), nb, kUtsBuckets, hipMemcpyHostToDevice));
        tab.p = *params;
        m.uts_tables_cached = true;
    }
    const UtsTables &T = tab.T;
    char *d_tab = (char *)m.arenas[kArenaUtsTables].mem;

    std::string why;
    const UtsPlan plan = uts_plan(*params, T, m.num_cus, shard, nshards, split_depth, max_levels,
                                  m.gview.hdr != nullptr, knobs, why);
    if (plan.status != HCLIB_HIP_OK) {
        set_error("%s", why.c_str());
        return plan.status;
    }
    const uts_kernel_t kern = uts_kernel(plan.mode, plan.feat, plan.ring, plan.global, plan.wpg);
    if (!kern) {
        set_error("%s: no kernel for mode %d, feat %d, ring %d, global %d, %d waves per workgroup", who, plan.mode,
                  plan.feat, plan.ring, (int)plan.global, plan.wpg);
        return HCLIB_HIP_EINVAL;
    }

    // the optional per-level histogram (a trace receives its stamps there)
    const size_t hb = (size_t)max_levels * 8;
    DevBuf hist_buf, chain_buf;
    if (max_levels) HX_TRY(hist_buf.alloc(hb, who));
    unsigned long long *d_hist = (unsigned long long *)hist_buf.p;
    if (max_levels) HX_HIP(hipMemsetAsync(d_hist, plan.feat >= 2 ? 0xff : 0, hb, m.stream));
    // FEAT 3 (diagnostic): the chain to follow, k_1..k_D of scripts/critpath/uts_chain.c
    uint32_t *d_chain = nullptr;
    if (plan.feat == 3) {
        std::vector<uint32_t> chain;
        const char *path = getenv("HCLIB_HIP_UTS_CHAIN");
        if (FILE *f = path ? fopen(path, "rb") : nullptr) {
            uint32_t w;
            while (fread(&w, 4, 1, f) == 1) chain.push_back(w);
            fclose(f);
        }
        if (chain.empty() || chain[0] + 1 != chain.size() || (size_t)max_levels < 4 * chain.size()) {
            set_error("hclib_hip_uts_search: chain trace needs HCLIB_HIP_UTS_CHAIN and max_levels >= 4 (D + 1)");
            return HCLIB_HIP_EINVAL;
        }
        HX_TRY(chain_buf.alloc(chain.size() * 4, who));
        d_chain = (uint32_t *)chain_buf.p;
        HX_HIP(hipMemcpy(d_chain, chain.data(), chain.size() * 4, hipMemcpyHostToDevice));
    }

    UtsCtx ctx;
    memcpy(ctx.root, T.root, sizeof(ctx.root));
    ctx.root_nc = T.root_nc;
    ctx.nrules = (int)T.rules.size();
    ctx.stationary = T.stationary;
    ctx.gran = params->compute_gran < 1 ? 1 : params->compute_gran;
    ctx.m = bin_rule_m(*params);  // read by BIN rules only (BIN and HYBRID trees), capped at 100
    ctx.shard = shard;
    ctx.nshards = nshards;
    ctx.split = split_depth;
    ctx.hist_levels = max_levels;
    ctx.lds_tables = plan.lds_tables;
    ctx.bin_thr = plan.bin_thr;
    ctx.nthr = (int)T.thr.size();
    ctx.geo_depth = plan.geo_depth;
    ctx.rules = (const int4 *)d_tab;
    ctx.thr = (const uint32_t *)(d_tab + pad(T.rules.size() * sizeof(int4)));
    ctx.nb = (const uint32_t *)((const char *)ctx.thr + pad(T.thr.size() * 4));
    ctx.hist = max_levels ? d_hist : nullptr;
    ctx.chain = d_chain;

    PoolView pool;
    HX_TRY(make_pool(plan.nq, plan.deque_cap, plan.chunk, UtsKind<kUtsBin, 0>::kWords, &pool));
    SchedConfig cfg;
    cfg.spill_hi = plan.spill_hi;
    cfg.spill_lo = plan.spill_lo;
    cfg.spin_limit = plan.spin_limit;
    cfg.nwaves = plan.nwaves;
    cfg.stamps = plan.stamps;
    cfg.hunger = plan.hunger;
    cfg.backoff = plan.backoff;
    cfg.carry = plan.carry;
    cfg.defer = plan.defer;
    cfg.dual = plan.dual;
    cfg.spills = plan.spills;
    cfg.hunger_init_full = plan.hunger_init_full;
    cfg.narrow_shed = plan.narrow_shed | plan.comm << 16;
    SeedCfg seed{plan.seed_target, plan.seed_max_levels, (uint32_t)UtsKind<kUtsBin, 0>::kWords, plan.seed_min_levels};
    seed.solo_cap = plan.seed_solo_cap;
    HX_TRY(reset_sched(pool, 1, plan.global, (uint32_t)plan.grid, seed.target ? &seed : nullptr));
    g_last_launch = plan.launch;
    SchedGlobals gl;
    float ms = 0;
    // (the hand-off waves are in plan.block, not in the grid: they hold no
    // work, have no exit record and are no wave of SchedConfig::nwaves)
    m.comm_wpg = plan.comm ? plan.wpg : 0;
    const int rc = launch_sched((const void *)kern, plan.grid / plan.wpg, plan.block, who, [&] {
        hipLaunchKernelGGL(kern, dim3(plan.grid / plan.wpg), dim3(plan.block), 0, m.stream, ctx, pool, m.globals, cfg);
    }, &gl, &ms);
    if (rc != HCLIB_HIP_OK) return rc;
    if (max_levels) {
        std::vector<unsigned long long> h(max_levels);
        HX_HIP(hipMemcpy(h.data(), d_hist, hb, hipMemcpyDeviceToHost));
        for (int i = 0; i < max_levels; ++i) level_hist[i] = h[i];
    }
    result->nodes = gl.counters[0];
    result->leaves = gl.counters[1];
    result->max_depth = gl.maxes[0];
    result->batches = gl.counters[kCtrBatches];
    result->chunks_pushed = gl.counters[kCtrPushed];
    result->chunks_stolen = gl.counters[kCtrStolen];
    result->kernel_ms = ms;
    result->busy_frac = busy_frac(gl);
    // s_memtime ticks at the shader clock, calibrated against the 100 MHz
    // s_memrealtime over the same wave lifetimes
    const double busy = (double)gl.counters[kCtrBusyCycles];
    const double mhz = gl.counters[kCtrRealTicks]
                           ? 100.0 * (double)gl.counters[kCtrClockTicks] / (double)gl.counters[kCtrRealTicks]
                           : 2400.0;
    result->us_per_batch = gl.counters[kCtrBatches] ? busy / gl.counters[kCtrBatches] / mhz : 0.0;
    return HCLIB_HIP_OK;
}
