// Every form of the finish-scope protocol (include/hclib_hip/hx_finish.h)
// against a serial model of the scope tree.
//
// The model: a seeded fork-join tree built on the host. Every node is a scope
// of `count` tasks; a task is a leaf with a value or the opener of a child
// scope. A scope's continuation word is its node index, its continuation is
//     cont(cw, sum) = (3 sum + 0x9E3779B1 cw + 1) mod 2^56
// (not PassSum: a wrong word or a wrong sum changes every value above it), and
// every run of a continuation counts fired[cw] and stores seen[cw] = sum. The
// host evaluates the tree bottom-up mod 2^56; after each launch fired == 1 and
// seen == the model's sum for every scope, the root value, the number of
// continuations the lanes report, the error word, the arena's allocation
// count and the arena's contents (every allocated id one distinct scope,
// closed, with the model's sum, its parent an HBM scope) must all agree.
//
//  A. one wave, a deterministic driver over a task list in global memory
//     (depth first and breadth first), the five forms:
//       1 finish_open / finish_check_out
//       2 finish_open with per-wave id blocks / finish_check_out
//       3 finish_open / finish_issue, finish_resolve a batch later, finish_drain
//       4 finish_open_local<N> / finish_check_out_local (N = 4 and 64), with
//         finish_promote of a seeded subset of the pending items under
//         divergent control flow
//       5 as 4 with the first HBM step in flight (q), resolved per batch
//  B. many waves, two kernels: one-wave workgroups build LDS scopes, check
//     part of the leaves out locally and promote the rest into {scope, value}
//     records; a second kernel of 256-thread workgroups checks the records
//     out (finish_check_out), the all-HBM continuations run there. Plus a
//     contention case: K pre-opened scopes of count 255 checked out by
//     255 K lanes at once, half of them carrying at almost every step.
//  C. the scheduler's export path: one user kind walks the tree through
//     run_worker (the launch glue of hclib::hip::run_tasks around a kernel
//     that initialises the kind's LocalScopes), with export_item / drain hooks.
//  Limits: counts 0 / 255 / 256, arena exhaustion in finish_open (with a
//     guard region) and in finish_promote (and the round it must close).
//
// No loop waits for another wave and every loop is bounded by a length the
// host knows: a wrong protocol gives wrong numbers, not a hang.
// `--plan` prints what every launch covers without touching a GPU;
// `--no-sched` skips part C. Prints "Check results: OK"
// (tests/test_finish_forms_gpu.py).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "hclib_hip_cpp.h"

constexpr uint32_t kNone = 0xffffffffu;
constexpr unsigned long long kMask = hx::kScopeSumMask;

// ---------------------------------------------------------------- the model
static inline bool is_lds_id(uint32_t s) { return s != hx::kScopeRoot && (s & hx::kScopeLds); }
static inline unsigned long long model_cont(uint32_t cw, unsigned long long sum) {
    return (3ull * sum + 0x9E3779B1ull * cw + 1ull) & kMask;
}

struct Rng {
    uint64_t s;
    uint64_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        uint64_t x = s;
        x ^= x >> 33;
        x *= 0xff51afd7ed558ccdull;
        x ^= x >> 33;
        return x;
    }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct Forest {
    std::vector<uint32_t> count, first, parent;  // per node (parent: a node, or kNone)
    std::vector<uint32_t> tchild, tnode;         // per task: the node it opens (kNone: a leaf), its own node
    std::vector<unsigned long long> tval;        // per task: a leaf's value (unmasked)
    std::vector<unsigned long long> sum, value;  // the model: what each continuation sees / returns
    uint32_t nodes() const { return (uint32_t)count.size(); }
    uint32_t tasks() const { return (uint32_t)tchild.size(); }

    static unsigned long long random_value(Rng &r) {
        switch (r.below(8)) {
        case 0: return r.below(1000);
        case 1: return r.next();                                       // bits above 55 set: must be masked
        case 2: return (1ull << 55) | (r.next() & (kMask >> 1));        // carries with another of its kind
        case 3: return kMask;
        case 4: return (0xABull << 56) | r.below(1u << 20);
        default: return (r.next() & kMask) >> r.below(40);
        }
    }
    uint32_t add_node(uint32_t c, Rng &r) {
        const uint32_t n = nodes();
        count.push_back(c);
        first.push_back(tasks());
        parent.push_back(kNone);
        for (uint32_t i = 0; i < c; ++i) {
            tchild.push_back(kNone);
            tnode.push_back(n);
            tval.push_back(random_value(r));
        }
        return n;
    }
    uint32_t open_under(uint32_t task, uint32_t c, Rng &r) {
        const uint32_t n = add_node(c, r);
        tchild[task] = n;
        parent[n] = tnode[task];
        return n;
    }
    // bottom-up: a child is always created after its parent
    void evaluate() {
        sum.assign(nodes(), 0);
        value.assign(nodes(), 0);
        for (uint32_t n = nodes(); n-- > 0;) {
            unsigned long long s = 0;
            for (uint32_t t = first[n]; t < first[n] + count[n]; ++t)
                s = (s + (tchild[t] == kNone ? (tval[t] & kMask) : value[tchild[t]])) & kMask;
            sum[n] = s;
            value[n] = model_cont(n, s);
        }
    }
    // ---- what the plan reports
    std::set<uint32_t> counts_present() const { return std::set<uint32_t>(count.begin(), count.end()); }
    // the longest run of count-1 scopes one check-out climbs
    uint32_t deepest_unit_chain() const {
        uint32_t best = 0;
        std::vector<uint32_t> len(nodes(), 0);
        for (uint32_t n = 0; n < nodes(); ++n) {
            if (count[n] != 1) continue;
            len[n] = 1 + (parent[n] != kNone ? len[parent[n]] : 0);
            best = std::max(best, len[n]);
        }
        return best;
    }
    // scopes of leaves only, every value >= 2^55, at least two of them: the
    // second check-out carries whatever the order
    uint32_t carry_scopes() const {
        uint32_t k = 0;
        for (uint32_t n = 0; n < nodes(); ++n) {
            bool all = count[n] >= 2;
            for (uint32_t t = first[n]; all && t < first[n] + count[n]; ++t)
                all = tchild[t] == kNone && (tval[t] & kMask) >= (1ull << 55);
            k += all ? 1u : 0u;
        }
        return k;
    }
    uint32_t masked_leaves() const {
        uint32_t k = 0;
        for (uint32_t t = 0; t < tasks(); ++t) k += (tchild[t] == kNone && (tval[t] >> 56)) ? 1u : 0u;
        return k;
    }
};

static uint32_t random_count(Rng &r) {
    static const uint32_t small[16] = {1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 4, 4, 8, 8, 16, 5};
    static const uint32_t wide[4] = {63, 64, 65, 255};
    if (r.below(32) == 0) return wide[r.below(4)];
    return small[r.below(16)];
}

// `specials`: the counts around the wave size and the limit, count-1 chains,
// guaranteed-carry scopes and an all-ones scope of 255 hang off the root
static Forest build_forest(uint64_t seed, uint32_t root_count, bool specials, uint32_t max_nodes, uint32_t max_tasks) {
    Rng r{seed};
    Forest f;
    f.add_node(root_count, r);
    std::vector<uint32_t> queue;
    uint32_t t = f.first[0];
    if (specials) {
        for (uint32_t c : {1u, 2u, 63u, 64u, 65u, 255u}) queue.push_back(f.open_under(t++, c, r));
        for (uint32_t i = 0; i < 8; ++i) {  // chains of 6..13 count-1 scopes
            uint32_t n = f.open_under(t++, 1, r);
            for (uint32_t d = 0; d < 5 + i; ++d) n = f.open_under(f.first[n], 1, r);
        }
        const uint32_t h = f.open_under(t++, 64, r);  // 64 guaranteed-carry scopes, siblings of one batch
        for (uint32_t j = 0; j < 64; ++j) {
            const uint32_t c = f.open_under(f.first[h] + j, 2 + (j % 3 == 0 ? 1 : 0), r);
            for (uint32_t i = 0; i < f.count[c]; ++i)
                f.tval[f.first[c] + i] = (1ull << 55) | (r.next() & (kMask >> 1)) | ((j & 1) ? r.next() << 56 : 0ull);
        }
        const uint32_t w = f.open_under(t++, 255, r);  // every check-out but the first carries
        for (uint32_t i = 0; i < 255; ++i) f.tval[f.first[w] + i] = ~0ull;
    }
    for (; t < f.first[0] + root_count; ++t) queue.push_back(f.open_under(t, random_count(r), r));
    for (size_t qi = 0; qi < queue.size() && f.nodes() < max_nodes && f.tasks() < max_tasks; ++qi) {
        const uint32_t n = queue[qi];
        for (uint32_t i = 0; i < f.count[n] && f.nodes() < max_nodes && f.tasks() < max_tasks; ++i) {
            if (f.tchild[f.first[n] + i] != kNone) continue;
            if (r.below(f.count[n] >= 63 ? 8 : 2) == 0) queue.push_back(f.open_under(f.first[n] + i, random_count(r), r));
        }
    }
    f.evaluate();
    return f;
}

// ------------------------------------------------------------ device side
struct Record {
    uint32_t scope, pad;
    unsigned long long value;
};

struct Dev {
    const uint32_t *ncount, *nfirst, *tchild, *trec;  // tchild[ntasks] = 0: the task that opens the root
    const unsigned long long *tval;
    uint32_t nnodes, ntasks;
    unsigned int *fired;
    unsigned long long *seen;
    uint32_t *err;
    unsigned long long *ctr;
    unsigned long long *list;  // {task, scope} items, list_cap per workgroup
    uint32_t list_cap;
    Record *rec;
    uint32_t nrec;
};

enum : int {
    C_RAN,       // continuations the lanes report (return values)
    C_LDS,       // opens that returned an LDS id
    C_HBM,       // finish_open_local opens that returned an HBM id
    C_CHANGED,   // promotions that changed an id
    C_ALREADY,   // promotions of a slot this driver had seen forwarded (same HBM id again)
    C_CROSS,     // check-outs through a slot the driver had seen forwarded
    C_STRADDLE,  // form 2: batches whose ids were not contiguous
    C_FULL,      // export batches with all 64 lanes in finish_promote
    C_SINGLE,    // ... with one lane, not lane 0
    C_PROMOTED,  // ids finish_promote took from the arena (the allocator's movement)
    C_BAD,       // a promotion that returned something impossible
    C_BATCHES,
    C_SUBSET,    // export batches with a strict subset of the lanes
    C_FOREIGN,   // form 2: ids the driver took from the arena between batches, as another wave would
    C_N = 16
};

struct Cont {
    unsigned int *fired;
    unsigned long long *seen;
    uint32_t n;
    __device__ unsigned long long operator()(uint32_t cw, unsigned long long sum) const {
        if (cw < n) {
            atomicAdd(&fired[cw], 1u);
            hx::st_agent(&seen[cw], sum);
        }
        return (3ull * sum + 0x9E3779B1ull * cw + 1ull) & hx::kScopeSumMask;
    }
};

__device__ __forceinline__ uint32_t mix32(uint32_t a) {
    a ^= a >> 16;
    a *= 0x7feb352du;
    a ^= a >> 15;
    a *= 0x846ca68bu;
    a ^= a >> 16;
    return a;
}

__device__ __forceinline__ void flush_counters(const Dev &d, const unsigned long long (&c)[C_N]) {
#pragma unroll
    for (int i = 0; i < C_N; ++i)
        if (c[i]) atomicAdd(&d.ctr[i], c[i]);
}

// what the driver learns from one finish_promote (return values only)
template <int NL>
__device__ __forceinline__ void note_promotion(uint32_t s, uint32_t s2, uint32_t (&fwd)[NL], unsigned long long (&c)[C_N]) {
    if (hx::scope_is_lds(s)) {
        const uint32_t slot = s & (hx::kScopeLds - 1);
        if (slot >= (uint32_t)NL || s2 == hx::kScopeRoot || hx::scope_is_lds(s2)) {
            c[C_BAD] += 1;
        } else if (fwd[slot]) {
            c[C_ALREADY] += 1;
            if (fwd[slot] - 1 != s2) c[C_BAD] += 1;  // a slot forwards to one HBM scope for good
        } else {
            c[C_CHANGED] += 1;
            fwd[slot] = 1 + s2;
        }
    } else if (s2 != s) {
        c[C_BAD] += 1;
    }
}

// One wave works the list in batches of 64 (a stack or a queue). PARTB: one
// workgroup per task of the pre-opened root scope (HBM scope 0); leaves with
// a record index are promoted and left for k_checkout_records.
template <int FORM, int N, bool PARTB>
__global__ __launch_bounds__(64) void k_drive(Dev d, hx::FinishArena a, int queue, uint32_t seed) {
    constexpr int NL = N > 0 ? N : 1;
    __shared__ hx::LocalScopes<NL> ls;
    __shared__ uint32_t blk[2];
    __shared__ uint32_t fwd[NL];  // the driver's own record: slot -> 1 + the HBM id a promotion returned
    const uint32_t lane = (uint32_t)hx::lane_id();
    ls.init();
    for (uint32_t i = lane; i < (uint32_t)NL; i += 64) fwd[i] = 0;
    if (lane < 2) blk[lane] = 0;
    __syncthreads();
    const Cont cont{d.fired, d.seen, d.nnodes};
    hx::FinishInFlight q;
    unsigned long long c[C_N] = {};
    unsigned long long *list = d.list + (size_t)blockIdx.x * d.list_cap;
    uint32_t head = 0, tail = 1;
    if (lane == 0)
        hx::st_agent(&list[0], PARTB ? ((unsigned long long)(d.nfirst[0] + blockIdx.x))  // scope 0
                                     : ((unsigned long long)d.ntasks | (unsigned long long)hx::kScopeRoot << 32));
    __threadfence();
    const uint32_t max_batches = d.ntasks + 2;
    for (uint32_t batch = 0; batch < max_batches && tail != head; ++batch) {
        if (FORM == 3 || FORM == 5) c[C_RAN] += hx::finish_resolve(a, q, cont);
        const uint32_t n = tail - head, b = n < 64u ? n : 64u;
        const bool has = lane < b;
        unsigned long long item = (unsigned long long)kNone;
        if (has) item = hx::ld_agent(&list[queue ? head + lane : tail - 1 - lane]);
        if (queue) head += b;
        else tail -= b;
        const uint32_t t = (uint32_t)item, sc = has ? (uint32_t)(item >> 32) : hx::kScopeRoot;
        const uint32_t child = has ? d.tchild[t] : kNone;
        const bool opens = has && child != kNone;
        const uint32_t cnt = opens ? d.ncount[child] : 0u;
        // ---- the opens of this batch
        if (FORM == 2 && (mix32(seed + batch) & 3u) == 0u && lane == 0) {
            // another wave's allocation between two of this wave's blocks: the
            // rest of the current block and the next block are not contiguous
            const uint32_t k = 1u + mix32(seed ^ batch) % 5u;
            hx::add_agent(a.next, k);
            c[C_FOREIGN] += k;
        }
        const uint32_t nb = FORM >= 4 ? hx::ld_agent(a.next) : 0u;
        uint32_t id;
        if (FORM == 1 || FORM == 3) id = hx::finish_open(a, opens, sc, cnt, child, d.err);
        else if (FORM == 2) id = hx::finish_open(a, opens, sc, cnt, child, d.err, blk);
        else id = hx::finish_open_local(a, ls, opens, sc, cnt, child, d.err);
        const bool opened = opens && id != hx::kScopeRoot;
        if (FORM >= 4) {
            const uint32_t na = hx::ld_agent(a.next);
            const unsigned long long hm = __ballot(opened && !hx::scope_is_lds(id));
            if (lane == 0) c[C_PROMOTED] += (na - nb) - (uint32_t)__popcll(hm);  // the fall-back promotes the parents
            if (opened && hx::scope_is_lds(id)) c[C_LDS] += 1;
            if (opened && !hx::scope_is_lds(id)) c[C_HBM] += 1;
        }
        if (FORM == 2) {
            const unsigned long long om = __ballot(opened);
            if (om) {
                const uint32_t rank = (uint32_t)__popcll(om & ((1ull << lane) - 1ull));
                const uint32_t base = id - rank, b0 = (uint32_t)__shfl((int)base, __builtin_ctzll(om));
                if (__ballot(opened && base != b0) && lane == 0) c[C_STRADDLE] += 1;
            }
        }
        // ---- the children of the opened scopes go onto the list
        const uint32_t push = opened ? cnt : 0u;
        uint32_t incl = push;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
            if (lane >= (uint32_t)o) incl += v;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        if (tail + total > d.list_cap) {  // (never: the list holds every task of the tree)
            if (lane == 0) hx::dev_error(d.err, hx::kErrStackOverflow);
            break;
        }
        for (uint32_t j = 0; j < push; ++j)
            hx::st_agent(&list[tail + (incl - push) + j],
                         (unsigned long long)(d.nfirst[child] + j) | (unsigned long long)id << 32);
        tail += total;
        __threadfence();
        // ---- the leaves check out
        if (has && !opens) {
            const unsigned long long val = d.tval[t];
            const uint32_t r = PARTB ? d.trec[t] : kNone;
            if (FORM >= 4 && hx::scope_is_lds(sc) && r == kNone && (sc & (hx::kScopeLds - 1)) < (uint32_t)NL &&
                fwd[sc & (hx::kScopeLds - 1)])
                c[C_CROSS] += 1;
            if (r != kNone) {
                // leaves the wave: its scope (and the chain above) to HBM
                const uint32_t s2 = hx::finish_promote(a, ls, sc, d.err);
                note_promotion<NL>(sc, s2, fwd, c);
                if (r < d.nrec) d.rec[r] = Record{s2, 0u, val};
            } else if (FORM == 1 || FORM == 2) {
                c[C_RAN] += hx::finish_check_out(a, sc, val, cont);
            } else if (FORM == 3) {
                if (q.s == hx::kScopeRoot && sc != hx::kScopeRoot) hx::finish_issue(a, q, sc, val);
                else c[C_RAN] += hx::finish_check_out(a, sc, val, cont);
            } else if (FORM == 4) {
                c[C_RAN] += hx::finish_check_out_local(a, ls, sc, val, cont);
            } else {
                c[C_RAN] += hx::finish_check_out_local(a, ls, sc, val, cont, &q);
            }
        }
        // ---- export: a seeded subset of the pending items is promoted
        if (FORM >= 4) {
            const uint32_t h = mix32(seed ^ (batch * 0x9E3779B9u));
            const uint32_t mode = h % 37u == 0u ? 2u : h % 13u == 1u ? 3u : h % 8u == 0u ? 1u : 0u;
            const uint32_t np = tail - head;
            const bool pend = lane < (np < 64u ? np : 64u);
            const uint32_t ppos = queue ? head + lane : tail - 1 - lane;
            const bool sel = pend && (mode == 2u || (mode == 1u && (mix32(h + lane) & 3u) == 0u) ||
                                      (mode == 3u && lane == 1u + (h >> 8) % 63u));
            const uint32_t pb = hx::ld_agent(a.next);
            if (sel) {
                const unsigned long long it = hx::ld_agent(&list[ppos]);
                const uint32_t s = (uint32_t)(it >> 32);
                const uint32_t s2 = hx::finish_promote(a, ls, s, d.err);  // a strict subset of the lanes
                const unsigned long long act = __ballot(1);
                if ((int)lane == __builtin_ctzll(act)) {
                    if (act == ~0ull) c[C_FULL] += 1;
                    else c[C_SUBSET] += 1;
                    if (__popcll(act) == 1 && lane != 0) c[C_SINGLE] += 1;
                }
                note_promotion<NL>(s, s2, fwd, c);
                if (mode == 1u && hx::scope_is_lds(s)) {
                    // a second item that still names the LDS scope leaves too:
                    // already forwarded, the same HBM scope again
                    const uint32_t s3 = hx::finish_promote(a, ls, s, d.err);
                    note_promotion<NL>(s, s3, fwd, c);
                    if (s3 != s2) c[C_BAD] += 1;
                }
                hx::st_agent(&list[ppos], (it & 0xffffffffull) | (unsigned long long)s2 << 32);
            }
            if (lane == 0) c[C_PROMOTED] += hx::ld_agent(a.next) - pb;
            __threadfence();
        }
        c[C_BATCHES] += lane == 0 ? 1u : 0u;
    }
    if (FORM == 3 || FORM == 5) c[C_RAN] += hx::finish_drain(a, q, cont);
    flush_counters(d, c);
}

// Part B, kernel 2: one record per lane, 256-thread workgroups
__global__ __launch_bounds__(256) void k_checkout_records(Dev d, hx::FinishArena a, uint32_t nrec) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrec) return;
    const Record r = d.rec[i];
    const uint32_t ran = hx::finish_check_out(a, r.scope, r.value, Cont{d.fired, d.seen, d.nnodes});
    if (ran) atomicAdd(&d.ctr[C_RAN], (unsigned long long)ran);
}

// ---- limits (one wave each)
// batch 0 (LOCAL only): 64 good opens, all LDS. Batch 1: lane 3 count 0, lane
// 7 count 256, lane 5 count 255, the others 1..3; good lanes check out `count`
// times with values 1..count. out[0..63] batch 0 ids, out[64..127] batch 1 ids
template <bool LOCAL>
__global__ __launch_bounds__(64) void k_limit_counts(Dev d, hx::FinishArena a, uint32_t *out) {
    __shared__ hx::LocalScopes<64> ls;
    const uint32_t lane = (uint32_t)hx::lane_id();
    ls.init();
    __syncthreads();
    const Cont cont{d.fired, d.seen, d.nnodes};
    unsigned long long c[C_N] = {};
    if (LOCAL) {
        const uint32_t id = hx::finish_open_local(a, ls, true, hx::kScopeRoot, 1, lane, d.err);
        out[lane] = id;
        if (id != hx::kScopeRoot) c[C_RAN] += hx::finish_check_out_local(a, ls, id, 1000ull + lane, cont);
    }
    const uint32_t cnt = lane == 3 ? 0u : lane == 7 ? 256u : lane == 5 ? 255u : 1u + lane % 3u;
    const uint32_t id = LOCAL ? hx::finish_open_local(a, ls, true, hx::kScopeRoot, cnt, 64 + lane, d.err)
                              : hx::finish_open(a, true, hx::kScopeRoot, cnt, 64 + lane, d.err);
    out[64 + lane] = id;
    if (id != hx::kScopeRoot)
        for (uint32_t j = 0; j < cnt && j < 256u; ++j)
            c[C_RAN] += LOCAL ? hx::finish_check_out_local(a, ls, id, 1ull + j, cont)
                              : hx::finish_check_out(a, id, 1ull + j, cont);
    flush_counters(d, c);
}

// 64 opens into an arena with room for fewer
__global__ __launch_bounds__(64) void k_limit_arena(Dev d, hx::FinishArena a, uint32_t *out) {
    const uint32_t lane = (uint32_t)hx::lane_id();
    const Cont cont{d.fired, d.seen, d.nnodes};
    unsigned long long c[C_N] = {};
    const uint32_t id = hx::finish_open(a, true, hx::kScopeRoot, 1, lane, d.err);
    out[lane] = id;
    if (id != hx::kScopeRoot) c[C_RAN] += hx::finish_check_out(a, id, 7ull + lane, cont);
    flush_counters(d, c);
}

// Lanes 0..7 each hold an LDS scope C (cw 8 + lane) inside an LDS scope P (cw
// lane). The arena (cap 12) starts with next = 8: promoting all eight chains
// needs 16 ids and fails. The wave then does what the host does between
// launches (next = 0, error word = 0; the LDS state could not outlive a
// launch) and lanes 0..3 promote again: 8 ids, no more — a round left open
// would take the failed round's marks on the chains of lanes 4..7 for its own.
// out[0..7] first returns, out[64] the error word after them, out[128..131]
// second returns, out[65] `next` after them.
__global__ __launch_bounds__(64) void k_limit_promote(Dev d, hx::FinishArena a, uint32_t *out) {
    __shared__ hx::LocalScopes<32> ls;
    const uint32_t lane = (uint32_t)hx::lane_id();
    ls.init();
    __syncthreads();
    const Cont cont{d.fired, d.seen, d.nnodes};
    unsigned long long c[C_N] = {};
    const bool act = lane < 8;
    const uint32_t P = hx::finish_open_local(a, ls, act, hx::kScopeRoot, 1, lane, d.err);
    const uint32_t C = hx::finish_open_local(a, ls, act, P, 1, 8 + lane, d.err);
    uint32_t r1 = kNone - 1, r2 = kNone - 1;
    if (act) r1 = hx::finish_promote(a, ls, C, d.err);
    out[lane] = r1;
    __threadfence();
    if (lane == 0) {
        out[64] = hx::ld_agent(d.err);
        hx::st_agent(a.next, 0u);
        hx::st_agent(d.err, 0u);
    }
    __threadfence();
    if (lane < 4) r2 = hx::finish_promote(a, ls, C, d.err);
    out[128 + lane] = r2;
    if (lane == 0) out[65] = hx::ld_agent(a.next);
    if (act) c[C_RAN] += hx::finish_check_out_local(a, ls, C, 100ull + lane, cont);
    flush_counters(d, c);
}

// ---- part C: the walk as a scheduler kind
constexpr int kWalkScopes = 128;
__shared__ hx::LocalScopes<kWalkScopes> s_walk_scopes;

struct WalkCtx {
    Dev d;
    hx::FinishArena fin;
};

struct WalkKind {
    // template = {node, the node's scope}; child k is task first[node] + k.
    // Fan-outs go up to 255, the protocol's own limit: the scheduler allows
    // kMaxChildren - 1 per task and splits them into range items
    static constexpr int kTmplWords = 2;
    static constexpr int kWords = 4;
    static constexpr bool kPure = false;
    static constexpr bool kBoundedChildren = true;
    using Ctx = WalkCtx;
    struct Acc {
        unsigned long long tasks = 0, ran = 0, lds = 0, hbm = 0;
        hx::FinishInFlight q;
        __device__ void flush(hx::SchedGlobals *g) {
            const unsigned long long v[4] = {hx::wave_sum(tasks), hx::wave_sum(ran), hx::wave_sum(lds), hx::wave_sum(hbm)};
            if (hx::lane_id() == 0)
                for (int i = 0; i < 4; ++i) hx::add_agent(&g->counters[i], v[i]);
        }
    };
    __device__ static Cont cont(const Ctx &c) { return Cont{c.d.fired, c.d.seen, c.d.nnodes}; }
    __device__ static int roots(const Ctx &c, Acc &, uint32_t *tmpl) {
        tmpl[0] = c.d.nnodes;  // its one task (index ntasks) opens node 0
        tmpl[1] = hx::kScopeRoot;
        return 1;
    }
    __device__ static int process(const Ctx &c, Acc &acc, const uint32_t *t, uint32_t k, uint32_t *child,
                                  uint32_t *err, bool) {
        acc.ran += hx::finish_resolve(c.fin, acc.q, cont(c));
        acc.tasks += 1;
        const uint32_t task = t[0] >= c.d.nnodes ? c.d.ntasks : c.d.nfirst[t[0]] + k;
        const uint32_t ch = task <= c.d.ntasks ? c.d.tchild[task] : kNone;
        const bool opens = ch != kNone;
        const uint32_t cnt = opens ? c.d.ncount[ch] : 0u;
        const uint32_t id = hx::finish_open_local(c.fin, s_walk_scopes, opens, t[1], cnt, ch, err);
        if (opens) {
            if (id == hx::kScopeRoot) return 0;  // arena error (reported)
            if (hx::scope_is_lds(id)) acc.lds += 1;
            else acc.hbm += 1;
            child[0] = ch;
            child[1] = id;
            return (int)cnt;
        }
        acc.ran += hx::finish_check_out_local(c.fin, s_walk_scopes, t[1], c.d.tval[task < c.d.ntasks ? task : 0],
                                              cont(c), &acc.q);
        return 0;
    }
    // the ring ran empty: the check-outs still in flight, to their ends
    __device__ static void drain(const Ctx &c, Acc &acc, uint32_t *) { acc.ran += hx::finish_drain(c.fin, acc.q, cont(c)); }
    // an item leaving the wave names an HBM scope (its LDS scope promoted)
    __device__ static void export_item(const Ctx &c, uint32_t *w, bool valid, uint32_t *err) {
        const uint32_t s = hx::finish_promote(c.fin, s_walk_scopes, valid ? w[1] : hx::kScopeRoot, err);
        if (valid) w[1] = s;
    }
};

constexpr int kWalkCap = 1024;
__global__ __launch_bounds__(64) void k_walk(WalkCtx ctx, hx::PoolView pool, hx::SchedGlobals *g, hx::SchedConfig cfg) {
    __shared__ hx::WaveStack<WalkKind, kWalkCap> st;
    s_walk_scopes.init();
    __syncthreads();
    hx::run_worker<WalkKind, kWalkCap>(ctx, pool, g, cfg, st, blockIdx.x == 0);
}

// ------------------------------------------------------------- host side
static int g_fail = 0, g_form_fail = 0;
static const char *g_what = "";
static void fail(const char *fmt, ...) {
    ++g_fail;
    if (++g_form_fail > 12) return;
    fprintf(stdout, "FAILED %s: ", g_what);
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stdout, fmt, ap);
    va_end(ap);
    fprintf(stdout, "\n");
}
#define HIP_OK(e)                                                                             \
    do {                                                                                      \
        const hipError_t e_ = (e);                                                            \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "FAILED %s:%d: %s: %s\n", __FILE__, __LINE__, #e, hipGetErrorString(e_)); \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

template <class T>
static T *to_device(const std::vector<T> &v) {
    T *p = nullptr;
    HIP_OK(hipMalloc((void **)&p, std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (!v.empty()) HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}
template <class T>
static std::vector<T> to_host(const T *p, size_t n) {
    std::vector<T> v(n);
    if (n) HIP_OK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}

// a forest on the device with its result arrays
struct DevForest {
    Dev d{};
    std::vector<void *> owned;
    template <class T>
    T *keep(T *p) {
        owned.push_back((void *)p);
        return p;
    }
    DevForest(const Forest &f, const std::vector<uint32_t> *trec, uint32_t nrec, uint32_t lists) {
        std::vector<uint32_t> tc = f.tchild;
        tc.push_back(0);  // the task that opens the root
        std::vector<unsigned long long> tv = f.tval;
        tv.push_back(0);
        d.ncount = keep(to_device(f.count));
        d.nfirst = keep(to_device(f.first));
        d.tchild = keep(to_device(tc));
        d.tval = keep(to_device(tv));
        d.trec = trec ? keep(to_device(*trec)) : nullptr;
        d.nnodes = f.nodes();
        d.ntasks = f.tasks();
        d.list_cap = f.tasks() + 64;
        d.nrec = nrec;
        HIP_OK(hipMalloc((void **)&d.fired, 4 * (size_t)d.nnodes));
        HIP_OK(hipMalloc((void **)&d.seen, 8 * (size_t)d.nnodes));
        HIP_OK(hipMalloc((void **)&d.err, 256));
        HIP_OK(hipMalloc((void **)&d.ctr, 8 * C_N));
        HIP_OK(hipMalloc((void **)&d.list, 8 * (size_t)d.list_cap * std::max(lists, 1u)));
        HIP_OK(hipMalloc((void **)&d.rec, sizeof(Record) * (size_t)std::max(nrec, 1u)));
        keep(d.fired), keep(d.seen), keep(d.err), keep(d.ctr), keep(d.list), keep(d.rec);
        clear();
    }
    void clear() {
        HIP_OK(hipMemset(d.fired, 0, 4 * (size_t)d.nnodes));
        HIP_OK(hipMemset(d.seen, 0xEE, 8 * (size_t)d.nnodes));
        HIP_OK(hipMemset(d.err, 0, 256));
        HIP_OK(hipMemset(d.ctr, 0, 8 * C_N));
        HIP_OK(hipMemset(d.rec, 0xFF, sizeof(Record) * (size_t)std::max(d.nrec, 1u)));
    }
    ~DevForest() {
        for (void *p : owned) (void)hipFree(p);
    }
};

static void fill_arena(const hclib::hip::finish_arena &fin, uint32_t cap) {
    HIP_OK(hipMemset(fin.view().scopes, 0xFF, sizeof(hx::FinishScope) * (size_t)cap));
}

// fired / seen / root / ran / error word / the arena's contents against the model.
// `unused_ok`: ids may have been taken and never opened (form 2's blocks)
static void check_against_model(const Forest &f, const DevForest &D, const hclib::hip::finish_arena &fin, uint32_t cap,
                                unsigned long long ran, bool unused_ok, bool all_in_hbm) {
    const std::vector<unsigned int> fired = to_host(D.d.fired, f.nodes());
    const std::vector<unsigned long long> seen = to_host(D.d.seen, f.nodes());
    uint32_t bad_fired = 0, bad_seen = 0, first_bad = kNone;
    for (uint32_t n = 0; n < f.nodes(); ++n) {
        if (fired[n] != 1) ++bad_fired, first_bad = std::min(first_bad, n);
        else if (seen[n] != f.sum[n]) ++bad_seen, first_bad = std::min(first_bad, n);
    }
    if (bad_fired)
        fail("continuation count: %u of %u scopes did not run exactly once (first: scope %u of count %u ran %u times)",
             bad_fired, f.nodes(), first_bad, f.count[first_bad], fired[first_bad]);
    if (bad_seen)
        fail("continuation sum: %u scopes saw a wrong sum (first: scope %u of count %u saw %llx, model %llx)", bad_seen,
             first_bad, f.count[first_bad], seen[first_bad], f.sum[first_bad]);
    const unsigned long long root = fin.root_value();
    if (root != f.value[0]) fail("root value %llx, model %llx", root, f.value[0]);
    if (ran != f.nodes()) fail("lanes report %llu continuations, %u scopes", ran, f.nodes());
    const uint32_t err = to_host(D.d.err, 1)[0];
    if (err != 0) fail("device error word %u", err);
    // the arena: every allocated id is one distinct scope of the model,
    // closed, holding the model's sum, under an HBM parent (or the root)
    const uint32_t next = fin.scopes_opened();
    if (next > cap) {
        fail("allocator at %u past the capacity %u", next, cap);
        return;
    }
    const std::vector<hx::FinishScope> sc = to_host(fin.view().scopes, next);
    std::vector<uint32_t> id_of(f.nodes(), kNone);
    uint32_t unused = 0, bad = 0;
    for (uint32_t i = 0; i < next; ++i) {
        if (sc[i].cont == kNone && sc[i].word == ~0ull) {
            ++unused;
            continue;
        }
        if (sc[i].cont >= f.nodes() || id_of[sc[i].cont] != kNone) {
            if (!bad++) fail("arena id %u: continuation word %u is no scope of the model, or a second copy of one", i, sc[i].cont);
            continue;
        }
        id_of[sc[i].cont] = i;
    }
    for (uint32_t i = 0; i < next; ++i) {
        if (sc[i].cont >= f.nodes() || id_of[sc[i].cont] != i) continue;
        const uint32_t n = sc[i].cont, p = f.parent[n];
        if ((sc[i].word >> 56) != 0 || (sc[i].word & kMask) != f.sum[n]) {
            if (!bad++) fail("arena id %u (scope %u): word %llx, model: closed with sum %llx", i, n, sc[i].word, f.sum[n]);
        }
        const bool parent_ok = p == kNone ? sc[i].parent == hx::kScopeRoot : sc[i].parent < next && id_of[p] == sc[i].parent;
        if (!parent_ok && !bad++)
            fail("arena id %u (scope %u): parent %x is not the HBM copy of scope %d", i, n, sc[i].parent, (int)p);
    }
    if (bad > 1) fail("... %u arena entries wrong", bad);
    if (unused && !unused_ok) fail("%u ids taken from the arena and never opened", unused);
    if (all_in_hbm)
        for (uint32_t n = 0; n < f.nodes(); ++n)
            if (id_of[n] == kNone) {
                fail("scope %u has no HBM copy", n);
                break;
            }
}

struct FormSpec {
    int form, n;
    const char *name;
};
static const FormSpec kForms[] = {{1, 0, "A1-open"},          {2, 0, "A2-blocks"},         {3, 0, "A3-issue-resolve"},
                                  {4, 4, "A4-local<4>"},      {4, 64, "A4-local<64>"},     {5, 4, "A5-local-inflight<4>"},
                                  {5, 64, "A5-local-inflight<64>"}};
static const char *kOrders[2] = {"stack", "queue"};

static void launch_drive(int form, int n, const Dev &d, const hx::FinishArena &a, int queue, uint32_t seed) {
    const dim3 g(1), b(64);
    if (form == 1) hipLaunchKernelGGL((k_drive<1, 0, false>), g, b, 0, 0, d, a, queue, seed);
    else if (form == 2) hipLaunchKernelGGL((k_drive<2, 0, false>), g, b, 0, 0, d, a, queue, seed);
    else if (form == 3) hipLaunchKernelGGL((k_drive<3, 0, false>), g, b, 0, 0, d, a, queue, seed);
    else if (form == 4 && n == 4) hipLaunchKernelGGL((k_drive<4, 4, false>), g, b, 0, 0, d, a, queue, seed);
    else if (form == 4) hipLaunchKernelGGL((k_drive<4, 64, false>), g, b, 0, 0, d, a, queue, seed);
    else if (n == 4) hipLaunchKernelGGL((k_drive<5, 4, false>), g, b, 0, 0, d, a, queue, seed);
    else hipLaunchKernelGGL((k_drive<5, 64, false>), g, b, 0, 0, d, a, queue, seed);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
}

// one launch of part A; returns whether every check held
static bool run_form(const Forest &f, DevForest &D, const FormSpec &fs, int queue, const char *label) {
    g_what = label;
    g_form_fail = 0;
    const uint32_t cap = f.nodes() + hx::kScopeBlock + 64 + 5 * (f.tasks() + 2);  // (form 2's foreign ids)
    hclib::hip::finish_arena fin(cap);
    if (!fin.ok()) {
        fail("finish_arena");
        return false;
    }
    fill_arena(fin, cap);
    D.clear();
    launch_drive(fs.form, fs.n, D.d, fin.view(), queue, 0xF1F0u + 97u * (uint32_t)fs.form + (uint32_t)fs.n + (uint32_t)queue);
    const std::vector<unsigned long long> c = to_host(D.d.ctr, C_N);
    check_against_model(f, D, fin, cap, c[C_RAN], fs.form == 2, fs.form <= 3);
    const uint32_t opened = fin.scopes_opened();
    if (fs.form == 1 || fs.form == 3) {
        if (opened != f.nodes()) fail("%u ids taken, %u scopes", opened, f.nodes());
    } else if (fs.form == 2) {
        if (opened < f.nodes() + c[C_FOREIGN] || opened > f.nodes() + c[C_FOREIGN] + hx::kScopeBlock)
            fail("%u ids taken, %u scopes + %llu foreign ids and at most one block of %u", opened, f.nodes(), c[C_FOREIGN],
                 hx::kScopeBlock);
        if (!c[C_STRADDLE]) fail("no batch of opens straddled a block boundary");
    } else {
        if (opened != c[C_HBM] + c[C_PROMOTED])
            fail("%u ids taken, the kernel counted %llu fall-back opens + %llu promoted", opened, c[C_HBM], c[C_PROMOTED]);
        if (c[C_LDS] + c[C_HBM] != f.nodes()) fail("%llu LDS + %llu HBM opens, %u scopes", c[C_LDS], c[C_HBM], f.nodes());
        if (c[C_BAD]) fail("%llu promotions returned an impossible id", c[C_BAD]);
        if (!c[C_LDS]) fail("no open returned an LDS scope");
        if (!c[C_HBM]) fail("no open fell back to an HBM scope (dry free list)");
        if (!c[C_PROMOTED]) fail("nothing was promoted");
        // (LocalScopes<4> is there for the dry free list and the promotion of
        // the parents it brings: with four slots hardly a pending item names an
        // LDS scope when the driver exports)
        if (fs.n > 4 && !c[C_CHANGED]) fail("no promotion changed an id");
        if (fs.n > 4 && !c[C_ALREADY]) fail("no promotion found its scope already forwarded");
        if (fs.n > 4 && !c[C_CROSS]) fail("no check-out went through a forwarded slot into HBM");
        if (!c[C_SUBSET]) fail("no promotion ran on a strict subset of the lanes");
        if (!c[C_FULL]) fail("no promotion ran on all 64 lanes");
        if (!c[C_SINGLE]) fail("no promotion ran on a single lane other than lane 0");
    }
    if (g_form_fail) return false;
    printf("  %-24s %-5s %5u scopes %6u tasks %5llu batches: ids %u", fs.name, kOrders[queue], f.nodes(), f.tasks(),
           c[C_BATCHES], opened);
    if (fs.form == 2) printf(", %llu foreign, %llu batches of non-contiguous ids", c[C_FOREIGN], c[C_STRADDLE]);
    if (fs.form >= 4)
        printf(", opens %llu LDS / %llu HBM, promotions %llu new / %llu known, %llu through forwards, rounds %llu subset / "
               "%llu full / %llu single",
               c[C_LDS], c[C_HBM], c[C_CHANGED], c[C_ALREADY], c[C_CROSS], c[C_SUBSET], c[C_FULL], c[C_SINGLE]);
    printf("\n");
    return true;
}

// ---- part B plans (host only)
struct PartBPlan {
    std::vector<uint32_t> trec;  // per task: its record, or kNone
    uint32_t nrec = 0, scopes_with_records = 0, max_span = 0, max_records = 0;
    uint32_t min_span_255 = kNone;  // over the count-255 scopes that have records
};
static void span_stats(const Forest &f, PartBPlan &p) {
    std::vector<std::set<uint32_t>> wgs(f.nodes());
    std::vector<uint32_t> per(f.nodes(), 0);
    for (uint32_t t = 0; t < f.tasks(); ++t)
        if (p.trec[t] != kNone) {
            wgs[f.tnode[t]].insert(p.trec[t] / 256);
            per[f.tnode[t]] += 1;
        }
    for (uint32_t n = 0; n < f.nodes(); ++n) {
        if (!per[n]) continue;
        p.scopes_with_records += 1;
        p.max_span = std::max(p.max_span, (uint32_t)wgs[n].size());
        p.max_records = std::max(p.max_records, per[n]);
        if (f.count[n] == 255) p.min_span_255 = std::min(p.min_span_255, (uint32_t)wgs[n].size());
    }
}
// `every`: all leaves become records (the contention case), else a seeded half
static PartBPlan plan_part_b(const Forest &f, uint64_t seed, bool every) {
    Rng r{seed};
    PartBPlan p;
    p.trec.assign(f.tasks(), kNone);
    std::vector<uint32_t> picked;
    for (uint32_t t = 0; t < f.tasks(); ++t)
        if (f.tchild[t] == kNone && (every || (r.next() & 1))) picked.push_back(t);
    for (size_t i = picked.size(); i > 1; --i) std::swap(picked[i - 1], picked[r.below((uint32_t)i)]);
    for (size_t i = 0; i < picked.size(); ++i) p.trec[picked[i]] = (uint32_t)i;
    p.nrec = (uint32_t)picked.size();
    span_stats(f, p);
    return p;
}

constexpr uint32_t kPartBWaves = 8;
constexpr uint32_t kContendScopes = 8;
static Forest build_contention() {
    Rng r{0xC0117E17ull};
    Forest f;
    f.add_node(kContendScopes, r);
    for (uint32_t i = 0; i < kContendScopes; ++i) {
        const uint32_t n = f.open_under(f.first[0] + i, 255, r);
        if (i % 2 == 0)
            for (uint32_t j = 0; j < 255; ++j) f.tval[f.first[n] + j] = kMask;  // almost every check-out carries
    }
    f.evaluate();
    return f;
}

static bool run_part_b_tree(const Forest &f, const PartBPlan &p) {
    g_what = "B-two-kernels";
    g_form_fail = 0;
    DevForest D(f, &p.trec, p.nrec, kPartBWaves);
    const uint32_t cap = f.nodes() + 64;
    hclib::hip::finish_arena fin(cap);
    if (!fin.ok()) {
        fail("finish_arena");
        return false;
    }
    fill_arena(fin, cap);
    // scope 0: the root, one task per wave of kernel 1
    if (fin.preopen({f.count[0]}, {hx::kScopeRoot}, {0u}) != HCLIB_HIP_OK) fail("preopen");
    hipLaunchKernelGGL((k_drive<4, 64, true>), dim3(f.count[0]), dim3(64), 0, 0, D.d, fin.view(), 0, 0xB0B0u);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_checkout_records, dim3((p.nrec + 255) / 256), dim3(256), 0, 0, D.d, fin.view(), p.nrec);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<unsigned long long> c = to_host(D.d.ctr, C_N);
    check_against_model(f, D, fin, cap, c[C_RAN], false, false);
    const uint32_t opened = fin.scopes_opened();
    // (eight waves move the allocator at once: what each promotion took cannot
    // be read off it here. The arena's contents above say that every id taken
    // is one distinct scope; the return values give a lower bound)
    if (opened <= 1 + c[C_HBM] || opened > f.nodes())
        fail("%u ids taken, the kernels saw 1 pre-opened + %llu fall-back opens and %llu promotions, %u scopes", opened,
             c[C_HBM], c[C_CHANGED], f.nodes());
    if (c[C_BAD]) fail("%llu promotions returned an impossible id", c[C_BAD]);
    if (!c[C_LDS] || !c[C_CHANGED] || !c[C_ALREADY] || !c[C_CROSS])
        fail("not reached: %llu LDS opens, %llu promotions new, %llu known, %llu check-outs through forwards", c[C_LDS],
             c[C_CHANGED], c[C_ALREADY], c[C_CROSS]);
    // every record names an HBM scope
    const std::vector<Record> rec = to_host(D.d.rec, p.nrec);
    uint32_t bad = 0;
    for (const Record &r : rec) bad += r.scope >= opened ? 1u : 0u;
    if (bad) fail("%u of %u records name no HBM scope", bad, p.nrec);
    if (g_form_fail) return false;
    printf("  %-24s %5u scopes %6u tasks: %u waves, %u records in %u workgroups of 256, ids %u (opens %llu LDS / %llu HBM, "
           "promotions %llu new / %llu known)\n",
           "B-two-kernels", f.nodes(), f.tasks(), f.count[0], p.nrec, (p.nrec + 255) / 256, opened, c[C_LDS], c[C_HBM],
           c[C_CHANGED], c[C_ALREADY]);
    return true;
}

static bool run_part_b_contention(const Forest &f, const PartBPlan &p) {
    g_what = "B-contention";
    g_form_fail = 0;
    DevForest D(f, &p.trec, p.nrec, 1);
    const uint32_t cap = f.nodes();
    hclib::hip::finish_arena fin(cap);
    if (!fin.ok()) {
        fail("finish_arena");
        return false;
    }
    std::vector<uint32_t> counts, parents, conts;
    for (uint32_t n = 0; n < f.nodes(); ++n) {
        counts.push_back(f.count[n]);
        parents.push_back(f.parent[n] == kNone ? hx::kScopeRoot : f.parent[n]);  // ids = node indices
        conts.push_back(n);
    }
    if (fin.preopen(counts, parents, conts) != HCLIB_HIP_OK) fail("preopen");
    std::vector<Record> rec(p.nrec);
    for (uint32_t t = 0; t < f.tasks(); ++t)
        if (p.trec[t] != kNone) rec[p.trec[t]] = Record{f.tnode[t], 0u, f.tval[t]};
    HIP_OK(hipMemcpy(D.d.rec, rec.data(), sizeof(Record) * rec.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_checkout_records, dim3((p.nrec + 255) / 256), dim3(256), 0, 0, D.d, fin.view(), p.nrec);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<unsigned long long> c = to_host(D.d.ctr, C_N);
    check_against_model(f, D, fin, cap, c[C_RAN], false, true);
    if (g_form_fail) return false;
    printf("  %-24s %u scopes of 255 under one of %u: %u check-outs at once from %u workgroups of 256\n", "B-contention",
           kContendScopes, kContendScopes, p.nrec, (p.nrec + 255) / 256);
    return true;
}

// ---- part C
static bool run_part_c(const Forest &f) {
    g_what = "C-scheduler-export";
    g_form_fail = 0;
    DevForest D(f, nullptr, 0, 1);
    hclib_hip_sched_launch_t L;
    hclib::hip::task_config tc;
    tc.chunk = 8;
    tc.spill_lo = 4;
    tc.hunger = 1;
    tc.spin_limit_ms = 5000;
    int rc = hclib_hip_sched_begin((uint32_t)WalkKind::kWords, tc.chunk, tc.waves_per_cu, &L);
    if (rc != HCLIB_HIP_OK) {
        fail("hclib_hip_sched_begin: %s", hclib_hip_last_error());
        return false;
    }
    // every wave's last promotion may leave nothing unused; fall-back opens take one id each
    const uint32_t cap = f.nodes() + 64;
    hclib::hip::finish_arena fin(cap);
    if (!fin.ok()) fail("finish_arena");
    fill_arena(fin, cap);
    hx::PoolView pool;
    pool.hdr = (hx::QueueHdr *)L.hdr;
    pool.seq = L.seq;
    pool.cnt = L.cnt;
    pool.data = L.data;
    pool.nq = L.nq;
    pool.cap = L.cap;
    pool.chunk = L.chunk;
    hx::SchedConfig cfg;
    cfg.spill_hi = tc.spill_hi;
    cfg.spill_lo = tc.spill_lo;
    cfg.spin_limit = tc.spin_limit_ms;
    cfg.nwaves = (uint32_t)L.grid;
    cfg.stamps = 0;
    cfg.hunger = tc.hunger;
    hipLaunchKernelGGL(k_walk, dim3(L.grid), dim3(64), 0, (hipStream_t)L.stream, WalkCtx{D.d, fin.view()}, pool,
                       (hx::SchedGlobals *)L.globals, cfg);
    hclib::hip::task_stats st;
    rc = hclib_hip_sched_end("device_finish_forms", st.counters, st.maxes, &st.kernel_ms);
    if (rc != HCLIB_HIP_OK) {
        fail("the launch: %s", hclib_hip_last_error());
        return false;
    }
    check_against_model(f, D, fin, cap, st.counters[1], false, false);
    const uint32_t opened = fin.scopes_opened();
    if (st.counters[0] != (unsigned long long)f.tasks() + 1) fail("%llu tasks ran, %u in the tree", (unsigned long long)st.counters[0], f.tasks() + 1);
    if (st.counters[2] + st.counters[3] != f.nodes())
        fail("%llu LDS + %llu HBM opens, %u scopes", (unsigned long long)st.counters[2], (unsigned long long)st.counters[3], f.nodes());
    if (!st.counters[2]) fail("no open returned an LDS scope");
    if (opened == 0 || opened <= st.counters[3]) fail("%u ids taken, %llu of them fall-back opens: nothing was promoted", opened, (unsigned long long)st.counters[3]);
    if (g_form_fail) return false;
    printf("  %-24s %5u scopes %6u tasks, fan-out up to 255 (the protocol's limit; the scheduler's is 2^24 - 1): %d waves, "
           "opens %llu LDS / %llu HBM, ids %u (%.3f ms)\n",
           "C-scheduler-export", f.nodes(), f.tasks(), L.grid, (unsigned long long)st.counters[2],
           (unsigned long long)st.counters[3], opened, st.kernel_ms);
    return true;
}

// ---- limits: an arena of the test's own, with a guard region behind it
struct RawArena {
    uint32_t cap, guard;
    hx::FinishScope *scopes = nullptr;
    uint32_t *ctl = nullptr;  // [0] next, [16..17] root value
    RawArena(uint32_t c, uint32_t g, uint32_t next0) : cap(c), guard(g) {
        HIP_OK(hipMalloc((void **)&scopes, sizeof(hx::FinishScope) * (size_t)(c + g)));
        HIP_OK(hipMemset(scopes, 0xA5, sizeof(hx::FinishScope) * (size_t)(c + g)));
        HIP_OK(hipMalloc((void **)&ctl, 256));
        HIP_OK(hipMemset(ctl, 0, 256));
        HIP_OK(hipMemcpy(ctl, &next0, 4, hipMemcpyHostToDevice));
    }
    ~RawArena() {
        (void)hipFree(scopes);
        (void)hipFree(ctl);
    }
    hx::FinishArena view() const { return hx::FinishArena{scopes, ctl, cap, (unsigned long long *)(ctl + 16)}; }
    uint32_t next() const { return to_host(ctl, 1)[0]; }
    bool guard_intact() const {
        const std::vector<unsigned char> g = to_host((const unsigned char *)(scopes + cap), sizeof(hx::FinishScope) * (size_t)guard);
        return std::all_of(g.begin(), g.end(), [](unsigned char b) { return b == 0xA5; });
    }
};

static Forest flat_forest(uint32_t n) {  // n scopes to hold fired / seen; no tasks of their own
    Rng r{1};
    Forest f;
    for (uint32_t i = 0; i < n; ++i) f.add_node(1, r);
    return f;
}

static bool limit_counts(bool local) {
    g_what = local ? "limits: bad count (finish_open_local)" : "limits: bad count (finish_open)";
    g_form_fail = 0;
    const Forest f = flat_forest(128);
    DevForest D(f, nullptr, 0, 1);
    RawArena A(256, 16, 0);
    uint32_t *out = nullptr;
    HIP_OK(hipMalloc((void **)&out, 4 * 256));
    HIP_OK(hipMemset(out, 0, 4 * 256));
    if (local) hipLaunchKernelGGL(k_limit_counts<true>, dim3(1), dim3(64), 0, 0, D.d, A.view(), out);
    else hipLaunchKernelGGL(k_limit_counts<false>, dim3(1), dim3(64), 0, 0, D.d, A.view(), out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<uint32_t> o = to_host(out, 256);
    (void)hipFree(out);
    const std::vector<unsigned int> fired = to_host(D.d.fired, 128);
    const std::vector<unsigned long long> seen = to_host(D.d.seen, 128);
    const uint32_t err = to_host(D.d.err, 1)[0];
    if (err != hx::kErrBadTask) fail("error word %u, want kErrBadTask (%u)", err, (uint32_t)hx::kErrBadTask);
    std::set<uint32_t> ids;
    unsigned long long want_ran = 0;
    for (uint32_t l = 0; l < 64; ++l) {
        const uint32_t cnt = l == 3 ? 0u : l == 7 ? 256u : l == 5 ? 255u : 1u + l % 3u, id = o[64 + l];
        if (local) {
            if (!is_lds_id(o[l])) fail("lane %u: a good batch's open gave %x, no LDS scope", l, o[l]);
            if (fired[l] != 1 || seen[l] != 1000ull + l) fail("lane %u: LDS scope ran %u times, sum %llx", l, fired[l], seen[l]);
            want_ran += 1;
        }
        if (cnt == 0 || cnt > 255) {
            if (id != hx::kScopeRoot) fail("lane %u: count %u opened scope %x", l, cnt, id);
            if (fired[64 + l] != 0) fail("lane %u: count %u ran a continuation", l, cnt);
            continue;
        }
        // beside a bad count every lane's scope is an HBM scope (finish_open_local routes the batch to finish_open)
        if (id == hx::kScopeRoot || id >= 256 || !ids.insert(id).second)
            fail("lane %u: count %u got id %x (no HBM scope, or one taken twice)", l, cnt, id);
        const unsigned long long sum = (unsigned long long)cnt * (cnt + 1) / 2;
        if (fired[64 + l] != 1 || seen[64 + l] != sum)
            fail("lane %u: count %u closed %u times with sum %llu, want once with %llu", l, cnt, fired[64 + l], seen[64 + l], sum);
        want_ran += 1;
    }
    const unsigned long long ran = to_host(D.d.ctr, C_N)[C_RAN];
    if (ran != want_ran) fail("%llu continuations reported, want %llu", ran, want_ran);
    if (!A.guard_intact()) fail("the guard region behind the arena was written");
    if (g_form_fail) return false;
    printf("  %-44s -> kErrBadTask: counts 0 and 256 get kScopeRoot, 255 opens and closes, 61 other lanes unaffected\n", g_what);
    return true;
}

static bool limit_arena_open() {
    g_what = "limits: arena exhausted in finish_open";
    g_form_fail = 0;
    const Forest f = flat_forest(64);
    DevForest D(f, nullptr, 0, 1);
    RawArena A(40, 64, 0);
    uint32_t *out = nullptr;
    HIP_OK(hipMalloc((void **)&out, 4 * 64));
    hipLaunchKernelGGL(k_limit_arena, dim3(1), dim3(64), 0, 0, D.d, A.view(), out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<uint32_t> o = to_host(out, 64);
    (void)hipFree(out);
    const std::vector<unsigned int> fired = to_host(D.d.fired, 64);
    const std::vector<unsigned long long> seen = to_host(D.d.seen, 64);
    const uint32_t err = to_host(D.d.err, 1)[0];
    if (err != hx::kErrArena) fail("error word %u, want kErrArena (%u)", err, (uint32_t)hx::kErrArena);
    std::set<uint32_t> ids;
    for (uint32_t l = 0; l < 64; ++l) {
        if (o[l] == hx::kScopeRoot) {
            if (fired[l]) fail("lane %u: no scope, yet a continuation ran", l);
            continue;
        }
        if (o[l] >= 40 || !ids.insert(o[l]).second) fail("lane %u: id %x outside the arena or taken twice", l, o[l]);
        if (fired[l] != 1 || seen[l] != 7ull + l) fail("lane %u: closed %u times, sum %llx", l, fired[l], seen[l]);
    }
    if (ids.size() != 40) fail("%zu lanes got a scope, the arena holds 40", ids.size());
    if (!A.guard_intact()) fail("the guard region behind the arena was written");
    if (g_form_fail) return false;
    printf("  %-44s -> kErrArena: 40 of 64 opens fit, 24 get kScopeRoot, nothing written at or past cap\n", g_what);
    return true;
}

static bool limit_arena_promote() {
    g_what = "limits: arena exhausted in finish_promote";
    g_form_fail = 0;
    const Forest f = flat_forest(16);
    DevForest D(f, nullptr, 0, 1);
    RawArena A(12, 64, 8);
    uint32_t *out = nullptr;
    HIP_OK(hipMalloc((void **)&out, 4 * 256));
    HIP_OK(hipMemset(out, 0, 4 * 256));
    hipLaunchKernelGGL(k_limit_promote, dim3(1), dim3(64), 0, 0, D.d, A.view(), out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<uint32_t> o = to_host(out, 256);
    (void)hipFree(out);
    const std::vector<unsigned int> fired = to_host(D.d.fired, 16);
    const std::vector<unsigned long long> seen = to_host(D.d.seen, 16);
    for (uint32_t l = 0; l < 8; ++l)
        if (o[l] != hx::kScopeRoot) fail("lane %u: the promotion into a full arena returned %x", l, o[l]);
    if (o[64] != hx::kErrArena) fail("error word %u after it, want kErrArena (%u)", o[64], (uint32_t)hx::kErrArena);
    const uint32_t err = to_host(D.d.err, 1)[0];
    if (err != 0) fail("error word %u after the second promotion", err);
    if (o[65] != 8 || A.next() != 8) fail("the second promotion took %u ids for 4 chains of 2 scopes", o[65]);
    std::set<uint32_t> ids;
    for (uint32_t l = 0; l < 4; ++l)
        if (o[128 + l] >= 8 || !ids.insert(o[128 + l]).second) fail("lane %u: the second promotion returned %x", l, o[128 + l]);
    for (uint32_t l = 0; l < 8; ++l) {
        const unsigned long long inner = 100ull + l, outer = model_cont(8 + l, inner);
        if (fired[8 + l] != 1 || seen[8 + l] != inner) fail("inner scope %u: ran %u times, sum %llx", l, fired[8 + l], seen[8 + l]);
        if (fired[l] != 1 || seen[l] != outer) fail("outer scope %u: ran %u times, sum %llx, want %llx", l, fired[l], seen[l], outer);
    }
    // the eight promoted copies: closed, the inner ones under the outer ones' HBM copies
    const std::vector<hx::FinishScope> sc = to_host(A.scopes, 8);
    uint32_t inner_ok = 0, outer_ok = 0;
    for (uint32_t i = 0; i < 8; ++i) {
        if ((sc[i].word >> 56) != 0) fail("promoted id %u is not closed: %llx", i, sc[i].word);
        if (sc[i].cont < 4 && sc[i].parent == hx::kScopeRoot) ++outer_ok;
        if (sc[i].cont >= 8 && sc[i].cont < 12 && sc[i].parent < 8 && sc[sc[i].parent].cont == sc[i].cont - 8) ++inner_ok;
    }
    if (inner_ok != 4 || outer_ok != 4) fail("the promoted copies: %u outer, %u inner under their outer, want 4 and 4", outer_ok, inner_ok);
    if (to_host(D.d.ctr, C_N)[C_RAN] != 16) fail("%llu continuations reported, want 16", to_host(D.d.ctr, C_N)[C_RAN]);
    if (!A.guard_intact()) fail("the guard region behind the arena was written");
    if (g_form_fail) return false;
    printf("  %-44s -> kErrArena: every lane gets kScopeRoot; after a reset 4 chains take 8 ids, the failed round's marks "
           "are not taken up\n",
           g_what);
    return true;
}

// ---------------------------------------------------------------- the plan
static std::string join_counts(const std::set<uint32_t> &s) {
    std::string o;
    for (uint32_t c : s) o += (o.empty() ? "" : ",") + std::to_string(c);
    return o;
}
static void plan_line(const char *part, const char *form, const char *order, int n, const Forest &f) {
    printf("plan part=%s form=%s order=%s N=%d scopes=%u tasks=%u counts=%s chain=%u carry=%u masked=%u", part, form, order, n,
           f.nodes(), f.tasks(), join_counts(f.counts_present()).c_str(), f.deepest_unit_chain(), f.carry_scopes(),
           f.masked_leaves());
}

int main(int argc, char **argv) {
    bool plan = false, sched = true;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--plan")) plan = true;
        else if (!strcmp(argv[i], "--no-sched")) sched = false;
        else {
            fprintf(stderr, "usage: %s [--plan] [--no-sched]\n", argv[0]);
            return 2;
        }
    }
    const Forest fa = build_forest(0xF1A15Eull, 28, true, 3000, 40000);
    const Forest fb = build_forest(0xB0B0B0ull, kPartBWaves, false, 900, 12000);
    const Forest fk = build_contention();
    const Forest fc = build_forest(0xC0C0C0ull, 28, true, 6000, 20000);
    const PartBPlan pb = plan_part_b(fb, 0xB1ull, false), pk = plan_part_b(fk, 0xB2ull, true);
    if (plan) {
        for (const FormSpec &fs : kForms)
            for (int qd = 0; qd < 2; ++qd) {
                plan_line("A", fs.name, kOrders[qd], fs.n, fa);
                printf("\n");
            }
        plan_line("B", "B-two-kernels", "stack", 64, fb);
        printf(" waves=%u records=%u record_scopes=%u max_records=%u max_span=%u span255=%d\n", kPartBWaves, pb.nrec,
               pb.scopes_with_records, pb.max_records, pb.max_span, pb.min_span_255 == kNone ? 0 : (int)pb.min_span_255);
        plan_line("B", "B-contention", "none", 0, fk);
        printf(" waves=0 records=%u record_scopes=%u max_records=%u max_span=%u span255=%d\n", pk.nrec, pk.scopes_with_records,
               pk.max_records, pk.max_span, pk.min_span_255 == kNone ? 0 : (int)pk.min_span_255);
        plan_line("C", "C-scheduler-export", "scheduler", kWalkScopes, fc);
        printf("\n");
        return 0;
    }
    if (hclib_hip_init(0) != HCLIB_HIP_OK) {
        fprintf(stderr, "FAILED hclib_hip_init: %s\n", hclib_hip_last_error());
        return 1;
    }
    {
        DevForest D(fa, nullptr, 0, 1);
        for (const FormSpec &fs : kForms) {
            bool ok = true;
            for (int qd = 0; qd < 2; ++qd) {
                const std::string label = std::string(fs.name) + " " + kOrders[qd];
                ok = run_form(fa, D, fs, qd, label.c_str()) && ok;
            }
            if (ok) printf("%s OK\n", fs.name);
        }
        if (run_part_b_tree(fb, pb)) printf("B-two-kernels OK\n");
        if (run_part_b_contention(fk, pk)) printf("B-contention OK\n");
        if (sched && run_part_c(fc)) printf("C-scheduler-export OK\n");
        // the defined error returns, each followed by a clean run of form 1
        bool ok = limit_counts(false);
        ok = run_form(fa, D, kForms[0], 0, "form 1 after a bad count") && ok;
        ok = limit_counts(true) && ok;
        ok = run_form(fa, D, kForms[0], 1, "form 1 after a bad count (local)") && ok;
        ok = limit_arena_open() && ok;
        ok = run_form(fa, D, kForms[0], 0, "form 1 after kErrArena in finish_open") && ok;
        ok = limit_arena_promote() && ok;
        ok = run_form(fa, D, kForms[0], 1, "form 1 after kErrArena in finish_promote") && ok;
        if (ok) printf("limits OK\n");
    }
    if (g_fail) {
        printf("Check results: FAILED (%d checks)\n", g_fail);
        return 1;
    }
    printf("Check results: OK\n");
    return 0;
}
