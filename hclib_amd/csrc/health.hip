// health.hip — BOTS Health (test/performance-regression/full-apps/bots/health:
// health.ref.c the algorithm, health.c the HClib port) as an iterated
// fork-join client of dynamic device dataflow (include/hclib_hip/hx_dyn.h):
// sim_time rounds of sim_village_par over the village tree as ONE launch of
// run_dyn_worker, the full final state bit-identical to the reference's.
//
//   task                 does (health.ref.c lines)
//   CALL(v, t, fin)      a village's round t (:426-461). With children: f =
//                        open(children + 1), a CALL(child, t, f) per child into
//                        f, POST(v, t, fin) awaiting f, then the village's own
//                        check_patients_inside / _assess_par / _waiting
//                        (:445-451) while the children run, and a check-out of
//                        f. Without children: those three and check_patients_
//                        population (:460), then the continuation below.
//   POST(v, t, fin)      what follows the taskwait (:453-460): the children's
//                        outboxes merged by ascending patient id into
//                        put_in_hosp (check_patients_realloc), check_patients_
//                        population, then the continuation
//   continuation         a check-out of fin (the parent's scope); the root has
//                        none (fin = kDynOpen) and creates CALL(root, t + 1)
//                        while t + 1 < sim_time (sim_village_main_par's loop)
//
// Data. A patient is its id: four int32 record words per patient (seed, time,
// time_left, hosps_visited) that never move. A list is an array of ids in the
// village's segment of one arena, and a length. A village of level l whose
// subtree holds P(l) patients has [population P(l)][waiting P(l)][assess 2^l]
// [inside 2^l][outbox 2^l]: patients only move upward, and free_personnel =
// 2^l - |assess| - |inside| >= 0 bounds the last three. The
// outbox holds what the village's assess step sends up this round; the parent's
// POST reads it after the scope has closed, which replaces the reference's
// write into the parent's realloc list and its lock. Villages are indexed in
// the reference's allocation order (a village, then its children cities .. 1
// with their subtrees), patients are numbered in it (sim_pid).
//
// Bodies are wave-wide: a list is walked 64 ids at a time, a ballot and a lane
// prefix count give every patient that leaves its place at the destination's
// tail and every one that stays its place in the compacted list, in source
// order. Compaction is in place: a chunk is in registers before anything is
// stored, and the write index never passes the read index. The free_personnel
// updates are prefix sums: the first min(free, n) of a sequence get staff.
//
// Memory protocol: lists, lengths and records are plain stores and plain
// loads. Every task ends with a release at agent scope ahead of the atomic that
// passes its work on (dyn_finish_check_out<false>, dyn_async_await<false>), and
// run_dyn_worker acquires at agent scope after it has read the task's ready
// slot and before the body (kSc1Payload = false). Round t + 1 of a village is
// ordered after its round t by the chain check-out .. POST(root, t) ->
// CALL(root, t + 1) -> CALL(child, t + 1), a release and an acquire on every
// link.
#include <string.h>

#include <vector>

#include "hx_client.h"

namespace hx {
namespace {

constexpr int kHlWords = 4;            // payload: {kind, village, round, fin}
constexpr int kHlMaxWavesPerCu = 8;    // 8 x 8 KB of LDS per CU
constexpr uint32_t kHlMergeMax = 2048; // ids one POST can merge in LDS: cities * 2^(level - 1) at the root
constexpr int kHlMaxLevel = 24;
enum : uint32_t { kHlCall = 0, kHlPost = 1 };
enum : int { kCntLeaf = 0, kCntInner = 1, kCntPost = 2, kCntKinds = 3 };
// per village, read-only: 8 words
enum : int { kVdLevel = 0, kVdSeg = 1, kVdChild0 = 2, kVdChildStride = 3, kVdSub = 4, kVdWords = 8 };
// per village, mutable: the five lengths and free_personnel, 8 words
enum : int { kVsPop = 0, kVsWait = 1, kVsAssess = 2, kVsInside = 3, kVsOut = 4, kVsFree = 5, kVsWords = 8 };

constexpr int32_t kIA = 16807, kIM = 2147483647, kIQ = 127773, kIR = 2836, kMask = 123459876;

struct HlCtx {
    int32_t *seed, *time, *time_left, *visits;  // per patient
    uint32_t *lists;                            // the arena of ids
    uint32_t *vs;                               // per village kVsWords
    const uint32_t *vd;                         // per village kVdWords
    unsigned long long *counts;                 // per task class (hx_client.h class_count)
    uint32_t villages, patients, list_words, cities, level, sim_time;
    int32_t assess_time, conv_time;
    float sick_p, conv_p, realloc_p;
};

// my_rand (:88-100) on words that wrap; the value is (float)AM * idum, one
// conversion and one f32 multiply by 2^-31
__host__ __device__ inline float hl_rand(int32_t &seed) {
    int32_t idum = seed ^ kMask;
    const int32_t k = idum / kIQ;
    idum = (int32_t)((uint32_t)kIA * (uint32_t)(idum - k * kIQ) - (uint32_t)kIR * (uint32_t)k);
    idum ^= kMask;
    if (idum < 0) idum = (int32_t)((uint32_t)idum + (uint32_t)kIM);
    seed = (int32_t)((uint32_t)idum * (uint32_t)kIM);
    return (float)(1.0 / 2147483647) * (float)idum;
}

__device__ __forceinline__ uint32_t hl_prefix(unsigned long long m) {
    return (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ uint32_t hl_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// one village's lists and lengths, in registers for the length of a task
struct HlVillage {
    uint32_t *pop, *wait, *assess, *inside, *out;
    uint32_t npop, nwait, nassess, ninside, nout, free;
    uint32_t sub, staff;  // capacities: population and waiting hold `sub`, the others `staff`
    bool ok;
};

__device__ __forceinline__ HlVillage hl_open(const HlCtx &c, uint32_t v) {
    HlVillage h;
    const uint32_t *d = c.vd + (size_t)v * kVdWords;
    const uint32_t level = hl_uniform(d[kVdLevel]), seg = hl_uniform(d[kVdSeg]);
    h.sub = hl_uniform(d[kVdSub]);
    h.staff = level < 31 ? 1u << level : 0u;
    h.ok = h.staff && (unsigned long long)seg + 2ull * h.sub + 3ull * h.staff <= c.list_words;
    h.pop = c.lists + seg;
    h.wait = h.pop + h.sub;
    h.assess = h.wait + h.sub;
    h.inside = h.assess + h.staff;
    h.out = h.inside + h.staff;
    const uint32_t *s = c.vs + (size_t)v * kVsWords;
    h.npop = hl_uniform(s[kVsPop]), h.nwait = hl_uniform(s[kVsWait]), h.nassess = hl_uniform(s[kVsAssess]);
    h.ninside = hl_uniform(s[kVsInside]), h.nout = hl_uniform(s[kVsOut]), h.free = hl_uniform(s[kVsFree]);
    h.ok = h.ok && h.npop <= h.sub && h.nwait <= h.sub && h.nassess <= h.staff && h.ninside <= h.staff &&
           h.nout <= h.staff && h.free <= h.staff;
    return h;
}

__device__ __forceinline__ void hl_close(const HlCtx &c, uint32_t v, const HlVillage &h) {
    if (lane_id() == 0) {
        uint32_t *s = c.vs + (size_t)v * kVsWords;
        s[kVsPop] = h.npop, s[kVsWait] = h.nwait, s[kVsAssess] = h.nassess, s[kVsInside] = h.ninside;
        s[kVsOut] = h.nout, s[kVsFree] = h.free;
    }
}

// an id read from a list, checked: a lane with a bad id takes no part (device error)
__device__ __forceinline__ bool hl_load(const HlCtx &c, DynWave &w, const uint32_t *list, uint32_t i, uint32_t n,
                                        uint32_t &id) {
    id = 0;
    if (i >= n) return false;
    id = list[i];
    if (id < c.patients) return true;
    dev_error(dyn_err(w.v), kErrBadTask);
    return false;
}

// room for k more ids in a list of n with capacity cap (wave-uniform); a list that would overflow is a device error
__device__ __forceinline__ bool hl_room(DynWave &w, uint32_t n, uint32_t k, uint32_t cap) {
    if (n + k <= cap) return true;
    if (lane_id() == 0) dev_error(dyn_err(w.v), kErrArena);
    return false;
}

// check_patients_inside (:280-297): time_left--, at 0 to the tail of population
__device__ __forceinline__ void hl_inside(const HlCtx &c, DynWave &w, HlVillage &h) {
    const uint32_t lane = (uint32_t)lane_id(), n = h.ninside;
    uint32_t kept = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        uint32_t id;
        const bool act = hl_load(c, w, h.inside, i0 + lane, n, id);
        int32_t left = 0;
        if (act) c.time_left[id] = left = c.time_left[id] - 1;
        const bool go = act && left == 0, stay = act && !go;
        const unsigned long long mgo = __ballot(go), mstay = __ballot(stay);
        const uint32_t ngo = (uint32_t)__popcll(mgo);
        const bool room = hl_room(w, h.npop, ngo, h.sub);
        if (stay) h.inside[kept + hl_prefix(mstay)] = id;
        if (go && room) h.pop[h.npop + hl_prefix(mgo)] = id;
        kept += (uint32_t)__popcll(mstay);
        if (room) h.npop += ngo;
        h.free += ngo;
    }
    h.ninside = kept;
}

// check_patients_assess_par (:299-345): time_left--, at 0 one draw: home (population), or a second draw: inside,
// or up (the outbox). Four ways: stay, inside, population, outbox
__device__ __forceinline__ void hl_assess(const HlCtx &c, DynWave &w, HlVillage &h, bool is_root) {
    const uint32_t lane = (uint32_t)lane_id(), n = h.nassess;
    uint32_t kept = 0;
    h.nout = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        uint32_t id;
        const bool act = hl_load(c, w, h.assess, i0 + lane, n, id);
        int32_t left = 0;
        if (act) c.time_left[id] = left = c.time_left[id] - 1;
        const bool done = act && left == 0;
        bool in = false, home = false, up = false;
        if (done) {
            int32_t s = c.seed[id];
            if (hl_rand(s) < c.conv_p) {
                in = hl_rand(s) > c.realloc_p || is_root;
                up = !in;
            } else {
                home = true;
            }
            c.seed[id] = s;
            if (in) {
                c.time_left[id] = c.conv_time;
                c.time[id] += c.conv_time;
            }
        }
        const bool stay = act && !done;
        const unsigned long long mstay = __ballot(stay), min = __ballot(in), mhome = __ballot(home), mup = __ballot(up);
        const uint32_t nin = (uint32_t)__popcll(min), nhome = (uint32_t)__popcll(mhome), nup = (uint32_t)__popcll(mup);
        const bool rin = hl_room(w, h.ninside, nin, h.staff), rhome = hl_room(w, h.npop, nhome, h.sub),
                   rup = hl_room(w, h.nout, nup, h.staff);
        if (stay) h.assess[kept + hl_prefix(mstay)] = id;
        if (in && rin) h.inside[h.ninside + hl_prefix(min)] = id;
        if (home && rhome) h.pop[h.npop + hl_prefix(mhome)] = id;
        if (up && rup) h.out[h.nout + hl_prefix(mup)] = id;
        kept += (uint32_t)__popcll(mstay);
        if (rin) h.ninside += nin;
        if (rhome) h.npop += nhome;
        if (rup) h.nout += nup;
        h.free += nhome + nup;
    }
    h.nassess = kept;
}

// check_patients_waiting (:347-369): the first min(free, n) to the tail of assess, time++ for the others
__device__ __forceinline__ void hl_waiting(const HlCtx &c, DynWave &w, HlVillage &h) {
    const uint32_t lane = (uint32_t)lane_id(), n = h.nwait;
    const uint32_t take = h.free < n ? h.free : n;
    if (!hl_room(w, h.nassess, take, h.staff)) return;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        uint32_t id;
        const bool act = hl_load(c, w, h.wait, i, n, id);
        __builtin_amdgcn_wave_barrier();  // (the chunk is loaded before any lane stores below it)
        if (act && i < take) {
            c.time_left[id] = c.assess_time;
            c.time[id] += c.assess_time;
            h.assess[h.nassess + i] = id;
        } else if (act) {
            c.time[id] += 1;
            h.wait[i - take] = id;
        }
    }
    h.nassess += take;
    h.nwait = n - take;
    h.free -= take;
}

// put_in_hosp (:409-424) for the patient of rank `rank` in a sequence that meets `free` free staff: the first `free`
// to the tail of assess, the others to the tail of waiting (wave-uniform h, per-lane id and rank)
__device__ __forceinline__ void hl_put(const HlCtx &c, const HlVillage &h, uint32_t id, uint32_t rank, uint32_t free) {
    c.visits[id] += 1;
    if (rank < free) {
        h.assess[h.nassess + rank] = id;
        c.time_left[id] = c.assess_time;
        c.time[id] += c.assess_time;
    } else {
        h.wait[h.nwait + rank - free] = id;
    }
}

__device__ __forceinline__ uint32_t *hl_lds() {
    __shared__ uint32_t s[kHlMergeMax];
    return s;
}

// check_patients_realloc (:371-386): the children's outboxes in ascending patient id. The ids are distinct, so a
// patient's rank among them is the count of smaller ids, and the rank is its place in the sequence put_in_hosp sees
__device__ __forceinline__ void hl_realloc(const HlCtx &c, DynWave &w, uint32_t v, HlVillage &h) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t *d = c.vd + (size_t)v * kVdWords;
    const uint32_t child0 = hl_uniform(d[kVdChild0]), stride = hl_uniform(d[kVdChildStride]);
    uint32_t *ids = hl_lds();
    uint32_t m = 0;
    for (uint32_t k = 0; k < c.cities; ++k) {
        const unsigned long long cv = (unsigned long long)child0 + (unsigned long long)k * stride;
        if (cv >= c.villages) {
            if (lane == 0) dev_error(dyn_err(w.v), kErrBadTask);
            return;
        }
        const HlVillage ch = hl_open(c, (uint32_t)cv);
        if (!ch.ok || m + ch.nout > kHlMergeMax) {
            if (lane == 0) dev_error(dyn_err(w.v), kErrArena);
            return;
        }
        for (uint32_t i0 = 0; i0 < ch.nout; i0 += 64) {
            uint32_t id;
            const bool act = hl_load(c, w, ch.out, i0 + lane, ch.nout, id);
            if (i0 + lane < ch.nout) ids[m + i0 + lane] = act ? id : 0u;
        }
        m += ch.nout;
    }
    if (!m) return;
    __syncthreads();
    const uint32_t take = h.free < m ? h.free : m;
    if (!hl_room(w, h.nassess, take, h.staff) || !hl_room(w, h.nwait, m - take, h.sub)) return;
    for (uint32_t i0 = 0; i0 < m; i0 += 64) {
        const bool act = i0 + lane < m;
        const uint32_t id = act ? ids[i0 + lane] : 0u;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < m; ++j) rank += ids[j] < id ? 1u : 0u;
        if (act) hl_put(c, h, id, rank, take);
    }
    h.nassess += take;
    h.nwait += m - take;
    h.free -= take;
    __syncthreads();  // the next merge overwrites the LDS
}

// check_patients_population (:388-407): one draw each, the sick to put_in_hosp in order
__device__ __forceinline__ void hl_population(const HlCtx &c, DynWave &w, HlVillage &h) {
    const uint32_t lane = (uint32_t)lane_id(), n = h.npop;
    uint32_t kept = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        uint32_t id;
        const bool act = hl_load(c, w, h.pop, i0 + lane, n, id);
        bool sick = false;
        if (act) {
            int32_t s = c.seed[id];
            sick = hl_rand(s) < c.sick_p;
            c.seed[id] = s;
        }
        const unsigned long long msick = __ballot(sick), mstay = __ballot(act && !sick);
        const uint32_t nsick = (uint32_t)__popcll(msick), take = h.free < nsick ? h.free : nsick;
        const bool room = hl_room(w, h.nassess, take, h.staff) && hl_room(w, h.nwait, nsick - take, h.sub);
        if (act && !sick) h.pop[kept + hl_prefix(mstay)] = id;
        if (sick && room) hl_put(c, h, id, hl_prefix(msick), take);
        kept += (uint32_t)__popcll(mstay);
        if (room) {
            h.nassess += take;
            h.nwait += nsick - take;
            h.free -= take;
        }
    }
    h.npop = kept;
}

struct HlKind : TimedKind<HlKind, HlCtx> {
    using Ctx = HlCtx;
    static constexpr bool kSc1Payload = false;  // lists and records move by plain loads behind the worker's acquire
    __device__ static void bad(DynWave &w) {
        if (lane_id() == 0) dev_error(dyn_err(w.v), kErrBadTask);
    }
    // what follows a village's round: out of the parent's scope, or the root's next round
    __device__ static void next(const Ctx &c, DynWave &w, uint32_t v, uint32_t t, uint32_t fin) {
        if (fin != kDynOpen) {
            dyn_finish_check_out<false>(w, fin);
        } else if (t + 1 < c.sim_time) {
            const uint32_t pl[kHlWords] = {kHlCall, v, t + 1, kDynOpen};
            dyn_async_await<false>(w, lane_id() == 0, pl, nullptr, 0);
        }
    }
    __device__ static void body(const Ctx &c, DynWave &w, const uint32_t *pay, int &which) {
        const uint32_t kind = pay[0], v = pay[1], t = pay[2], fin = pay[3];
        const uint32_t lane = (uint32_t)lane_id();
        if (kind > kHlPost || v >= c.villages || t >= c.sim_time) return bad(w);
        HlVillage h = hl_open(c, v);
        if (!h.ok) return bad(w);
        const uint32_t *d = c.vd + (size_t)v * kVdWords;
        const uint32_t level = hl_uniform(d[kVdLevel]);
        const bool inner = level > 1;
        if (kind == kHlPost) {
            if (!inner) return bad(w);
            which = kCntPost;
            hl_realloc(c, w, v, h);
            hl_population(c, w, h);
            hl_close(c, v, h);
            return next(c, w, v, t, fin);
        }
        if (!inner) {
            which = kCntLeaf;
            hl_inside(c, w, h);
            hl_assess(c, w, h, level == c.level);
            hl_waiting(c, w, h);
            hl_population(c, w, h);
            hl_close(c, v, h);
            return next(c, w, v, t, fin);
        }
        which = kCntInner;
        const uint32_t f = dyn_finish_open(w, c.cities + 1);
        if (f == kDynOpen) return;
        const uint32_t child0 = hl_uniform(d[kVdChild0]), stride = hl_uniform(d[kVdChildStride]);
        for (uint32_t k0 = 0; k0 < c.cities; k0 += 64) {
            const uint32_t k = k0 + lane;
            const uint32_t pl[kHlWords] = {kHlCall, child0 + k * stride, t, f};
            dyn_async_await<true>(w, k < c.cities, pl, nullptr, 0);  // (nothing the children read was written here)
        }
        const uint32_t pl[kHlWords] = {kHlPost, v, t, fin};
        const uint32_t fut[1] = {f};
        dyn_async_await<true>(w, lane == 0, pl, fut, 1);
        hl_inside(c, w, h);
        hl_assess(c, w, h, level == c.level);
        hl_waiting(c, w, h);
        hl_close(c, v, h);
        dyn_finish_check_out<false>(w, f);
    }
};

__global__ __launch_bounds__(64) void k_health(HlCtx c, DynView v) { run_dyn_worker<HlKind>(c, v); }

ClassCounters<kCntKinds> g_hl;  // the last launch's

// Everything a launch allocates is a closed form of the settings.
struct HlPlan {
    unsigned long long villages = 0, inner = 0, patients = 0, tasks = 0, scopes = 0, nodes = 0, list_words = 0, bytes = 0;
    unsigned long long sub[kHlMaxLevel + 1] = {};    // P(l): the population of a subtree of level l
    unsigned long long size[kHlMaxLevel + 1] = {};   // villages of a subtree of level l
    unsigned long long words[kHlMaxLevel + 1] = {};  // list words of a subtree of level l
};

int hl_plan(const char *who, const hclib_hip_health_params_t *p, HlPlan &pl) {
    if (!p) {
        set_error("%s: params must not be NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    if (p->level < 1 || p->cities < 1 || p->population_ratio < 1 || p->sim_time < 0) {
        set_error("%s: level = %d, cities = %d, population_ratio = %d must be at least 1 and sim_time = %d at least 0", who,
                  p->level, p->cities, p->population_ratio, p->sim_time);
        return HCLIB_HIP_EINVAL;
    }
    if (p->assess_time < 1 || p->convalescence_time < 1) {
        set_error("%s: assess_time = %d and convalescence_time = %d must be at least 1 (a zero makes time_left step past "
                  "zero and never return)", who, p->assess_time, p->convalescence_time);
        return HCLIB_HIP_EINVAL;
    }
    const float pr[3] = {p->get_sick_p, p->convalescence_p, p->realloc_p};
    for (int k = 0; k < 3; ++k)
        if (!(pr[k] >= 0.0f && pr[k] <= 1.0f)) {
            set_error("%s: probability %d = %g must lie in [0, 1]", who, k, (double)pr[k]);
            return HCLIB_HIP_EINVAL;
        }
    const unsigned long long limit = 1ull << 31, c = (unsigned long long)p->cities;
    bool fits = p->level <= kHlMaxLevel;
    for (int l = 1; fits && l <= p->level; ++l) {
        const unsigned long long staff = 1ull << l;
        pl.sub[l] = c * pl.sub[l - 1] + staff * (unsigned long long)p->population_ratio;
        pl.size[l] = c * pl.size[l - 1] + 1;
        pl.words[l] = c * pl.words[l - 1] + 2 * pl.sub[l] + 3 * staff;
        fits = pl.sub[l] < limit && pl.size[l] < limit && pl.words[l] < 2 * limit;
    }
    if (fits) {
        pl.villages = pl.size[p->level];
        pl.inner = pl.size[p->level - 1];
        pl.patients = pl.sub[p->level];
        pl.list_words = pl.words[p->level];
        const unsigned long long t = (unsigned long long)p->sim_time;
        pl.tasks = t * (pl.villages + pl.inner);
        pl.scopes = pl.nodes = t * pl.inner;
        fits = pl.tasks < 0xfffffff0ull;
    }
    if (!fits) {
        set_error("%s: level = %d, cities = %d, population_ratio = %d, sim_time = %d need villages, patients, list words "
                  "or tasks that a 32-bit index cannot address (at most 2^31 villages and patients, 2^32 - 17 tasks, "
                  "level <= %d)", who, p->level, p->cities, p->population_ratio, p->sim_time, kHlMaxLevel);
        return HCLIB_HIP_EINVAL;
    }
    if (p->level > 1 && c * (1ull << (p->level - 1)) > kHlMergeMax) {
        set_error("%s: a village's merge of its children's patients is sorted in LDS: cities * 2^(level - 1) = %llu must "
                  "be at most %u", who, c * (1ull << (p->level - 1)), kHlMergeMax);
        return HCLIB_HIP_EINVAL;
    }
    pl.bytes = g_hl.kBytes + 4ull * ((kVdWords + kVsWords) * pl.villages + 4 * pl.patients + pl.list_words);
    return HCLIB_HIP_OK;
}

// The initial state (allocate_village, :143-195), in allocation order.
struct HlHost {
    std::vector<uint32_t> vd, vs, lists;
    std::vector<int32_t> rec[4], vid;
};

void hl_alloc(const hclib_hip_health_params_t &p, const HlPlan &pl, HlHost &h, int level, uint32_t vid, uint32_t &seg) {
    const uint32_t me = (uint32_t)h.vid.size(), staff = 1u << level, pop = staff * (uint32_t)p.population_ratio;
    h.vid.push_back((int32_t)vid);
    uint32_t *d = &h.vd[(size_t)me * kVdWords], *s = &h.vs[(size_t)me * kVsWords];
    d[kVdLevel] = (uint32_t)level, d[kVdSeg] = seg, d[kVdChild0] = me + 1, d[kVdChildStride] = (uint32_t)pl.size[level - 1];
    d[kVdSub] = (uint32_t)pl.sub[level];
    s[kVsPop] = pop, s[kVsFree] = staff;
    int32_t seed = (int32_t)(vid * ((uint32_t)kIQ + (uint32_t)p.seed));
    for (uint32_t k = 0; k < pop; ++k) {
        h.lists[seg + k] = (uint32_t)h.rec[0].size();
        h.rec[0].push_back(seed);
        (void)hl_rand(seed);
    }
    seg += 2 * (uint32_t)pl.sub[level] + 3 * staff;
    if (level > 1)
        for (uint32_t i = (uint32_t)p.cities; i > 0; --i) hl_alloc(p, pl, h, level - 1, vid * (uint32_t)p.cities + i, seg);
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_health_bounds(const hclib_hip_health_params_t *params, uint64_t out[6]) {
    if (!out) {
        set_error("hclib_hip_health_bounds: out must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    HlPlan pl;
    HX_TRY(hl_plan("hclib_hip_health_bounds", params, pl));
    out[0] = pl.villages, out[1] = pl.patients, out[2] = pl.tasks, out[3] = pl.scopes, out[4] = pl.nodes;
    out[5] = pl.bytes;
    return HCLIB_HIP_OK;
}

extern "C" void hclib_hip_health_last_ticks(uint64_t out[3]) {
    for (int k = 0; k < kCntKinds; ++k) out[k] = g_hl.ticks[k];
}

extern "C" int hclib_hip_health(const hclib_hip_health_params_t *params, hclib_hip_health_result_t *result,
                                hclib_hip_health_state_t *state) {
    // argument errors first, before the device is touched
    if (!result) {
        set_error("hclib_hip_health: result must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    HlPlan pl;
    HX_TRY(hl_plan("hclib_hip_health", params, pl));
    if (state && !(state->seed && state->time && state->time_left && state->hosps_visited && state->village &&
                   state->lists)) {
        set_error("hclib_hip_health: every array of state must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    HX_TRY(ensure_device());
    Module &m = mod();
    const hclib_hip_health_params_t &p = *params;
    const size_t V = (size_t)pl.villages, P = (size_t)pl.patients, L = (size_t)pl.list_words;

    HlHost h;
    h.vd.assign(V * kVdWords, 0), h.vs.assign(V * kVsWords, 0), h.lists.assign(L, 0);
    h.rec[0].reserve(P);
    uint32_t seg = 0;
    hl_alloc(p, pl, h, p.level, 0u, seg);
    for (int k = 1; k < 4; ++k) h.rec[k].assign(P, 0);

    // [counts: a line per task class][village descriptors][village lengths][seed][time][time_left][visits][lists]
    char *d = nullptr;
    if (const int rc = arena_reserve(kArenaHealth, (size_t)pl.bytes, "hclib_hip_health", (void **)&d)) {
        set_error("hclib_hip_health: hipMalloc(%llu) failed (%llu villages, %llu patients)", pl.bytes, pl.villages,
                  pl.patients);
        return rc;
    }
    HlCtx cx;
    cx.counts = (unsigned long long *)d;
    uint32_t *w32 = (uint32_t *)(d + g_hl.kBytes);
    cx.vd = w32;
    cx.vs = w32 + V * kVdWords;
    cx.seed = (int32_t *)(cx.vs + V * kVsWords);
    cx.time = cx.seed + P, cx.time_left = cx.time + P, cx.visits = cx.time_left + P;
    cx.lists = (uint32_t *)(cx.visits + P);
    cx.villages = (uint32_t)V, cx.patients = (uint32_t)P, cx.list_words = (uint32_t)L;
    cx.cities = (uint32_t)p.cities, cx.level = (uint32_t)p.level, cx.sim_time = (uint32_t)p.sim_time;
    cx.assess_time = p.assess_time, cx.conv_time = p.convalescence_time;
    cx.sick_p = p.get_sick_p, cx.conv_p = p.convalescence_p, cx.realloc_p = p.realloc_p;
    // (the host vectors outlive the copies: every path below synchronises the stream)
    HX_HIP(hipMemcpyAsync((void *)cx.vd, h.vd.data(), V * kVdWords * 4, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(cx.vs, h.vs.data(), V * kVsWords * 4, hipMemcpyHostToDevice, m.stream));
    for (int k = 0; k < 4; ++k)
        HX_HIP(hipMemcpyAsync(cx.seed + (size_t)k * P, h.rec[k].data(), P * 4, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(cx.lists, h.lists.data(), L * 4, hipMemcpyHostToDevice, m.stream));

    memset(result, 0, sizeof(*result));
    hclib_hip_dyn_stats_t st{};
    uint64_t fin[2] = {0, 0};
    int rc = HCLIB_HIP_OK;
    if (p.sim_time > 0) {
        const uint32_t root[kHlWords] = {kHlCall, 0u, 0u, kDynOpen};
        // (HCLIB_HIP_HEALTH_WAVES_PER_CU: for measurements and the schedule-independence test)
        int wpc = env_int("HCLIB_HIP_HEALTH_WAVES_PER_CU", 1);
        wpc = wpc < 1 ? 1 : (wpc > kHlMaxWavesPerCu ? kHlMaxWavesPerCu : wpc);
        rc = launch_dyn(kHlWords, root, pl.tasks, pl.scopes, pl.nodes, wpc, "hclib_hip_health", d, g_hl, &st, fin,
                        [&](int grid, const DynView &v) {
                            hipLaunchKernelGGL(k_health, dim3(grid), dim3(64), 0, m.stream, cx, v);
                        });
    } else {
        g_hl = ClassCounters<kCntKinds>();
        HX_HIP(hipStreamSynchronize(m.stream));
    }
    result->tasks = st.tasks;
    result->finishes = fin[0];
    // tasks checked in to scopes: children + 1 at every open, and what dyn_finish_check_in added (nothing here)
    result->check_ins = g_hl.tasks[kCntInner] * ((uint64_t)p.cities + 1) + fin[1];
    result->leaf_calls = g_hl.tasks[kCntLeaf];
    result->inner_calls = g_hl.tasks[kCntInner];
    result->posts = g_hl.tasks[kCntPost];
    result->kernel_ms = st.kernel_ms;
    result->rounds_per_s = st.kernel_ms > 0 ? p.sim_time / (st.kernel_ms * 1e-3) : 0.0;
    if (rc) return rc;

    HX_HIP(hipMemcpy(h.vs.data(), cx.vs, V * kVsWords * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) HX_HIP(hipMemcpy(h.rec[k].data(), cx.seed + (size_t)k * P, P * 4, hipMemcpyDeviceToHost));
    HX_HIP(hipMemcpy(h.lists.data(), cx.lists, L * 4, hipMemcpyDeviceToHost));
    // get_results (:197-276), and the state in village order
    size_t at = 0;
    for (size_t v = 0; v < V; ++v) {
        const uint32_t *dsc = &h.vd[v * kVdWords], *s = &h.vs[v * kVsWords];
        const uint32_t staff = 1u << dsc[kVdLevel], sub = dsc[kVdSub];
        const uint32_t off[4] = {dsc[kVdSeg], dsc[kVdSeg] + sub, dsc[kVdSeg] + 2 * sub, dsc[kVdSeg] + 2 * sub + staff};
        const uint32_t cap[4] = {sub, sub, staff, staff};
        int64_t *where[4] = {&result->in_village, &result->waiting, &result->assess, &result->inside};
        result->hospitals += 1;
        result->personnel += staff;
        if (state) {
            int32_t *row = state->village + v * 7;
            row[0] = h.vid[v], row[1] = (int32_t)dsc[kVdLevel], row[2] = (int32_t)s[kVsFree];
            for (int k = 0; k < 4; ++k) row[3 + k] = (int32_t)s[k];
        }
        for (int k = 0; k < 4; ++k) {
            if (s[k] > cap[k] || at + s[k] > P) {
                set_error("hclib_hip_health: village %zu came back with a list of %u patients", v, s[k]);
                return HCLIB_HIP_EDEVICE;
            }
            *where[k] += s[k];
            result->population += s[k];
            for (uint32_t i = 0; i < s[k]; ++i) {
                const uint32_t id = h.lists[off[k] + i];
                if (id >= P) {
                    set_error("hclib_hip_health: village %zu came back with patient id %u", v, id);
                    return HCLIB_HIP_EDEVICE;
                }
                result->hosps_visited += h.rec[3][id];
                result->total_time += h.rec[1][id];
                if (state) state->lists[at + i] = (int32_t)id;
            }
            at += s[k];
        }
    }
    if (at != P) {
        set_error("hclib_hip_health: %zu of %zu patients are in a list", at, P);
        return HCLIB_HIP_EDEVICE;
    }
    if (state) {
        int32_t *dst[4] = {state->seed, state->time, state->time_left, state->hosps_visited};
        for (int k = 0; k < 4; ++k) memcpy(dst[k], h.rec[k].data(), P * 4);
    }
    return HCLIB_HIP_OK;
}
