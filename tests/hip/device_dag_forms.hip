// Every put form of the device promise DAG (include/hclib_hip/hx_dag.h) through
// hclib::hip::dag + run_dag / run_dag_groups, each against a serial host
// evaluation of the same graph.
//
// Forms (one Kind each):
//   W-putn<N,SC1>  run_dag_worker, the body calls dag_put_n<N, SC1>   N = 1, 3, 8
//   G0<N>          run_dag_group with put() (no kPutN): dag_put per promise
//   G1-sc1<N>      kPutN = N, kSc1Payload = true   (the plain split put)
//   G1-plain<N>    kPutN = N, kSc1Payload = false  (plain stores and loads)
//   G3<N>          kTagged without kReserve
//   G4<3>          kTagged + kReserve (N = 1 is device_dag.hip's ReserveKind)
//
// A task's value is a chain of mix() over its own id and the values behind
// the promises it awaits, in await order, so a missing, early or duplicated
// release changes it. Every task publishes {1 << 32 | value} in its output
// word and {index << 40 | 1 << 32 | value} as the datum of each of its N
// promises. W-putn and G0 read each input through dag_get of the datum and
// through the producer's output word and compare the two; the other
// workgroup Kinds have no DagWave in their bodies and read the output words
// (the tagged ones poll them). A missing tag counts as a stale read.
//
// Graphs (seeded, 1,000 to 6,000 tasks, the same for every form of one N):
//   ladder     rungs whose promises have 0, 1, 2, 63, 64, 65, 127, 128, 129
//              and 200 waiter entries in total, in two splits over the N
//              promises, and for N = 3 the splits {20,0,44} {1,63,1} {0,0,64}
//              {64,1,0} {30,30,3} {0,0,0}; the first waiter of a list awaits
//              its promise twice;
//   random     3,000 tasks awaiting 0..8 earlier promises, some twice, some
//              put before the launch, a few hub promises with long lists;
//   chain-fan  device_dag.hip's reserved-slot shape (a 200-waiter root, then
//              a 300-long chain in which every released task is the kept
//              one), five times side by side.
//
// Errors (designed error returns, nothing written outside the arrays): a
// second put on a short-list and on a long-list promise, a task awaiting a
// promise nothing puts; each followed by a clean launch.
//
// --plan builds every graph and prints, per (form, graph), how many puts take
// the short and the long branch, without any HIP call.
// Prints "Check results: OK" (tests/test_dag_forms_gpu.py).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "hclib_hip_cpp.h"

#define CHECK(c, ...)                                              \
    do {                                                           \
        if (!(c)) {                                                \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                          \
            fprintf(stderr, "\n");                                 \
            exit(1);                                               \
        }                                                          \
    } while (0)

typedef unsigned long long u64;

__host__ __device__ inline u64 mix(u64 x) {  // splitmix64 finaliser
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

constexpr uint32_t kNone = 0xffffffffu;
constexpr int kMaxAwaits = 8;
constexpr int kAwWords = 1 + kMaxAwaits;  // {k, p0..p7} per task
constexpr u64 kTag = 1ull << 32;

// ------------------------------------------------------------ device side
struct FormCtx {
    const uint32_t *aw;  // [T * kAwWords] the awaits of every task
    u64 *out;            // [T + extra] tagged output words; [T, ..) the promises put before the launch
    unsigned *bad;       // stale or untagged reads
    uint32_t T, N;
    uint32_t dbl_task, dbl_promise;  // the task whose promise 0 is dbl_promise instead (a second put), or kNone
};

enum { kPlain = 0, kSc1 = 1, kPoll = 2 };

__device__ inline u64 wait_tag(const u64 *p) {
    u64 v = 0;
    const u64 t0 = __builtin_amdgcn_s_memrealtime();
    while (((v = hx::ld_agent(p)) >> 32) == 0 && __builtin_amdgcn_s_memrealtime() - t0 < 100000000ull)
        __builtin_amdgcn_s_sleep(1);
    return v;
}

// The task's output word, from its inputs (wave-uniform). MODE: how another
// task's output word is read. w: the DagWave, where the body has one.
template <int MODE>
__device__ inline u64 task_word(const FormCtx &c, uint32_t t, const hx::DagWave *w) {
    const uint32_t *a = c.aw + (size_t)t * kAwWords;
    const uint32_t k = a[0], NT = c.N * c.T;
    u64 acc = mix(t);
    unsigned nbad = 0;
    for (uint32_t q = 0; q < k && q < (uint32_t)kMaxAwaits; ++q) {
        const uint32_t p = a[1 + q];
        const uint32_t src = p < NT ? p / c.N : c.T + (p - NT);
        u64 word;
        if (MODE == kPlain) word = c.out[src];
        else if (MODE == kSc1) word = hx::ld_agent(&c.out[src]);
        else word = wait_tag(&c.out[src]);
        if ((word >> 32) != 1) ++nbad;
        if (w) {
            const u64 index = p < NT ? (u64)(p - src * c.N) << 40 : 0;
            if (hx::dag_get(*w, p) != (word | index)) ++nbad;
            if (!hx::dag_is_satisfied(*w, p)) ++nbad;
        }
        acc = mix(acc ^ (u64)(uint32_t)word);
    }
    if (nbad && hx::lane_id() == 0) atomicAdd(c.bad, nbad);
    return kTag | (uint32_t)acc;
}

template <int N>
__device__ inline void form_promises(const FormCtx &c, uint32_t t, uint32_t (&p)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = (uint32_t)N * t + (uint32_t)i;
    if (t == c.dbl_task) p[0] = c.dbl_promise;
}
template <int N>
__device__ inline void form_datums(u64 word, u64 (&d)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = word | ((u64)i << 40);
}

// W-putn<N, SC1>
template <int N, bool SC1>
struct WKind {
    using Ctx = FormCtx;
    __device__ static void run(const Ctx &c, hx::DagWave &w, uint32_t t, const uint32_t *pl) {
        if (pl[0] != t && hx::lane_id() == 0) atomicAdd(c.bad, 1u);
        const u64 word = task_word<SC1 ? kSc1 : kPlain>(c, t, &w);
        if (hx::lane_id() == 0) {
            if (SC1) hx::st_agent(&c.out[t], word);
            else c.out[t] = word;
        }
        uint32_t p[N];
        u64 d[N];
        form_promises<N>(c, t, p);
        form_datums<N>(word, d);
        hx::dag_put_n<N, SC1>(w, p, d);
    }
};

// G0<N>: put() after the body, one dag_put per promise; plain stores and loads
template <int N>
struct G0Kind {
    using Ctx = FormCtx;
    static constexpr bool kSc1Payload = false;
    __device__ static bool run_group(const Ctx &c, uint32_t t, const uint32_t *pl, int wave) {
        const int nwaves = (int)(blockDim.x >> 6);
        if (wave != (int)(t % (uint32_t)nwaves)) return true;
        if (pl[0] != t && hx::lane_id() == 0) atomicAdd(c.bad, 1u);
        const u64 word = task_word<kPlain>(c, t, nullptr);
        if (hx::lane_id() == 0) c.out[t] = word;
        return true;
    }
    __device__ static void put(const Ctx &c, hx::DagWave &w, uint32_t t) {
        const u64 word = task_word<kPlain>(c, t, &w);  // from the inputs again, with dag_get
        uint32_t p[N];
        u64 d[N];
        form_promises<N>(c, t, p);
        form_datums<N>(word, d);
#pragma unroll
        for (int i = 0; i < N; ++i) hx::dag_put(w, p[i], d[i]);
    }
};

// G1-sc1 / G1-plain / G3 / G4: the split put (kPutN)
template <int N, int MODE, bool TAGGED, bool RESERVE>
struct GKind {
    using Ctx = FormCtx;
    static constexpr int kPutN = N;
    static constexpr bool kSc1Payload = MODE != kPlain;
    static constexpr bool kTagged = TAGGED;
    static constexpr bool kReserve = RESERVE;
    __device__ static bool run_group(const Ctx &c, uint32_t t, const uint32_t *pl, int wave) {
        const int nwaves = (int)(blockDim.x >> 6);
        if (wave != (int)(t % (uint32_t)nwaves)) return true;
        if (pl[0] != t && hx::lane_id() == 0) atomicAdd(c.bad, 1u);
        const u64 word = task_word<MODE>(c, t, nullptr);
        if (hx::lane_id() == 0) {
            if (MODE == kPlain) c.out[t] = word;
            else hx::st_agent(&c.out[t], word);
        }
        return true;
    }
    __device__ static void promises(const Ctx &c, uint32_t t, uint32_t (&p)[N]) { form_promises<N>(c, t, p); }
    // the inputs are still there (satisfied promises stay): the value again
    __device__ static void datums(const Ctx &c, uint32_t t, unsigned long long (&d)[N]) {
        form_datums<N>(task_word<MODE>(c, t, nullptr), d);
    }
};

// ------------------------------------------------------------- host graphs
constexpr uint32_t kExtra = 0x80000000u;  // while a graph is built: promise kExtra + j is extra promise j

struct Graph {
    std::string name;
    int N = 1;
    uint32_t T = 0;
    std::vector<std::vector<uint32_t>> aw;  // per task, the promises it awaits (resolved by finish())
    uint32_t npre = 0;                      // extra promises put before the launch: ids N*T .. N*T + npre - 1
    bool stuck = false;                     // one more extra promise that nothing puts, awaited by the last task
    // a task with no waiters that may put a short-list / long-list promise a second time
    uint32_t dbl_short_task = kNone, dbl_short_promise = kNone, dbl_long_task = kNone, dbl_long_promise = kNone;
    // derived
    std::vector<uint32_t> entries;  // waiter entries per promise (awaits on promises not put before the launch)
    std::vector<uint32_t> val;      // the host evaluation
    uint32_t dup_awaits = 0, preput_awaits = 0, releases = 0;

    uint32_t add(std::vector<uint32_t> awaits) {
        aw.push_back(std::move(awaits));
        return T++;
    }
    uint32_t npromises() const { return (uint32_t)N * T + npre + (stuck ? 1u : 0u); }
    static uint32_t preval(uint32_t j) { return (uint32_t)mix(1000 + j); }
    void finish() {
        if (stuck) add({kExtra + npre});
        const uint32_t NT2 = (uint32_t)N * T;
        entries.assign(npromises(), 0);
        val.assign(T, 0);
        for (uint32_t t = 0; t < T; ++t) {
            bool registered = false;
            std::set<uint32_t> seen;
            u64 acc = mix(t);
            for (uint32_t &p : aw[t]) {
                if (p & kExtra) p = NT2 + (p - kExtra);
                if (!seen.insert(p).second) ++dup_awaits;
                const bool pre = p >= NT2 && p < NT2 + npre;
                if (pre) ++preput_awaits;
                else {
                    ++entries[p];
                    registered = true;
                }
                if (p < NT2) CHECK(p / (uint32_t)N < t, "%s: task %u awaits a later task", name.c_str(), t);
                acc = mix(acc ^ (u64)(p < NT2 ? val[p / (uint32_t)N] : preval(p - NT2)));
            }
            CHECK(aw[t].size() <= (size_t)kMaxAwaits, "%s: too many awaits", name.c_str());
            val[t] = (uint32_t)acc;
            if (registered) ++releases;
        }
    }
    uint32_t total(uint32_t t) const {
        uint32_t s = 0;
        for (int i = 0; i < N; ++i) s += entries[(uint32_t)N * t + (uint32_t)i];
        return s;
    }
    uint32_t widest(uint32_t t) const {
        uint32_t s = 0;
        for (int i = 0; i < N; ++i) s = std::max(s, entries[(uint32_t)N * t + (uint32_t)i]);
        return s;
    }
};

// how W waiter entries are spread over a rung's N promises
static std::vector<uint32_t> split(uint32_t W, int N, int round) {
    std::vector<uint32_t> c((size_t)N, 0);
    if (N == 1) {
        c[0] = W;
    } else if (round == 0) {  // nearly all on promise 0, one in the middle, one on the last
        const uint32_t last = W >= 2 ? 1 : 0, mid = W >= 3 ? 1 : 0;
        c[(size_t)N - 1] = last;
        c[(size_t)N / 2] += mid;
        c[0] += W - last - mid;
    } else {  // even, the remainder on the last
        for (int i = 0; i < N; ++i) c[(size_t)i] = W / (uint32_t)N;
        c[(size_t)N - 1] += W % (uint32_t)N;
    }
    return c;
}

static Graph ladder(int N, bool stuck) {
    Graph g;
    g.name = "ladder";
    g.N = N;
    g.stuck = stuck;
    const uint32_t totals[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 200};
    for (int round = 0; round < 2; ++round) {
        std::vector<std::vector<uint32_t>> rungs;
        for (uint32_t W : totals) rungs.push_back(split(W, N, round));
        if (N == 3) {
            rungs.push_back({20, 0, 44});
            rungs.push_back({1, 63, 1});
            rungs.push_back({0, 0, 64});
            rungs.push_back({64, 1, 0});
            rungs.push_back({30, 30, 3});
            rungs.push_back({0, 0, 0});
        }
        uint32_t prev = kNone;  // the rungs of one round hang on each other; the rounds run side by side
        for (const auto &cnt : rungs) {
            const uint32_t R = prev == kNone ? g.add({}) : g.add({(uint32_t)N * prev + (uint32_t)N - 1});
            uint32_t W = 0;
            for (uint32_t c : cnt) W += c;
            for (int i = 0; i < N; ++i) {
                const uint32_t p = (uint32_t)N * R + (uint32_t)i, c = cnt[(size_t)i];
                uint32_t e = 0, nth = 0;
                while (e < c) {
                    uint32_t w;
                    if (nth == 0 && c >= 3) {  // the first waiter awaits the promise twice
                        w = g.add({p, p});
                        e += 2;
                    } else {
                        w = g.add({p});
                        e += 1;
                    }
                    // the second waiter of promise 0 has no waiter of its own (the next
                    // rung hangs on the last waiter): it may put p a second time
                    if (round == 0 && i == 0 && nth == 1 && e < c) {
                        if (W == 63) g.dbl_short_task = w, g.dbl_short_promise = p;
                        if (W == 200) g.dbl_long_task = w, g.dbl_long_promise = p;
                    }
                    ++nth;
                    prev = w;
                }
            }
        }
    }
    g.finish();
    return g;
}

static Graph random_graph(int N) {
    Graph g;
    g.name = "random";
    g.N = N;
    g.npre = 16;
    const uint32_t T = 3000;
    const uint32_t hubs[] = {0, 1, 2, 600, 601, 1200, 1800, 2400};
    u64 s = 7 + (u64)N;
    for (uint32_t t = 0; t < T; ++t) {
        s = mix(s);
        const uint32_t k = t < 8 ? 0 : (uint32_t)(s % (kMaxAwaits + 1));
        std::vector<uint32_t> a;
        for (uint32_t q = 0; q < k; ++q) {
            s = mix(s);
            const uint32_t r = (uint32_t)(s >> 20);
            if (q > 0 && r % 7 == 0) {  // the same promise twice
                a.push_back(a[q - 1]);
            } else if (r % 11 == 0) {  // a promise put before the launch
                a.push_back(kExtra + (uint32_t)((s >> 8) % g.npre));
            } else if (q == 0 && r % 2 == 0) {  // a hub: long waiter lists
                uint32_t nh = 0;
                while (nh < 8 && hubs[nh] < t) ++nh;
                a.push_back((uint32_t)N * hubs[(s >> 8) % nh]);
            } else {
                const uint32_t back = 1 + (uint32_t)((s >> 8) % (t < 300 ? t : 300));
                a.push_back((uint32_t)N * (t - back) + (uint32_t)((s >> 4) % (u64)N));
            }
        }
        g.add(a);
    }
    g.finish();
    return g;
}

static Graph chain_fan(int N) {
    Graph g;
    g.name = "chain-fan";
    g.N = N;
    const uint32_t fan = 200, chain = 300;
    for (int copy = 0; copy < 5; ++copy) {
        const uint32_t root = g.add({});
        uint32_t last = root;
        for (uint32_t f = 0; f < fan; ++f) last = g.add({(uint32_t)N * root});
        for (uint32_t c = 0; c < chain; ++c) last = g.add({(uint32_t)N * last + (uint32_t)N - 1});
    }
    g.finish();
    return g;
}

// ------------------------------------------------------------------ forms
struct Built;
struct Form {
    const char *name;
    int N;
    bool per_promise;  // dag_put per promise: the long branch is a list of more than 64, not a total
    bool group;
    bool dbl, stuck;   // error launches
    int (*launch)(const FormCtx &, hclib::hip::dag &, hclib_hip_dag_stats_t *, int, int, uint32_t);
};

template <class Kind>
static int launch_worker(const FormCtx &c, hclib::hip::dag &g, hclib_hip_dag_stats_t *st, int waves_per_cu, int,
                         uint32_t spin_ms) {
    return hclib::hip::run_dag<Kind>(c, g, st, waves_per_cu, spin_ms);
}
template <class Kind>
static int launch_groups(const FormCtx &c, hclib::hip::dag &g, hclib_hip_dag_stats_t *st, int groups_per_cu,
                         int waves_per_group, uint32_t spin_ms) {
    return hclib::hip::run_dag_groups<Kind>(c, g, st, groups_per_cu, waves_per_group, spin_ms);
}

static const Form kForms[] = {
    {"W-putn<1,false>", 1, false, false, true, false, &launch_worker<WKind<1, false>>},
    {"W-putn<1,true>", 1, false, false, true, false, &launch_worker<WKind<1, true>>},
    {"W-putn<3,false>", 3, false, false, true, false, &launch_worker<WKind<3, false>>},
    {"W-putn<3,true>", 3, false, false, true, false, &launch_worker<WKind<3, true>>},
    {"W-putn<8,false>", 8, false, false, true, false, &launch_worker<WKind<8, false>>},
    {"W-putn<8,true>", 8, false, false, true, false, &launch_worker<WKind<8, true>>},
    {"G0<1>", 1, true, true, true, true, &launch_groups<G0Kind<1>>},
    {"G0<3>", 3, true, true, true, true, &launch_groups<G0Kind<3>>},
    {"G1-sc1<1>", 1, false, true, true, true, &launch_groups<GKind<1, kSc1, false, false>>},
    {"G1-sc1<3>", 3, false, true, true, true, &launch_groups<GKind<3, kSc1, false, false>>},
    {"G1-plain<1>", 1, false, true, false, false, &launch_groups<GKind<1, kPlain, false, false>>},
    {"G1-plain<3>", 3, false, true, false, false, &launch_groups<GKind<3, kPlain, false, false>>},
    {"G3<1>", 1, false, true, true, false, &launch_groups<GKind<1, kPoll, true, false>>},
    {"G3<3>", 3, false, true, true, false, &launch_groups<GKind<3, kPoll, true, false>>},
    {"G4<3>", 3, false, true, false, true, &launch_groups<GKind<3, kPoll, true, true>>},
};

// the branch a task's put takes in this form
static bool is_long(const Form &f, const Graph &g, uint32_t t) {
    return (f.per_promise ? g.widest(t) : g.total(t)) > 64;
}

static void print_plan(const Form &f, const Graph &g) {
    uint32_t ns = 0, nl = 0;
    std::set<uint32_t> totals;
    std::set<std::array<uint32_t, 3>> splits;
    for (uint32_t t = 0; t < g.T; ++t) {
        (is_long(f, g, t) ? nl : ns) += 1;
        totals.insert(g.total(t));
        if (g.N == 3) splits.insert({g.entries[3 * t], g.entries[3 * t + 1], g.entries[3 * t + 2]});
    }
    printf("plan form=%s graph=%s tasks=%u short=%u long=%u dup=%u preput=%u releases=%u", f.name, g.name.c_str(),
           g.T, ns, nl, g.dup_awaits, g.preput_awaits, g.releases);
    if (g.name == "ladder") {
        printf(" totals=");
        const char *sep = "";
        for (uint32_t w : totals) printf("%s%u", sep, w), sep = ",";
        if (g.N == 3) {
            printf(" splits=");
            sep = "";
            for (const auto &s : splits) printf("%s%u/%u/%u", sep, s[0], s[1], s[2]), sep = ",";
        }
    }
    printf("\n");
}

// A graph on the device: its dag, the awaits table and the output words.
struct Built {
    Graph g;
    hclib::hip::dag dag{1};
    std::vector<u64> out0;  // the output words before a launch
    uint32_t *d_aw = nullptr;
    u64 *d_out = nullptr;
    unsigned *d_bad = nullptr;

    explicit Built(Graph gg) : g(std::move(gg)) {
        const uint32_t NT = (uint32_t)g.N * g.T, nextra = g.npromises() - NT;
        for (uint32_t p = 0; p < g.npromises(); ++p) dag.promise();
        out0.assign((size_t)g.T + nextra, 0);
        for (uint32_t j = 0; j < g.npre; ++j) {
            out0[g.T + j] = kTag | Graph::preval(j);
            dag.put(NT + j, out0[g.T + j]);
        }
        std::vector<uint32_t> aw((size_t)g.T * kAwWords, 0);
        for (uint32_t t = 0; t < g.T; ++t) {
            aw[(size_t)t * kAwWords] = (uint32_t)g.aw[t].size();
            for (size_t q = 0; q < g.aw[t].size(); ++q) aw[(size_t)t * kAwWords + 1 + q] = g.aw[t][q];
            dag.async_await(&t, g.aw[t].data(), (int)g.aw[t].size());
        }
        CHECK(hipMalloc((void **)&d_aw, aw.size() * 4) == hipSuccess &&
                  hipMalloc((void **)&d_out, out0.size() * 8) == hipSuccess &&
                  hipMalloc((void **)&d_bad, 4) == hipSuccess,
              "hipMalloc");
        CHECK(hipMemcpy(d_aw, aw.data(), aw.size() * 4, hipMemcpyHostToDevice) == hipSuccess, "copy");
    }
    ~Built() {
        (void)hipFree(d_aw);
        (void)hipFree(d_out);
        (void)hipFree(d_bad);
    }
    FormCtx ctx(uint32_t dbl_task = kNone, uint32_t dbl_promise = kNone) {
        CHECK(hipMemcpy(d_out, out0.data(), out0.size() * 8, hipMemcpyHostToDevice) == hipSuccess, "copy");
        CHECK(hipMemset(d_bad, 0, 4) == hipSuccess, "memset");
        // the launch runs on the module's own non-blocking stream: the fill is done first
        CHECK(hipDeviceSynchronize() == hipSuccess, "synchronize");
        return FormCtx{d_aw, d_out, d_bad, g.T, (uint32_t)g.N, dbl_task, dbl_promise};
    }
};

static unsigned g_launches = 0;

// one clean launch, every assertion of the issue
static void clean_launch(const Form &f, Built &b, int a, int w) {
    const Graph &g = b.g;
    hclib_hip_dag_stats_t st;
    const int rc = f.launch(b.ctx(), b.dag, &st, a, w, 5000);
    ++g_launches;
    CHECK(rc == HCLIB_HIP_OK, "%s %s (%d, %d): %s", f.name, g.name.c_str(), a, w, hclib_hip_last_error());
    std::vector<u64> got(b.out0.size());
    unsigned nbad = 0;
    CHECK(hipMemcpy(got.data(), b.d_out, got.size() * 8, hipMemcpyDeviceToHost) == hipSuccess, "copy back");
    CHECK(hipMemcpy(&nbad, b.d_bad, 4, hipMemcpyDeviceToHost) == hipSuccess, "copy back");
    CHECK(nbad == 0, "%s %s (%d, %d): %u stale or untagged reads", f.name, g.name.c_str(), a, w, nbad);
    const uint32_t NT = (uint32_t)g.N * g.T;
    for (uint32_t t = 0; t < g.T; ++t) {
        const u64 want = kTag | g.val[t];
        CHECK(got[t] == want, "%s %s (%d, %d): task %u got %llx want %llx", f.name, g.name.c_str(), a, w, t, got[t],
              want);
        for (uint32_t i = 0; i < (uint32_t)g.N; ++i) {
            const uint32_t p = (uint32_t)g.N * t + i;
            CHECK(b.dag.satisfied(p) && b.dag.datum(p) == (want | ((u64)i << 40)),
                  "%s %s (%d, %d): promise %u satisfied %d datum %llx", f.name, g.name.c_str(), a, w, p,
                  (int)b.dag.satisfied(p), (u64)b.dag.datum(p));
        }
    }
    for (uint32_t j = 0; j < g.npre; ++j)
        CHECK(b.dag.satisfied(NT + j) && b.dag.datum(NT + j) == b.out0[g.T + j], "%s %s: pre-put promise %u", f.name,
              g.name.c_str(), NT + j);
    CHECK(st.tasks == g.T && st.puts == (u64)g.N * g.T && st.releases == g.releases,
          "%s %s (%d, %d): %llu tasks %llu puts %llu releases, want %u %llu %u", f.name, g.name.c_str(), a, w,
          (u64)st.tasks, (u64)st.puts, (u64)st.releases, g.T, (u64)g.N * g.T, g.releases);
}

static void error_launch(const Form &f, Built &b, uint32_t dbl_task, uint32_t dbl_promise, const char *what,
                         const char *word) {
    hclib_hip_dag_stats_t st;
    const int a = f.group ? 1 : 4, w = f.group ? 2 : 0;
    const int rc = f.launch(b.ctx(dbl_task, dbl_promise), b.dag, &st, a, w, 300);
    ++g_launches;
    CHECK(rc == HCLIB_HIP_EDEVICE && strstr(hclib_hip_last_error(), word), "%s %s: rc %d (%s)", f.name, what, rc,
          hclib_hip_last_error());
    printf("%-16s %-22s -> %s (%.3f ms)\n", f.name, what, hclib_hip_last_error(), st.kernel_ms);
}

int main(int argc, char **argv) {
    const bool plan = argc > 1 && !strcmp(argv[1], "--plan");
    int reps = 20;  // about 6 s on an MI355X, a quarter of it the five 300 ms deadlock launches
    if (argc > 2 && !strcmp(argv[1], "--reps")) reps = atoi(argv[2]);
    CHECK(reps >= 3, "at least 3 launches per (Kind, graph, shape)");
    if (plan) {
        for (const Form &f : kForms)
            for (const Graph &g : {ladder(f.N, false), random_graph(f.N), chain_fan(f.N)}) print_plan(f, g);
        return 0;
    }
    CHECK(hclib_hip_init(0) == HCLIB_HIP_OK, "hclib_hip_init: %s", hclib_hip_last_error());
    const auto t0 = std::chrono::steady_clock::now();
    std::map<int, std::vector<std::unique_ptr<Built>>> graphs;  // per N
    std::map<int, std::unique_ptr<Built>> stuck;
    for (int N : {1, 3, 8}) {
        graphs[N].emplace_back(new Built(ladder(N, false)));
        graphs[N].emplace_back(new Built(random_graph(N)));
        graphs[N].emplace_back(new Built(chain_fan(N)));
        if (N != 8) stuck[N].reset(new Built(ladder(N, true)));
        for (auto &b : graphs[N])
            CHECK(b->g.T >= 1000 && b->g.T <= 6000, "%s: %u tasks", b->g.name.c_str(), b->g.T);
    }
    for (const Form &f : kForms) {
        const unsigned before = g_launches;
        const auto f0 = std::chrono::steady_clock::now();
        for (auto &b : graphs[f.N]) {
            uint32_t nl = 0;
            for (uint32_t t = 0; t < b->g.T; ++t) nl += is_long(f, b->g, t) ? 1u : 0u;
            CHECK(nl >= 5 && b->g.T - nl >= 5, "%s %s: %u long puts", f.name, b->g.name.c_str(), nl);
            if (f.group) {
                for (int waves : {1, 2, 4})
                    for (int groups : {1, 2})
                        for (int r = 0; r < reps; ++r) clean_launch(f, *b, groups, waves);
            } else {
                for (int waves : {1, 4, 8})
                    for (int r = 0; r < reps; ++r) clean_launch(f, *b, waves, 0);
            }
        }
        Built &lad = *graphs[f.N][0];
        if (f.dbl) {
            const Graph &g = lad.g;
            CHECK(g.dbl_short_task != kNone && g.dbl_long_task != kNone, "ladder: no task for the second put");
            CHECK(g.total(g.dbl_short_task) == 0 && g.total(g.dbl_long_task) == 0, "ladder: the second putter has waiters");
            CHECK(g.entries[g.dbl_short_promise] >= 2 && g.entries[g.dbl_short_promise] <= 64 &&
                      g.entries[g.dbl_long_promise] > 64,
                  "ladder: the lists of the second puts");
            error_launch(f, lad, g.dbl_short_task, g.dbl_short_promise, "second put (short)", "single assignment");
            clean_launch(f, lad, 1, f.group ? 2 : 0);
            error_launch(f, lad, g.dbl_long_task, g.dbl_long_promise, "second put (long)", "single assignment");
            clean_launch(f, lad, 1, f.group ? 2 : 0);
        }
        if (f.stuck) {
            error_launch(f, *stuck[f.N], kNone, kNone, "unsatisfied future", "deadlock");
            clean_launch(f, lad, 1, 2);
        }
        const double ms =
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - f0).count();
        printf("%-16s %4u launches OK  %8.1f ms\n", f.name, g_launches - before, ms);
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%u launches in %.2f s\n", g_launches, sec);
    printf("Check results: OK\n");
    return 0;
}
