// The limits of dynamic device dataflow (include/hclib_hip/hx_dyn.h) through
// hclib::hip::run_dyn:
//
//  * wide awaits — a root creates P promises; awaiter tasks await up to
//    kDynMaxFutures (8) of them, some the same promise twice, some entries
//    kDynOpen holes. Three populations: A awaits promises the root has put
//    already (every future is found put), B awaits promises whose putter tasks
//    are created afterwards (every future takes a wait node), C is created by
//    eight generator tasks, 63 awaiters and the putter of one C promise at a
//    time, so that putters run while the other generators register awaiters
//    on any C promise (put before, after or while the awaiter registers: the
//    compare-and-swap retry). Each
//    awaiter stores mix(sum of its futures' data + id); the sum does not
//    depend on the order, so the host evaluates the same. tasks, created,
//    puts and promises are exact; releases depends on timing and is only
//    bounded.
//  * one promise with 5,000 wait nodes (the put's serial walk), every
//    waiter's value checked.
//  * pool limits — a small graph that needs exactly 11 tasks, 4 promises and
//    12 wait nodes: OK with every cap at the need; with the task, promise or
//    wait-node cap one below, HCLIB_HIP_EDEVICE "a device pool ran out" with
//    the used/cap pair, promptly, and the next launch is clean. The Kind
//    checks the kDynOpen / kDynEmpty returns and never uses them as indices.
//  * every body counts the launches' tasks that fewer than 64 lanes entered:
//    a wave that has run one task must run the next with all its lanes (the
//    generators of the wide case create one task per lane).
//
// The data are salted per launch: the pools' datum words are not cleared
// between launches, so an early release reads a value of another salt.
// Prints "Check results: OK" (tests/test_dyn_limits_gpu.py).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
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
using hx::DynWave;
using hx::kDynEmpty;
using hx::kDynOpen;

__host__ __device__ inline u64 mix(u64 x) {  // splitmix64 finaliser
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

enum : uint32_t { kRoot = 0, kAwaiter = 1, kPutter = 2, kGenerator = 3 };
enum : uint32_t { kWide = 0, kFan = 1, kSmall = 2 };
constexpr int kWords = 11;  // {kind, id, nfut, f0..f7}

// wide awaits: the promise ranges and awaiter counts of the three populations
constexpr uint32_t kPA = 32, kPB = 32, kPC = 64, kP = kPA + kPB + kPC;
constexpr uint32_t kNA = 256, kNB = 256, kGen = 8, kGenBatches = 8, kNC = kGen * kGenBatches * 63;
constexpr uint32_t kAwaiters = kNA + kNB + kNC;
static_assert(kPC == kGen * kGenBatches, "one putter per creation of a generator");
constexpr uint32_t kFanWaiters = 5000;
// the small graph: 4 promises, 6 awaiters on 2 promises each, 4 putters
constexpr uint32_t kSmallP = 4, kSmallA = 6;

struct LimCtx {
    uint32_t mode;
    u64 salt;
    u64 *out;            // one word per awaiter
    unsigned *refused;   // [0] creations the runtime refused (kDynOpen / kDynEmpty returns)
                         // [1] bodies entered by fewer than the wave's 64 lanes
};

__host__ __device__ inline u64 datum_of(u64 salt, uint32_t p) { return mix(salt + 77ull * p); }

// awaiter `id` of the wide case: its futures among promises [lo, hi) (relative
// to the first promise), holes as kDynOpen
__host__ __device__ inline int awaiter_futs(uint32_t id, uint32_t lo, uint32_t hi, uint32_t (&f)[8]) {
    const bool full = id % 16 == 0;  // eight futures, no hole
    const int nf = full ? 8 : 1 + (int)(mix(id) % 8);
    for (int k = 0; k < 8; ++k) {
        const u64 r = mix(8ull * id + (u64)k + 12345);
        if (k >= nf) f[k] = 0xffffffffu;
        else if (!full && r % 5 == 0) f[k] = 0xffffffffu;            // a hole
        else if (k > 0 && (r >> 8) % 6 == 0) f[k] = f[k - 1];        // the same promise twice (or the hole again)
        else f[k] = lo + (uint32_t)((r >> 16) % (hi - lo));
    }
    return nf;
}
__host__ __device__ inline void awaiter_range(uint32_t id, uint32_t &lo, uint32_t &hi) {
    if (id < kNA) lo = 0, hi = kPA;
    else if (id < kNA + kNB) lo = kPA, hi = kPA + kPB;
    else lo = kPA + kPB, hi = kP;
}

struct LimKind {
    using Ctx = LimCtx;
    static constexpr bool kSc1Payload = true;

    __device__ static void refused(const Ctx &c, bool mine) {
        const u64 m = __ballot(mine);
        if (m && hx::lane_id() == 0) atomicAdd(c.refused, (unsigned)__popcll(m));
    }
    // one creation of the wide case: awaiters first .. first + n - 1 in lanes
    // [0, n) and, unless put_p is kDynOpen, the putter of promise put_p in lane 63
    __device__ static void wide_batch(const Ctx &c, DynWave &w, uint32_t base, uint32_t first, uint32_t n,
                                      uint32_t put_p) {
        const uint32_t lane = (uint32_t)hx::lane_id(), id = first + lane;
        const bool aw = lane < n, pt = put_p != kDynOpen && lane == 63;
        uint32_t lo = 0, hi = 1, f[8], pl[kWords] = {kAwaiter, id, 0};
        awaiter_range(aw ? id : 0, lo, hi);
        const int nf = awaiter_futs(id, lo, hi, f);
        pl[2] = (uint32_t)nf;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (!aw) f[k] = kDynOpen;
            else if (f[k] != kDynOpen) f[k] += base;
            pl[3 + k] = f[k];
        }
        if (pt) pl[0] = kPutter, pl[1] = put_p;
        // every lane passes 8: its unused entries are holes
        const uint32_t t = hx::dyn_async_await<true>(w, aw || pt, pl, f, 8);
        refused(c, (aw || pt) && t == kDynEmpty);
    }
    __device__ static void wide_awaiters(const Ctx &c, DynWave &w, uint32_t base, uint32_t first, uint32_t n) {
        for (uint32_t i0 = 0; i0 < n; i0 += 64) wide_batch(c, w, base, first + i0, n - i0 < 64 ? n - i0 : 64, kDynOpen);
    }
    __device__ static void putters(const Ctx &c, DynWave &w, uint32_t first, uint32_t n, uint32_t ngen,
                                   uint32_t gen_base) {
        // lanes [0, ngen): generators; then the putters of promises first .. first + n - 1
        const uint32_t lane = (uint32_t)hx::lane_id();
        for (uint32_t i0 = 0; i0 < ngen + n; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool on = i < ngen + n;
            uint32_t pl[kWords] = {kPutter, 0, 0};
            if (i < ngen) pl[0] = kGenerator, pl[1] = i, pl[2] = gen_base;
            else pl[1] = first + (i - ngen);
            const uint32_t t = hx::dyn_async_await<true>(w, on, pl, nullptr, 0);
            refused(c, on && t == kDynEmpty);
        }
    }

    __device__ static void run(const Ctx &c, DynWave &w, uint32_t, const uint32_t *pay) {
        const uint32_t lane = (uint32_t)hx::lane_id();
        // a body is wave-wide: all 64 lanes enter, on a wave's first task and on every later one
        const u64 entered = __ballot(1);
        if (entered != ~0ull && lane == (uint32_t)__builtin_ctzll(entered)) atomicAdd(c.refused + 1, 1u);
        if (pay[0] == kPutter) {
            hx::dyn_put<true>(w, pay[1], datum_of(c.salt, pay[1]));
            return;
        }
        if (pay[0] == kAwaiter) {
            u64 sum = pay[1];
            for (int k = 0; k < 8; ++k)
                if (pay[3 + k] != kDynOpen) sum += hx::dyn_get(w, pay[3 + k]);
            if (lane == 0) hx::st_agent(&c.out[pay[1]], mix(sum));
            return;
        }
        if (pay[0] == kGenerator) {
            // population C: kGenBatches creations of 63 awaiters and the putter of one of
            // this generator's promises, while the other generators' putters run
            for (uint32_t b = 0; b < kGenBatches; ++b)
                wide_batch(c, w, pay[2], kNA + kNB + (pay[1] * kGenBatches + b) * 63, 63,
                           pay[2] + kPA + kPB + pay[1] * kGenBatches + b);
            return;
        }
        // the root
        if (c.mode == kWide) {
            const uint32_t base = hx::dyn_promises(w, kP);
            if (base == kDynOpen) {
                refused(c, lane == 0);
                return;
            }
            for (uint32_t p = 0; p < kPA; ++p) hx::dyn_put<true>(w, base + p, datum_of(c.salt, base + p));
            wide_awaiters(c, w, base, 0, kNA);        // A: every future already put
            wide_awaiters(c, w, base, kNA, kNB);      // B: registered before the putters exist
            putters(c, w, base + kPA, kPB, 0, base);
            putters(c, w, 0, 0, kGen, base);          // C: the generators create awaiters and putters
        } else if (c.mode == kFan) {
            const uint32_t p = hx::dyn_promises(w, 1);
            if (p == kDynOpen) {
                refused(c, lane == 0);
                return;
            }
            for (uint32_t i0 = 0; i0 < kFanWaiters; i0 += 64) {
                const uint32_t id = i0 + lane;
                uint32_t pl[kWords] = {kAwaiter, id, 1, p};
                for (int k = 1; k < 8; ++k) pl[3 + k] = kDynOpen;
                const uint32_t t = hx::dyn_async_await<true>(w, id < kFanWaiters, pl, &pl[3], 1);
                refused(c, id < kFanWaiters && t == kDynEmpty);
            }
            putters(c, w, p, 1, 0, 0);
        } else {
            const uint32_t base = hx::dyn_promises(w, kSmallP);
            if (base == kDynOpen) {  // never an index
                refused(c, lane == 0);
                return;
            }
            uint32_t pl[kWords] = {kAwaiter, lane, 2, base + lane % kSmallP, base + (lane + 1) % kSmallP};
            for (int k = 2; k < 8; ++k) pl[3 + k] = kDynOpen;
            const uint32_t t = hx::dyn_async_await<true>(w, lane < kSmallA, pl, &pl[3], 2);
            refused(c, lane < kSmallA && t == kDynEmpty);
            putters(c, w, base, kSmallP, 0, 0);
        }
    }
};

struct Dev {
    u64 *out = nullptr;
    unsigned *refused = nullptr;
    Dev() {
        CHECK(hipMalloc((void **)&out, 8 * 8192) == hipSuccess && hipMalloc((void **)&refused, 8) == hipSuccess,
              "hipMalloc");
    }
    LimCtx ctx(uint32_t mode, u64 salt) {
        CHECK(hipMemset(out, 0, 8 * 8192) == hipSuccess && hipMemset(refused, 0, 8) == hipSuccess, "memset");
        // the launch runs on the module's own non-blocking stream: the fills are done first
        CHECK(hipDeviceSynchronize() == hipSuccess, "synchronize");
        return LimCtx{mode, salt, out, refused};
    }
    std::vector<u64> words(uint32_t n) {
        std::vector<u64> h(n);
        CHECK(hipMemcpy(h.data(), out, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess, "copy back");
        return h;
    }
    unsigned raw_refused() {
        unsigned r = 0;
        (void)hipMemcpy(&r, refused, 4, hipMemcpyDeviceToHost);
        return r;
    }
    unsigned nrefused() {
        unsigned r[2] = {0, 0};
        CHECK(hipMemcpy(r, refused, 8, hipMemcpyDeviceToHost) == hipSuccess, "copy back");
        CHECK(r[1] == 0, "%u task bodies were entered by fewer than 64 lanes", r[1]);
        return r[0];
    }
};

static const std::vector<uint32_t> kRootPayload(kWords, 0);

static uint32_t g_b_released = 0;

static void wide(Dev &d, u64 salt, int waves_per_cu) {
    hclib::hip::dyn_caps caps;
    caps.tasks = 8192, caps.promises = 256, caps.wait_nodes = 8 * kAwaiters;
    caps.waves_per_cu = waves_per_cu;
    caps.spin_limit_ms = 2000;
    hclib_hip_dyn_stats_t st;
    const int rc = hclib::hip::run_dyn<LimKind>(d.ctx(kWide, salt), kWords, kRootPayload, caps, &st);
    if (rc != HCLIB_HIP_OK) {  // what ran, before the failure is reported
        const std::string msg = hclib_hip_last_error();
        std::vector<uint64_t> dat(kP);
        std::vector<uint8_t> put(kP);
        (void)hclib_hip_dyn_datum(0, kP, dat.data(), put.data());
        const std::vector<u64> got = d.words(kAwaiters);
        uint32_t np[3] = {0, 0, 0}, na[3] = {0, 0, 0};
        for (uint32_t p = 0; p < kP; ++p) np[p < kPA ? 0 : p < kPA + kPB ? 1 : 2] += put[p];
        for (uint32_t id = 0; id < kAwaiters; ++id) na[id < kNA ? 0 : id < kNA + kNB ? 1 : 2] += got[id] != 0;
        fprintf(stderr,
                "wide awaits (%d waves per CU): %llu tasks %llu created %llu puts %llu promises %llu releases, %u refused; "
                "promises put A %u B %u C %u; awaiters run A %u B %u C %u\n",
                waves_per_cu, (u64)st.tasks, (u64)st.created, (u64)st.puts, (u64)st.promises, (u64)st.releases,
                d.raw_refused(), np[0], np[1], np[2], na[0], na[1], na[2]);
        CHECK(false, "wide awaits: %s", msg.c_str());
    }
    CHECK(d.nrefused() == 0, "wide awaits: a creation was refused");
    const std::vector<uint64_t> datum = hclib::hip::dyn_datum(0, kP);
    CHECK(datum.size() == kP, "dyn_datum: %s", hclib_hip_last_error());
    for (uint32_t p = 0; p < kP; ++p) CHECK(datum[p] == datum_of(salt, p), "wide awaits: promise %u", p);
    const std::vector<u64> got = d.words(kAwaiters);
    uint32_t dups = 0, holes = 0, eights = 0;
    g_b_released = 0;
    for (uint32_t id = 0; id < kAwaiters; ++id) {
        uint32_t lo, hi, f[8];
        awaiter_range(id, lo, hi);
        const int nf = awaiter_futs(id, lo, hi, f);
        u64 sum = id;
        int live = 0;
        for (int k = 0; k < 8; ++k) {
            if (f[k] == kDynOpen) {
                holes += k < nf ? 1u : 0u;
                continue;
            }
            CHECK(f[k] >= lo && f[k] < hi, "awaiter %u: future %u outside its range", id, f[k]);
            sum += datum_of(salt, f[k]);
            ++live;
            for (int j = 0; j < k; ++j)
                if (f[j] == f[k]) {
                    ++dups;
                    break;
                }
        }
        eights += live == 8 ? 1u : 0u;
        // population B registers before its putters exist: released by a put unless it awaits holes only
        if (id >= kNA && id < kNA + kNB && live) ++g_b_released;
        CHECK(got[id] == mix(sum), "wide awaits: awaiter %u (%d futures) got %llx want %llx", id, live, got[id],
              mix(sum));
    }
    CHECK(dups >= 50 && holes >= 50 && eights >= 30, "wide awaits: %u duplicates, %u holes, %u awaiters of 8", dups,
          holes, eights);
    const u64 tasks = 1 + kAwaiters + kPB + kPC + kGen;
    CHECK(st.tasks == tasks && st.created == tasks - 1 && st.puts == kP && st.promises == kP,
          "wide awaits: %llu tasks %llu created %llu puts %llu promises", (u64)st.tasks, (u64)st.created,
          (u64)st.puts, (u64)st.promises);
    CHECK(st.releases <= st.created, "wide awaits: %llu releases of %llu tasks", (u64)st.releases, (u64)st.created);
    CHECK(st.releases >= g_b_released, "wide awaits: %llu releases, B alone has %u", (u64)st.releases, g_b_released);
    printf("wide awaits: %u awaiters (%u of 8 futures, %u duplicates, %u holes), %llu released by puts (%.3f ms)\n",
           kAwaiters, eights, dups, holes, (u64)st.releases, st.kernel_ms);
}

static void fan(Dev &d, u64 salt) {
    hclib::hip::dyn_caps caps;
    caps.tasks = kFanWaiters + 2, caps.promises = 1, caps.wait_nodes = kFanWaiters;
    hclib_hip_dyn_stats_t st;
    const int rc = hclib::hip::run_dyn<LimKind>(d.ctx(kFan, salt), kWords, kRootPayload, caps, &st);
    CHECK(rc == HCLIB_HIP_OK, "fan: %s", hclib_hip_last_error());
    CHECK(d.nrefused() == 0, "fan: a creation was refused");
    const std::vector<u64> got = d.words(kFanWaiters);
    for (uint32_t id = 0; id < kFanWaiters; ++id)
        CHECK(got[id] == mix((u64)id + datum_of(salt, 0)), "fan: waiter %u", id);
    // the putter is created after every waiter has registered: all are released by its put
    CHECK(st.tasks == kFanWaiters + 2 && st.created == kFanWaiters + 1 && st.puts == 1 && st.promises == 1 &&
              st.releases == kFanWaiters,
          "fan: %llu tasks %llu created %llu puts %llu releases", (u64)st.tasks, (u64)st.created, (u64)st.puts,
          (u64)st.releases);
    printf("one promise with %u wait nodes: OK (%.3f ms)\n", kFanWaiters, st.kernel_ms);
}

// the small graph under the caps given: OK, or the pool error naming `pair`
static void small(Dev &d, u64 salt, uint32_t tasks, uint32_t promises, uint32_t nodes, const char *pair) {
    hclib::hip::dyn_caps caps;
    caps.tasks = tasks, caps.promises = promises, caps.wait_nodes = nodes;
    caps.spin_limit_ms = 2000;
    hclib_hip_dyn_stats_t st;
    const int rc = hclib::hip::run_dyn<LimKind>(d.ctx(kSmall, salt), kWords, kRootPayload, caps, &st);
    if (pair) {
        const char *msg = hclib_hip_last_error();
        CHECK(rc == HCLIB_HIP_EDEVICE && strstr(msg, "a device pool ran out") && strstr(msg, pair),
              "caps %u/%u/%u: rc %d (%s), want %s", tasks, promises, nodes, rc, msg, pair);
        // a pool error ends the launch at once: far below the 2,000 ms spin limit
        CHECK(st.kernel_ms < 200.0, "caps %u/%u/%u: %.3f ms", tasks, promises, nodes, st.kernel_ms);
        printf("caps %u/%u/%u -> %s (%.3f ms)\n", tasks, promises, nodes, msg, st.kernel_ms);
        return;
    }
    CHECK(rc == HCLIB_HIP_OK, "caps %u/%u/%u: %s", tasks, promises, nodes, hclib_hip_last_error());
    CHECK(d.nrefused() == 0, "small: a creation was refused");
    const std::vector<u64> got = d.words(kSmallA);
    for (uint32_t id = 0; id < kSmallA; ++id)
        CHECK(got[id] == mix((u64)id + datum_of(salt, id % kSmallP) + datum_of(salt, (id + 1) % kSmallP)),
              "small: awaiter %u", id);
    CHECK(st.tasks == 1 + kSmallA + kSmallP && st.created == kSmallA + kSmallP && st.puts == kSmallP &&
              st.promises == kSmallP && st.releases == kSmallA,
          "small: %llu tasks %llu created %llu puts %llu releases", (u64)st.tasks, (u64)st.created, (u64)st.puts,
          (u64)st.releases);
}

int main() {
    CHECK(hclib_hip_init(0) == HCLIB_HIP_OK, "hclib_hip_init: %s", hclib_hip_last_error());
    const auto t0 = std::chrono::steady_clock::now();
    Dev d;
    u64 salt = 1;
    for (int rep = 0; rep < 4; ++rep)
        for (int waves : {1, 4, 8}) wide(d, mix(salt++), waves);
    for (int rep = 0; rep < 3; ++rep) fan(d, mix(salt++));
    const uint32_t T = 1 + kSmallA + kSmallP, P = kSmallP, W = 2 * kSmallA;
    small(d, mix(salt++), T, P, W, nullptr);  // every cap exactly at the need
    small(d, mix(salt++), T - 1, P, W, "tasks 11/10");
    small(d, mix(salt++), T, P, W, nullptr);
    small(d, mix(salt++), T, P - 1, W, "promises 4/3");
    small(d, mix(salt++), T, P, W, nullptr);
    small(d, mix(salt++), T, P, W - 1, "wait nodes 12/11");
    small(d, mix(salt++), T, P, W, nullptr);
    printf("pool limits: exact caps OK, one below refused, next launch clean\n");
    printf("%.2f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    printf("Check results: OK\n");
    return 0;
}
