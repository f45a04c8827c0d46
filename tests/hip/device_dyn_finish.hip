// Finish scopes of dynamic device dataflow (include/hclib_hip/hx_dyn.h:
// dyn_finish_open / dyn_finish_check_in / dyn_finish_check_out) through
// hclib::hip::run_dyn, with task kinds defined in this file:
//
//  * fib with finish scopes — test/fib/fib.c:57-71 as the reference writes
//    it: fib(n, res) stores n, or runs finish { async fib(n-1, &x); async
//    fib(n-2, &y); } and then stores x + y. Here the finish is a scope opened
//    with two check-ins and the code after it a task that awaits the scope
//    and inherits the caller's own scope. Values move through plain stores and
//    loads, ordered by the check-outs alone. fib(0..20) against fib_iter, with
//    the task and scope counts the program implies.
//
//  * a tree with dynamic check-in: every node checks its two children in to
//    ONE root scope (no scope per node) down to depth 12; each of the 4096
//    leaves stores a word with a plain store; one task awaits the scope and
//    reads all the words with plain loads.
//
//  * the error: a second check-out of a scope that is already put returns
//    HCLIB_HIP_EDEVICE (single assignment) and the launch drains.
//
// Prints "Check results: OK" (tests/test_dyn_finish_gpu.py).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

using hx::DynWave;
using hx::kDynOpen;

// ------------------------------------------------------------------ fib
enum : uint32_t { kMain = 0, kFib = 1, kSum = 2 };

struct FibCtx {
    int n;
    unsigned long long *vals;  // result slots; slot 0 is fib(n)
    uint32_t *next;            // next free slot
    uint32_t nslots;
};

struct FibFinishKind {
    using Ctx = FibCtx;
    static constexpr bool kSc1Payload = false;  // values move by plain stores and loads
    // payload: {kind, a, b, c, fin}: main {}, fib {n, res, -, fin}, sum {x, y, res, fin}
    __device__ static void run(const Ctx &c, DynWave &w, uint32_t, const uint32_t *pay) {
        const uint32_t kind = pay[0];
        const int lane = hx::lane_id();
        if (kind == kMain) {  // finish { async fib(n, &vals[0]); }
            const uint32_t f0 = hx::dyn_finish_open(w, 1);
            const uint32_t p[5] = {kFib, (uint32_t)c.n, 0u, 0u, f0};
            hx::dyn_async_await<true>(w, lane == 0, p, nullptr, 0);
            return;
        }
        if (kind == kFib) {
            const uint32_t n = pay[1], res = pay[2], fin = pay[4];
            if (n < 2) {
                if (lane == 0) c.vals[res] = n;
                hx::dyn_finish_check_out<false>(w, fin);
                return;
            }
            uint32_t s = 0;
            if (lane == 0) s = hx::add_agent(c.next, 2u);
            s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
            if (s + 2 > c.nslots) {
                if (lane == 0) hx::dev_error(hx::dyn_err(w.v), hx::kErrBadTask);
                return;
            }
            const uint32_t f = hx::dyn_finish_open(w, 2);
            // lanes 0, 1: fib(n-1) -> s, fib(n-2) -> s+1 into f; lane 2: the code
            // after the finish, awaiting f, checked in to fin in this task's place
            uint32_t pl[5] = {kFib, n - 1, s, 0u, f}, fut[1] = {kDynOpen};
            if (lane == 1) {
                pl[1] = n - 2, pl[2] = s + 1;
            } else if (lane == 2) {
                pl[0] = kSum, pl[1] = s, pl[2] = s + 1, pl[3] = res, pl[4] = fin;
                fut[0] = f;
            }
            hx::dyn_async_await<true>(w, lane < 3, pl, fut, 1);
            return;
        }
        // sum: everything checked in to the scope has checked out
        if (lane == 0) c.vals[pay[3]] = c.vals[pay[1]] + c.vals[pay[2]];
        hx::dyn_finish_check_out<false>(w, pay[4]);
    }
};

static unsigned long long fib_iter(int n) {  // test/fib/fib.c:38-46
    unsigned long long a = 0, b = 1;
    for (int i = 0; i < n; ++i) {
        const unsigned long long t = a + b;
        a = b;
        b = t;
    }
    return a;
}

// ----------------------------------------------------------------- tree
constexpr int kDepth = 12;
enum : uint32_t { kTreeMain = 0, kTreeNode = 1, kTreeRead = 2 };

__host__ __device__ inline uint32_t leaf_word(uint32_t i) { return i * 2654435761u + 12345u; }

struct TreeCtx {
    uint32_t *words;     // [1 << kDepth]
    uint32_t *mismatch;  // the reader's count (preset to ~0)
};

struct TreeKind {
    using Ctx = TreeCtx;
    static constexpr bool kSc1Payload = false;
    // payload: {kind, depth, index, scope}
    __device__ static void run(const Ctx &c, DynWave &w, uint32_t, const uint32_t *pay) {
        const int lane = hx::lane_id();
        if (pay[0] == kTreeMain) {
            const uint32_t root = hx::dyn_finish_open(w, 1);
            uint32_t pl[4] = {kTreeNode, 0u, 0u, root}, fut[1] = {kDynOpen};
            if (lane == 1) {
                pl[0] = kTreeRead;
                fut[0] = root;
            }
            hx::dyn_async_await<true>(w, lane < 2, pl, fut, 1);
            return;
        }
        if (pay[0] == kTreeNode) {
            const uint32_t d = pay[1], i = pay[2], scope = pay[3];
            if (d == (uint32_t)kDepth) {
                if (lane == 0 && i < (1u << kDepth)) c.words[i] = leaf_word(i);
                hx::dyn_finish_check_out<false>(w, scope);
                return;
            }
            hx::dyn_finish_check_in(w, scope, 2);
            const uint32_t pl[4] = {kTreeNode, d + 1, 2 * i + (uint32_t)(lane & 1), scope};
            hx::dyn_async_await<true>(w, lane < 2, pl, nullptr, 0);
            hx::dyn_finish_check_out<true>(w, scope);
            return;
        }
        uint32_t bad = 0;
        for (uint32_t i = (uint32_t)lane; i < (1u << kDepth); i += 64) bad += c.words[i] != leaf_word(i) ? 1u : 0u;
        bad = hx::wave_sum(bad);
        if (lane == 0) hx::st_agent(c.mismatch, bad);
    }
};

// ---------------------------------------------------------------- error
struct BadFinishKind {
    using Ctx = int;
    static constexpr bool kSc1Payload = true;
    __device__ static void run(const Ctx &, DynWave &w, uint32_t, const uint32_t *) {
        const uint32_t f = hx::dyn_finish_open(w, 1);
        hx::dyn_finish_check_out<true>(w, f);  // count 0: the scope is put
        hx::dyn_finish_check_out<true>(w, f);
    }
};

static void finish_stats(uint64_t &finishes, uint64_t &check_ins) {
    uint64_t s[2] = {0, 0};
    hclib_hip_dyn_finish_stats(s);
    finishes = s[0];
    check_ins = s[1];
}

int main() {
    CHECK(hclib_hip_init(0) == HCLIB_HIP_OK, "hclib_hip_init: %s", hclib_hip_last_error());
    hclib::hip::dyn_caps caps;
    caps.tasks = 100000;
    caps.promises = 100000;
    caps.wait_nodes = 100000;
    const uint32_t nslots = 1u << 16;
    unsigned long long *vals = nullptr;
    uint32_t *next = nullptr;
    CHECK(hipMalloc((void **)&vals, nslots * sizeof(unsigned long long)) == hipSuccess &&
              hipMalloc((void **)&next, 256) == hipSuccess,
          "hipMalloc");
    for (int n = 0; n <= 20; ++n) {
        const uint32_t one = 1;
        CHECK(hipMemset(vals, 0xff, nslots * sizeof(unsigned long long)) == hipSuccess &&
                  hipMemcpy(next, &one, 4, hipMemcpyHostToDevice) == hipSuccess,
              "reset");
        hclib_hip_dyn_stats_t st;
        const int rc = hclib::hip::run_dyn<FibFinishKind>(FibCtx{n, vals, next, nslots}, 5, {kMain, 0, 0, 0, 0}, caps, &st);
        CHECK(rc == HCLIB_HIP_OK, "run_dyn<FibFinishKind>(%d): %s", n, hclib_hip_last_error());
        unsigned long long got = 0;
        CHECK(hipMemcpy(&got, vals, sizeof(got), hipMemcpyDeviceToHost) == hipSuccess, "copy");
        CHECK(got == fib_iter(n), "fib(%d) = %llu, want %llu", n, got, fib_iter(n));
        // fib calls: 2 fib(n+1) - 1; each inner call (fib(n+1) - 1 of them) opens
        // one scope and creates one sum task; main opens one more scope; every
        // scope is put exactly once, by its last check-out
        const unsigned long long calls = 2 * fib_iter(n + 1) - 1, inner = fib_iter(n + 1) - 1;
        uint64_t finishes = 0, check_ins = 0;
        finish_stats(finishes, check_ins);
        CHECK(st.tasks == 1 + calls + inner && st.created == calls + inner, "fib(%d): %llu tasks run, %llu created", n,
              (unsigned long long)st.tasks, (unsigned long long)st.created);
        CHECK(finishes == 1 + inner && st.promises == 1 + inner && st.puts == 1 + inner && check_ins == 0,
              "fib(%d): %llu scopes, %llu promises, %llu puts, %llu check-ins", n, (unsigned long long)finishes,
              (unsigned long long)st.promises, (unsigned long long)st.puts, (unsigned long long)check_ins);
        uint8_t put = 0;
        CHECK(hclib_hip_dyn_datum(0, 1, nullptr, &put) == HCLIB_HIP_OK && put == 1, "fib(%d): main's scope not put", n);
        if (n == 20)
            printf("fib(20) = %llu with finish scopes: %llu tasks, %llu scopes (%.3f ms)\n", got,
                   (unsigned long long)st.tasks, (unsigned long long)finishes, st.kernel_ms);
    }
    (void)hipFree(vals);
    (void)hipFree(next);

    // the tree
    const uint32_t nleaf = 1u << kDepth, nodes = 2 * nleaf - 1;
    uint32_t *words = nullptr, *mismatch = nullptr;
    CHECK(hipMalloc((void **)&words, nleaf * 4) == hipSuccess && hipMalloc((void **)&mismatch, 256) == hipSuccess,
          "hipMalloc");
    CHECK(hipMemset(words, 0xab, nleaf * 4) == hipSuccess && hipMemset(mismatch, 0xff, 4) == hipSuccess, "reset");
    hclib_hip_dyn_stats_t st;
    int rc = hclib::hip::run_dyn<TreeKind>(TreeCtx{words, mismatch}, 4, {kTreeMain, 0, 0, 0}, caps, &st);
    CHECK(rc == HCLIB_HIP_OK, "run_dyn<TreeKind>: %s", hclib_hip_last_error());
    uint32_t bad = 0;
    CHECK(hipMemcpy(&bad, mismatch, 4, hipMemcpyDeviceToHost) == hipSuccess, "copy");
    uint64_t finishes = 0, check_ins = 0;
    finish_stats(finishes, check_ins);
    CHECK(bad == 0, "tree: the reader saw %u stale or missing words of %u", bad, nleaf);
    CHECK(st.tasks == 2ull + nodes && check_ins == nodes - 1ull && finishes == 1 && st.puts == 1,
          "tree: %llu tasks, %llu check-ins, %llu scopes, %llu puts", (unsigned long long)st.tasks,
          (unsigned long long)check_ins, (unsigned long long)finishes, (unsigned long long)st.puts);
    printf("tree of %u nodes checked in to one scope: %llu check-ins, 0 mismatches of %u words (%.3f ms)\n", nodes,
           (unsigned long long)check_ins, nleaf, st.kernel_ms);
    (void)hipFree(words);
    (void)hipFree(mismatch);

    // the error
    caps.spin_limit_ms = 300;
    rc = hclib::hip::run_dyn<BadFinishKind>(0, 1, {0u}, caps);
    CHECK(rc == HCLIB_HIP_EDEVICE && strstr(hclib_hip_last_error(), "single assignment"), "second check-out: %d %s", rc,
          hclib_hip_last_error());
    printf("second check-out of a put scope: %s\n", hclib_hip_last_error());
    printf("Check results: OK\n");
    return 0;
}
