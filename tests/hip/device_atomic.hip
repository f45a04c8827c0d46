// Privatised atomics in device code (include/hclib_hip/hx_atomic.h,
// hclib::hip::atomic_sum_t / atomic_max_t / atomic_or_t and
// forasync{1,2,3}D_gather in include/hclib_hip_cpp.h), the device form of
// inc/hclib_atomic.h:141-186:
//  * update() under eight active masks, for int32 / int64 / float / double;
//  * __device__ lambdas that update atomics on the forasync iteration sets
//    (src/hclib.c:110-416, restated on the host here), and the reducing
//    sweep forasync*_gather on the same sets;
//  * a user Kind on run_tasks holding three views in its Ctx;
//  * accumulation over launches, reset, several atomics in one kernel, a
//    64-bit sum past 2^32.
// Every expected value comes from a serial loop on the host. Prints one
// line per check, then "Check results: OK" (tests/test_atomic_gpu.py).
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "hclib_hip_cpp.h"

#define CHECK(c, ...)                                        \
    do {                                                     \
        if (!(c)) {                                          \
            fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                    \
            fprintf(stderr, "\n");                           \
            exit(1);                                         \
        }                                                    \
    } while (0)

using hclib::hip::atomic_max_t;
using hclib::hip::atomic_or_t;
using hclib::hip::atomic_sum_t;

// ------------------------------------------------------------ active masks
template <typename T>
__global__ __launch_bounds__(256) void k_masks(unsigned long long mask, hx::AtomicView<T, hx::Sum> s,
                                               hx::AtomicView<T, hx::Max> m, hx::AtomicView<T, hx::Or> o) {
    const int lane = (int)(threadIdx.x & 63u);
    if ((mask >> lane) & 1ull) {
        s += (T)(lane + 1);
        m.update((T)(-(lane + 1)));
        o |= (T)(lane == 63);
    }
}

template <typename T>
static void check_masks(const char *name) {
    const unsigned long long masks[] = {~0ull,
                                        1ull,
                                        1ull << 63,
                                        0x5555555555555555ull,
                                        0x00000000ffffffffull,
                                        0xffffffff00000000ull,
                                        0x8000000000000001ull,
                                        0ull};
    const T lowest = std::numeric_limits<T>::lowest();
    atomic_sum_t<T> s((T)0);
    atomic_max_t<T> m(lowest);
    atomic_or_t<T> o((T)0);
    CHECK(s.ok() && m.ok() && o.ok(), "atomic create: %s", hclib_hip_last_error());
    const int blocks = 4, waves = blocks * 4;
    for (unsigned long long mask : masks) {
        CHECK(s.reset() == 0 && m.reset() == 0 && o.reset() == 0, "reset: %s", hclib_hip_last_error());
        hipLaunchKernelGGL(k_masks<T>, dim3(blocks), dim3(256), 0, nullptr, mask, s.view(), m.view(), o.view());
        CHECK(hipGetLastError() == hipSuccess, "k_masks launch");
        T ws = (T)0, wm = lowest, wo = (T)0;  // serial host evaluation
        for (int w = 0; w < waves; ++w)
            for (int lane = 0; lane < 64; ++lane)
                if ((mask >> lane) & 1ull) {
                    ws = (T)(ws + (T)(lane + 1));
                    const T v = (T)(-(lane + 1));
                    wm = v > wm ? v : wm;
                    wo = (T)((wo != (T)0 || lane == 63) ? 1 : 0);
                }
        const T gs = s.get(), gm = m.get(), go = o.get();
        CHECK(gs == ws && gm == wm && go == wo, "%s mask %016llx: sum %g max %g or %g, want %g %g %g", name, mask,
              (double)gs, (double)gm, (double)go, (double)ws, (double)wm, (double)wo);
    }
    printf("active masks (%s): sum / max / or under 8 masks, empty mask leaves the default\n", name);
}

// ------------------------------------------- reference iteration sets (host)
// one dimension's indices in the order the reference's tiles visit them
static void ref_runner(int low, int high, int stride, std::vector<int> &out) {
    for (int i = low; i < high; i += stride) out.push_back(i);
}
static void ref_recursive(int low, int high, int stride, int tile, std::vector<int> &out) {
    if ((high - low) > tile) {
        const int mid = (high + low) / 2;
        ref_recursive(low, mid, stride, tile, out);
        ref_recursive(mid, high, stride, tile, out);
    } else {
        ref_runner(low, high, stride, out);
    }
}
static void ref_flat1d(int low, int high, int stride, int tile, std::vector<int> &out) {
    const int nb_chunks = high / tile, size = tile * nb_chunks;
    int low0;
    for (low0 = low; low0 < size; low0 += tile) ref_runner(low0, low0 + tile, stride, out);
    if (size < high) ref_runner(low0, high, stride, out);
}
static void ref_flat_nd(int low, int high, int stride, int tile, std::vector<int> &out) {
    for (int low0 = low; low0 < high; low0 += tile)
        ref_runner(low0, (low0 + tile) > high ? high : (low0 + tile), stride, out);
}
struct Dom {
    int low, high, stride, tile;
};
static std::vector<int> ref_dim(Dom d, int ndim, int mode) {
    if (d.tile == -1) {
        const int nw = hclib_hip_num_workers();
        d.tile = ((d.high - d.low) + nw - 1) / nw;
    }
    if (d.tile < 1) d.tile = 1;
    std::vector<int> v;
    if (mode == FORASYNC_MODE_RECURSIVE) ref_recursive(d.low, d.high, d.stride, d.tile, v);
    else if (ndim == 1) ref_flat1d(d.low, d.high, d.stride, d.tile, v);
    else ref_flat_nd(d.low, d.high, d.stride, d.tile, v);
    return v;
}

static void set_dims(hclib_loop_domain_t *l, const Dom *d, int nd) {
    for (int x = 0; x < nd; ++x) l[x] = hclib_loop_domain_t{d[x].low, d[x].high, d[x].stride, d[x].tile};
}

__host__ __device__ static inline long long linear(int i, int j, int k) {
    return ((long long)i * 1000 + j) * 1000 + k;
}

struct Want {
    long long sum = 0, max = std::numeric_limits<long long>::lowest(), last = 0;
    int flag = 0;
    long long count = 0;
};
static Want want_of(const Dom *d, int nd, int mode) {
    std::vector<int> v[3] = {{0}, {0}, {0}};
    for (int x = 0; x < nd; ++x) v[x] = ref_dim(d[x], nd, mode);
    Want w;
    for (int i : v[0])
        for (int j : v[1])
            for (int k : v[2]) {
                const long long l = linear(i, j, k);
                w.sum += l;
                w.max = l > w.max ? l : w.max;
                w.count++;
            }
    w.last = w.max;  // the flag is raised by the iteration with the largest index
    w.flag = w.count > 0 ? 1 : 0;
    return w;
}

// updates from lambdas (forasyncND) and the reducing sweep (forasyncND_gather)
// on one domain: both must give the host's sum / max / or
template <int ND>
static void check_domain(const Dom *d, int mode) {
    const Want w = want_of(d, ND, mode);
    const long long lowest = std::numeric_limits<long long>::lowest();
    atomic_sum_t<long long> s(0), gs(0);
    atomic_max_t<long long> m(lowest), gm(lowest);
    atomic_or_t<int> o(0), go(0);
    CHECK(s.ok() && m.ok() && o.ok() && gs.ok() && gm.ok() && go.ok(), "atomic create: %s", hclib_hip_last_error());
    const auto sv = s.view();
    const auto mv = m.view();
    const auto ov = o.view();
    const long long last = w.last;
    int rc[4];
    if constexpr (ND == 1) {
        auto mk = [&]() {
            hclib::loop_domain_1d L(d[0].low, d[0].high);
            set_dims(L.get_internal(), d, 1);
            return L;
        };
        auto L0 = mk(), L1 = mk(), L2 = mk(), L3 = mk();
        rc[0] = hclib::hip::forasync1D(&L0, [=] __device__(int i) {
            const long long l = linear(i, 0, 0);
            sv += l;
            mv.update(l);
            ov |= (int)(l == last);
        }, mode);
        rc[1] = hclib::hip::forasync1D_gather(&L1, gs, [=] __device__(int i) { return linear(i, 0, 0); }, mode);
        rc[2] = hclib::hip::forasync1D_gather(&L2, gm, [=] __device__(int i) { return linear(i, 0, 0); }, mode);
        rc[3] = hclib::hip::forasync1D_gather(&L3, go, [=] __device__(int i) { return (int)(linear(i, 0, 0) == last); },
                                              mode);
    } else if constexpr (ND == 2) {
        auto mk = [&]() {
            hclib::loop_domain_2d L(d[0].low, d[0].high, d[1].low, d[1].high);
            set_dims(L.get_internal(), d, 2);
            return L;
        };
        auto L0 = mk(), L1 = mk(), L2 = mk(), L3 = mk();
        rc[0] = hclib::hip::forasync2D(&L0, [=] __device__(int i, int j) {
            const long long l = linear(i, j, 0);
            sv += l;
            mv.update(l);
            ov |= (int)(l == last);
        }, mode);
        rc[1] = hclib::hip::forasync2D_gather(&L1, gs, [=] __device__(int i, int j) { return linear(i, j, 0); }, mode);
        rc[2] = hclib::hip::forasync2D_gather(&L2, gm, [=] __device__(int i, int j) { return linear(i, j, 0); }, mode);
        rc[3] = hclib::hip::forasync2D_gather(&L3, go,
                                              [=] __device__(int i, int j) { return (int)(linear(i, j, 0) == last); }, mode);
    } else {
        auto mk = [&]() {
            hclib::loop_domain_3d L(d[0].low, d[0].high, d[1].low, d[1].high, d[2].low, d[2].high);
            set_dims(L.get_internal(), d, 3);
            return L;
        };
        auto L0 = mk(), L1 = mk(), L2 = mk(), L3 = mk();
        rc[0] = hclib::hip::forasync3D(&L0, [=] __device__(int i, int j, int k) {
            const long long l = linear(i, j, k);
            sv += l;
            mv.update(l);
            ov |= (int)(l == last);
        }, mode);
        rc[1] = hclib::hip::forasync3D_gather(&L1, gs, [=] __device__(int i, int j, int k) { return linear(i, j, k); },
                                              mode);
        rc[2] = hclib::hip::forasync3D_gather(&L2, gm, [=] __device__(int i, int j, int k) { return linear(i, j, k); },
                                              mode);
        rc[3] = hclib::hip::forasync3D_gather(
            &L3, go, [=] __device__(int i, int j, int k) { return (int)(linear(i, j, k) == last); }, mode);
    }
    for (int r : rc) CHECK(r == HCLIB_HIP_OK, "forasync%dD: %s", ND, hclib_hip_last_error());
    const long long a = s.get(), b = m.get(), ga = gs.get(), gb = gm.get();
    const int c = o.get(), gc = go.get();
    CHECK(a == w.sum && b == w.max && c == w.flag,
          "forasync%dD {%d,%d,%d,%d}.. mode %d lambda updates: sum %lld max %lld or %d, want %lld %lld %d", ND, d[0].low,
          d[0].high, d[0].stride, d[0].tile, mode, a, b, c, w.sum, w.max, w.flag);
    CHECK(ga == w.sum && gb == w.max && gc == w.flag,
          "forasync%dD_gather {%d,%d,%d,%d}.. mode %d: sum %lld max %lld or %d, want %lld %lld %d", ND, d[0].low,
          d[0].high, d[0].stride, d[0].tile, mode, ga, gb, gc, w.sum, w.max, w.flag);
}

// ------------------------------------------------------ a Kind with views
// a complete binary tree: template {depth of the children, index of the
// parent}; child k is node (depth, 2 * parent + k)
constexpr int kTreeDepth = 12;
struct TreeCtx {
    hx::AtomicView<unsigned long long, hx::Sum> nodes;
    hx::AtomicView<int, hx::Max> depth;
    hx::AtomicView<int, hx::Or> found;
};
struct TreeKind {
    static constexpr int kTmplWords = 2;
    static constexpr int kWords = 4;
    static constexpr bool kPure = false;  // the atomics are side effects: lanes run different tasks
    static constexpr bool kBoundedChildren = true;
    using Ctx = TreeCtx;
    struct Acc {
        __device__ void flush(hx::SchedGlobals *) {}
    };
    __device__ static int roots(const Ctx &, Acc &, uint32_t *t) {
        t[0] = 0;
        t[1] = 0;
        return 1;
    }
    __device__ static int process(const Ctx &c, Acc &, const uint32_t *t, uint32_t k, uint32_t *child, uint32_t *,
                                  bool) {
        const int depth = (int)t[0];
        const uint32_t idx = 2u * t[1] + k;
        c.nodes += 1ull;
        c.depth.update(depth);
        c.found |= (int)(depth == kTreeDepth && idx == (1u << kTreeDepth) - 1u);
        if (depth == kTreeDepth) return 0;
        child[0] = (uint32_t)depth + 1u;
        child[1] = idx;
        return 2;
    }
};

__global__ __launch_bounds__(256) void k_two(hx::AtomicView<int, hx::Sum> a, hx::AtomicView<int, hx::Sum> b, int n) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) {
        a += 1;
        b += i;
    }
}

int main() {
    CHECK(hclib_hip_init(0) == HCLIB_HIP_OK, "hclib_hip_init: %s", hclib_hip_last_error());
    check_masks<int32_t>("int32");
    check_masks<int64_t>("int64");
    check_masks<float>("float");
    check_masks<double>("double");

    // the domains and modes of tests/test_gpu.py CASES_1D, both modes each;
    // FLAT {10, 100, 1, 33} overruns to 108
    const Dom c1[] = {{10, 100, 1, 33}, {0, 1000, 3, 7}, {5, 777, 4, -1}, {0, 0, 1, 5}, {3, 4, 1, 1}, {0, 4096, 1, 1}};
    for (const Dom &d : c1)
        for (int mode : {FORASYNC_MODE_FLAT, FORASYNC_MODE_RECURSIVE}) check_domain<1>(&d, mode);
    {
        const Dom q{10, 100, 1, 33};
        const Want w = want_of(&q, 1, FORASYNC_MODE_FLAT);
        long long s = 0;
        for (int i = 10; i <= 108; ++i) s += linear(i, 0, 0);
        CHECK(w.sum == s && w.count == 99, "FLAT {10,100,1,33}: the host set is not 10..108");
    }
    printf("forasync1D lambdas and forasync1D_gather: sum / max / or on 6 domains x 2 modes\n");
    const Dom c2[2] = {{0, 37, 1, 5}, {3, 50, 2, 7}};
    const Dom c3[3] = {{2, 17, 3, 4}, {1, 9, 1, 2}, {0, 5, 2, 2}};
    for (int mode : {FORASYNC_MODE_FLAT, FORASYNC_MODE_RECURSIVE}) {
        check_domain<2>(c2, mode);
        check_domain<3>(c3, mode);
    }
    printf("forasync2D / 3D lambdas and _gather: sum / max / or, FLAT and RECURSIVE\n");

    // a user Kind on run_tasks; a second launch accumulates; reset restores
    {
        atomic_sum_t<unsigned long long> nodes(0);
        atomic_max_t<int> depth(std::numeric_limits<int>::lowest());
        atomic_or_t<int> found(0);
        CHECK(nodes.ok() && depth.ok() && found.ok(), "atomic create: %s", hclib_hip_last_error());
        const TreeCtx ctx{nodes.view(), depth.view(), found.view()};
        const unsigned long long want = (2ull << kTreeDepth) - 1ull;  // 8191
        int rc = hclib::hip::run_tasks<TreeKind>(ctx);
        CHECK(rc == HCLIB_HIP_OK, "run_tasks<TreeKind>: %s", hclib_hip_last_error());
        CHECK(nodes.get() == want && depth.get() == kTreeDepth && found.get() == 1,
              "tree kind: %llu nodes, depth %d, found %d; want %llu, %d, 1", nodes.get(), depth.get(), found.get(), want,
              kTreeDepth);
        printf("user Kind on run_tasks: %llu nodes, max depth %d, flag %d\n", nodes.get(), depth.get(), found.get());
        rc = hclib::hip::run_tasks<TreeKind>(ctx);
        CHECK(rc == HCLIB_HIP_OK, "run_tasks<TreeKind>: %s", hclib_hip_last_error());
        CHECK(nodes.get() == 2 * want, "two launches without a reset: %llu nodes, want %llu", nodes.get(), 2 * want);
        CHECK(nodes.reset() == 0 && depth.reset() == 0 && found.reset() == 0, "reset: %s", hclib_hip_last_error());
        CHECK(nodes.get() == 0 && depth.get() == std::numeric_limits<int>::lowest() && found.get() == 0,
              "after reset: %llu, %d, %d", nodes.get(), depth.get(), found.get());
        printf("accumulation over two launches, then reset to the defaults\n");
    }
    // a non-zero default reads back, counts once, and survives a reset; two
    // atomics updated by one kernel keep their own values
    {
        atomic_sum_t<int> a(7), b(-3);
        CHECK(a.ok() && b.ok(), "atomic create: %s", hclib_hip_last_error());
        CHECK(a.get() == 7 && b.get() == -3, "defaults read %d, %d", a.get(), b.get());
        const int n = 1000;
        hipLaunchKernelGGL(k_two, dim3(4), dim3(256), 0, nullptr, a.view(), b.view(), n);
        CHECK(hipGetLastError() == hipSuccess, "k_two launch");
        CHECK(a.get() == 7 + n && b.get() == -3 + n * (n - 1) / 2, "two atomics: %d, %d", a.get(), b.get());
        CHECK(a.reset() == 0, "reset: %s", hclib_hip_last_error());
        CHECK(a.get() == 7 && b.get() == -3 + n * (n - 1) / 2, "reset of one atomic: %d, %d", a.get(), b.get());
        printf("two atomics in one kernel, non-zero defaults, reset of one\n");
    }
    // a 64-bit sum past 2^32
    {
        atomic_sum_t<uint64_t> big(0);
        CHECK(big.ok(), "atomic create: %s", hclib_hip_last_error());
        const auto v = big.view();
        hclib::loop_domain_1d L(100000);
        int rc = hclib::hip::forasync1D(&L, [=] __device__(int) { v += (uint64_t)0x10000; });
        CHECK(rc == HCLIB_HIP_OK, "forasync1D: %s", hclib_hip_last_error());
        uint64_t want = 0;
        for (int i = 0; i < 100000; ++i) want += 0x10000;
        CHECK(big.get() == want && want > (1ull << 32), "u64 sum %llu, want %llu", (unsigned long long)big.get(),
              (unsigned long long)want);
        printf("u64 sum of 100000 x 0x10000 = %llu\n", (unsigned long long)want);
    }
    printf("Check results: OK\n");
    return 0;
}
