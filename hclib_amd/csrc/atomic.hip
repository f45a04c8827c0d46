// atomic.hip — privatised atomics: the host drop-in of inc/hclib_atomic.h and
// the device atomics behind hx::AtomicView (include/hclib_hip/hx_atomic.h).
//
// Host (src/hclib_atomic.c:3-54): one padded element per host worker, updated
// by the worker that runs the task, folded by hclib_atomic_gather.
//
// Device: nslots 128-byte slots in HBM, one per wave of the largest launch
// this library makes, plus one result word. Waves update their own slot
// (hx_atomic.h); k_atomic_gather folds the slots with one workgroup in a
// fixed order, so a value depends on the launch shapes that produced the
// slots and on nothing else. hclib_hip_forasync_reduce is the reducing sweep
// with the built-in body update(x[i]): partials stay in registers, every
// wave touches its slot once.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/hclib_atomic.h"
#include "../../include/hclib_forasync_sets.h"
#include "../../include/hclib_hip/hx_atomic.h"
#include "hx_module.h"

// ------------------------------------------------------------------- host
extern "C" {

void hclib_atomic_init(hclib_atomic_t *atomic, const size_t ele_size_in_bytes, atomic_init_func init,
                       void *user_data) {
    if (!atomic || !init || ele_size_in_bytes == 0) {
        fprintf(stderr, "hclib_atomic_init: needs storage, an init callback and a non-zero element size\n");
        abort();
    }
    const size_t line = CACHE_LINE_LEN_IN_BYTES;
    atomic->nthreads = (size_t)hclib_get_num_workers();
    atomic->val_size = ele_size_in_bytes;
    atomic->padded_val_size = (ele_size_in_bytes + line - 1) / line * line;
    atomic->vals = NULL;
    if (posix_memalign((void **)&atomic->vals, line, atomic->nthreads * atomic->padded_val_size) != 0) {
        fprintf(stderr, "hclib_atomic_init: out of memory\n");
        abort();
    }
    memset(atomic->vals, 0, atomic->nthreads * atomic->padded_val_size);
    for (size_t w = 0; w < atomic->nthreads; ++w) init(atomic->vals + w * atomic->padded_val_size, user_data);
}

hclib_atomic_t *hclib_atomic_create(const size_t ele_size_in_bytes, atomic_init_func init, void *user_data) {
    hclib_atomic_t *atomic = (hclib_atomic_t *)malloc(sizeof(hclib_atomic_t));
    if (!atomic) {
        fprintf(stderr, "hclib_atomic_create: out of memory\n");
        abort();
    }
    hclib_atomic_init(atomic, ele_size_in_bytes, init, user_data);
    return atomic;
}

void hclib_atomic_update(hclib_atomic_t *atomic, atomic_update_func f, void *user_data) {
    const size_t w = (size_t)hclib_get_current_worker();
    f(atomic->vals + w * atomic->padded_val_size, user_data);
}

void *hclib_atomic_gather(hclib_atomic_t *atomic, atomic_gather_func f, void *user_data) {
    char *out = (char *)malloc(atomic->padded_val_size);
    if (!out) {
        fprintf(stderr, "hclib_atomic_gather: out of memory\n");
        abort();
    }
    memcpy(out, atomic->vals, atomic->padded_val_size);
    for (size_t w = 1; w < atomic->nthreads; ++w) f(out, atomic->vals + w * atomic->padded_val_size, user_data);
    return out;
}

}  // extern "C"

// ----------------------------------------------------------------- device
struct hclib_hip_atomic {
    int dtype, op;
    uint32_t nslots, stride;
    char *mem;        // nslots * stride bytes of slots, then the result line
    uint64_t start;   // bits every slot is reset to
    uint64_t base;    // bits folded in once at the gather (SUM: the default)
};

namespace hx {

constexpr int kGatherThreads = 1024;
constexpr int kReduceThreads = 256;

static size_t dtype_size(int dtype) {
    return (dtype == HCLIB_HIP_ATOMIC_I32 || dtype == HCLIB_HIP_ATOMIC_U32 || dtype == HCLIB_HIP_ATOMIC_F32) ? 4 : 8;
}

__global__ __launch_bounds__(256) void k_atomic_fill(char *slots, uint32_t nslots, uint32_t stride,
                                                     unsigned long long bits, int size) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += gridDim.x * blockDim.x) {
        if (size == 4) *(uint32_t *)(slots + (size_t)i * stride) = (uint32_t)bits;
        else *(unsigned long long *)(slots + (size_t)i * stride) = bits;
    }
}

// One workgroup: thread t folds slots t, t + 1024, ... in that order, then
// the 1024 partials fold pairwise through LDS (t with t + 512, + 256, ...).
// The order is fixed, so the same slot contents always give the same bits.
template <typename T, typename Op>
__global__ __launch_bounds__(kGatherThreads) void k_atomic_gather(const char *slots, uint32_t nslots, uint32_t stride,
                                                                  T base, T *out) {
    __shared__ T part[kGatherThreads];
    const int t = (int)threadIdx.x;
    T acc = Op::template identity<T>();
    for (uint32_t i = (uint32_t)t; i < nslots; i += kGatherThreads)
        acc = Op::template combine<T>(acc, ld_agent((const T *)(slots + (size_t)i * stride)));
    part[t] = acc;
    __syncthreads();
    for (int s = kGatherThreads / 2; s > 0; s >>= 1) {
        if (t < s) part[t] = Op::template combine<T>(part[t], part[t + s]);
        __syncthreads();
    }
    if (t == 0) *out = Op::template combine<T>(base, part[0]);
}

// ---------------------------------------------------------- reducing sweep
template <typename T>
struct Vec16 {
    static constexpr int N = 16 / (int)sizeof(T);
    typedef T type __attribute__((ext_vector_type(16 / sizeof(T))));
};

// x[0, n): `head` elements up to the first 16-byte boundary, then nv 16-byte
// vectors swept grid-stride (UNROLL independent loads per lane in flight),
// then the tail; head and tail are fewer than N elements each and go to the
// first threads of the grid. Lane partials live in registers, one slot update
// per wave at the end (every lane active: the full-wave path of update()).
template <typename T, typename Op, int UNROLL>
__global__ __launch_bounds__(kReduceThreads) void k_reduce_contig(const T *__restrict__ x, int64_t n, int64_t head,
                                                                  AtomicView<T, Op> a) {
    using V = typename Vec16<T>::type;
    constexpr int N = Vec16<T>::N;
    const int64_t gt = (int64_t)blockIdx.x * kReduceThreads + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * kReduceThreads;
    const int64_t nv = (n - head) / N;
    const V *xv = reinterpret_cast<const V *>(x + head);
    T acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = Op::template identity<T>();
    int64_t i = gt;
    for (; i + (UNROLL - 1) * step < nv; i += UNROLL * step) {
        V v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) v[u] = __builtin_nontemporal_load(&xv[i + u * step]);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] = Op::template combine<T>(acc[e], v[u][e]);
    }
    for (; i < nv; i += step) {
        const V v = __builtin_nontemporal_load(&xv[i]);
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = Op::template combine<T>(acc[e], v[e]);
    }
    const int64_t tail = head + nv * N;
    if (gt < head) acc[0] = Op::template combine<T>(acc[0], x[gt]);
    if (tail + gt < n) acc[0] = Op::template combine<T>(acc[0], x[tail + gt]);
    T r = acc[0];
#pragma unroll
    for (int e = 1; e < N; ++e) r = Op::template combine<T>(r, acc[e]);
    a.update(r);
}

// any other 1-D set: iteration t of the sweep -> index through the run table
// (hclib_hip_forasync_plan: runs + prefix counts, binary search)
template <typename T, typename Op>
__global__ __launch_bounds__(kReduceThreads) void k_reduce_runs(const T *__restrict__ x, hclib_hip_sweep_plan_t p,
                                                                AtomicView<T, Op> a) {
    const int64_t step = (int64_t)gridDim.x * kReduceThreads;
    T acc = Op::template identity<T>();
    for (int64_t t = (int64_t)blockIdx.x * kReduceThreads + threadIdx.x; t < p.total; t += step) {
        int lo = 0, hi = p.nruns[0] - 1;
        while (lo < hi) {  // the last run with prefix <= t
            const int mid = (lo + hi + 1) >> 1;
            if (p.prefix[0][mid] <= t) lo = mid;
            else hi = mid - 1;
        }
        const hclib_hip_run_t r = p.runs[0][lo];
        acc = Op::template combine<T>(acc, x[r.first + (int64_t)(t - p.prefix[0][lo]) * r.stride]);
    }
    a.update(acc);
}

// dtype x op -> one instantiation
template <template <typename, typename> class F, typename T, typename... A>
static int dispatch_op(int op, A... args) {
    switch (op) {
    case HCLIB_HIP_ATOMIC_SUM: return F<T, Sum>::run(args...);
    case HCLIB_HIP_ATOMIC_MAX: return F<T, Max>::run(args...);
    default: return F<T, Or>::run(args...);
    }
}
template <template <typename, typename> class F, typename... A>
static int dispatch(int dtype, int op, A... args) {
    switch (dtype) {
    case HCLIB_HIP_ATOMIC_I32: return dispatch_op<F, int32_t>(op, args...);
    case HCLIB_HIP_ATOMIC_U32: return dispatch_op<F, uint32_t>(op, args...);
    case HCLIB_HIP_ATOMIC_I64: return dispatch_op<F, int64_t>(op, args...);
    case HCLIB_HIP_ATOMIC_U64: return dispatch_op<F, uint64_t>(op, args...);
    case HCLIB_HIP_ATOMIC_F32: return dispatch_op<F, float>(op, args...);
    default: return dispatch_op<F, double>(op, args...);
    }
}

template <typename T>
static T from_bits(uint64_t bits) {
    T v;
    memcpy(&v, &bits, sizeof(T));
    return v;
}

template <typename T, typename Op>
static AtomicView<T, Op> view_of(const hclib_hip_atomic *a) {
    return AtomicView<T, Op>{a->mem, a->nslots, a->stride};
}

template <typename T, typename Op>
struct GatherLaunch {
    static int run(const hclib_hip_atomic *a, hipStream_t st, void *out) {
        hipLaunchKernelGGL((k_atomic_gather<T, Op>), dim3(1), dim3(kGatherThreads), 0, st, (const char *)a->mem,
                           a->nslots, a->stride, from_bits<T>(a->base), (T *)out);
        HX_HIP(hipGetLastError());
        return HCLIB_HIP_OK;
    }
};

// the identity's bits: what SUM slots start at and what MAX / OR fold in as base
template <typename T, typename Op>
struct IdentityBits {
    static int run(uint64_t *bits) {
        const T v = Op::template identity<T>();
        *bits = 0;
        memcpy(bits, &v, sizeof(T));
        return HCLIB_HIP_OK;
    }
};

template <typename T, typename Op>
struct ReduceLaunch {
    static int run(const hclib_hip_atomic *a, const void *xp, const hclib_hip_sweep_plan_t *plan, int64_t first,
                   int64_t count, hipStream_t st) {
        const T *x = (const T *)xp;
        const AtomicView<T, Op> v = view_of<T, Op>(a);
        // every wave of the grid owns a slot: at most nslots / 4 workgroups
        const int64_t cap = (int64_t)a->nslots / (kReduceThreads / 64);
        if (!plan) {
            constexpr int N = Vec16<T>::N;
            const T *x0 = x + first;
            const int64_t mis = (int64_t)(((uintptr_t)x0 & 15) / sizeof(T));
            int64_t head = (N - mis) % N;
            if (head > count) head = count;
            const int64_t nv = (count - head) / N;
            // measured on MI355X (scripts/bench_reduce.py --sweep, profiles/r07/reduce_sweep.log,
            // 1 GiB of f32): 32 KiB of loads in flight per CU is the best shape however it
            // is split (8 workgroups x 1 load per lane 7.17 TB/s, 4 x 2 7.13, 2 x 4 7.10);
            // 16 KiB gives 6.6-6.7, 64 KiB and more 5.7-6.0
            const int unroll = env_int("HCLIB_HIP_REDUCE_UNROLL", 1);
            int64_t grid = (int64_t)mod().num_cus * env_int("HCLIB_HIP_REDUCE_BLOCKS_PER_CU", 8);
            const int64_t need = (nv + kReduceThreads - 1) / kReduceThreads;
            if (grid > need) grid = need;
            if (grid > cap) grid = cap;
            if (grid < 1) grid = 1;
            void (*k)(const T *, int64_t, int64_t, AtomicView<T, Op>) =
                unroll >= 8 ? k_reduce_contig<T, Op, 8>
                            : (unroll >= 4 ? k_reduce_contig<T, Op, 4>
                                           : (unroll >= 2 ? k_reduce_contig<T, Op, 2> : k_reduce_contig<T, Op, 1>));
            hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kReduceThreads), 0, st, x0, count, head, v);
        } else {
            int64_t grid = (plan->total + kReduceThreads - 1) / kReduceThreads;
            const int64_t maxg = (int64_t)mod().num_cus * 16;
            if (grid > maxg) grid = maxg;
            if (grid > cap) grid = cap;
            hipLaunchKernelGGL((k_reduce_runs<T, Op>), dim3((unsigned)grid), dim3(kReduceThreads), 0, st, x, *plan, v);
        }
        HX_HIP(hipGetLastError());
        return HCLIB_HIP_OK;
    }
};

static uint32_t pow2_at_least(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

static bool bad_kind(int dtype, int op, const char *who) {
    if (dtype < HCLIB_HIP_ATOMIC_I32 || dtype > HCLIB_HIP_ATOMIC_F64) {
        set_error("%s: dtype %d is not one of HCLIB_HIP_ATOMIC_I32 .. F64", who, dtype);
        return true;
    }
    if (op < HCLIB_HIP_ATOMIC_SUM || op > HCLIB_HIP_ATOMIC_OR) {
        set_error("%s: op %d is not HCLIB_HIP_ATOMIC_SUM, MAX or OR", who, op);
        return true;
    }
    return false;
}

}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_atomic_create(int dtype, int op, const void *default_value, hclib_hip_atomic_t **out) {
    if (out) *out = nullptr;
    if (bad_kind(dtype, op, "hclib_hip_atomic_create")) return HCLIB_HIP_EINVAL;
    if (!default_value || !out) {
        set_error("hclib_hip_atomic_create: NULL default value or result pointer");
        return HCLIB_HIP_EINVAL;
    }
    HX_TRY(ensure_device());
    hclib_hip_atomic *a = new hclib_hip_atomic();
    a->dtype = dtype;
    a->op = op;
    a->stride = HCLIB_HIP_ATOMIC_STRIDE;
    // the widest launches: forasync_device / hclib_hip_forasync sweep 16
    // workgroups of 4 waves per CU; the megakernels run at most 32 waves per CU
    uint32_t workers = (uint32_t)mod().num_cus * 64u;
    if ((uint32_t)hclib_hip_num_workers() > workers) workers = (uint32_t)hclib_hip_num_workers();
    a->nslots = pow2_at_least(workers);
    uint64_t dflt = 0, ident = 0;
    memcpy(&dflt, default_value, dtype_size(dtype));
    int rc = dispatch<IdentityBits>(dtype, op, &ident);
    // SUM: slots at zero, the default added once by the gather; MAX / OR are
    // idempotent, every slot starts at the default
    a->start = op == HCLIB_HIP_ATOMIC_SUM ? ident : dflt;
    a->base = op == HCLIB_HIP_ATOMIC_SUM ? dflt : ident;
    if (rc == HCLIB_HIP_OK &&
        hip_check(hipMalloc((void **)&a->mem, (size_t)a->nslots * a->stride + HCLIB_HIP_ATOMIC_STRIDE), "hipMalloc"))
        rc = HCLIB_HIP_ENOMEM;
    // ready for any stream once create returns
    if (rc == HCLIB_HIP_OK) rc = hclib_hip_atomic_reset(a, nullptr);
    if (rc == HCLIB_HIP_OK) rc = hip_check(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    if (rc != HCLIB_HIP_OK) {
        if (a->mem) (void)hipFree(a->mem);
        delete a;
        return rc;
    }
    *out = a;
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_atomic_destroy(hclib_hip_atomic_t *a) {
    if (!a) {
        set_error("hclib_hip_atomic_destroy: NULL atomic");
        return HCLIB_HIP_EINVAL;
    }
    const int rc = hip_check(hipFree(a->mem), "hipFree");  // hipFree waits for the device
    delete a;
    return rc;
}

extern "C" int hclib_hip_atomic_view(const hclib_hip_atomic_t *a, hclib_hip_atomic_view_t *view) {
    if (!a || !view) {
        set_error("hclib_hip_atomic_view: NULL atomic or view");
        return HCLIB_HIP_EINVAL;
    }
    view->slots = a->mem;
    view->nslots = a->nslots;
    view->stride = a->stride;
    view->dtype = a->dtype;
    view->op = a->op;
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_atomic_reset(hclib_hip_atomic_t *a, void *stream) {
    if (!a) {
        set_error("hclib_hip_atomic_reset: NULL atomic");
        return HCLIB_HIP_EINVAL;
    }
    hipLaunchKernelGGL(k_atomic_fill, dim3((a->nslots + 255) / 256), dim3(256), 0, (hipStream_t)stream, a->mem, a->nslots,
                       a->stride, (unsigned long long)a->start, (int)dtype_size(a->dtype));
    HX_HIP(hipGetLastError());
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_atomic_gather_async(hclib_hip_atomic_t *a, void *stream, void *device_out) {
    if (!a || !device_out) {
        set_error("hclib_hip_atomic_gather_async: NULL atomic or output");
        return HCLIB_HIP_EINVAL;
    }
    return dispatch<GatherLaunch>(a->dtype, a->op, (const hclib_hip_atomic *)a, (hipStream_t)stream, device_out);
}

extern "C" int hclib_hip_atomic_gather(hclib_hip_atomic_t *a, void *stream, void *host_out) {
    if (!a || !host_out) {
        set_error("hclib_hip_atomic_gather: NULL atomic or output");
        return HCLIB_HIP_EINVAL;
    }
    void *word = a->mem + (size_t)a->nslots * a->stride;
    HX_TRY(hclib_hip_atomic_gather_async(a, stream, word));
    HX_HIP(hipMemcpyAsync(host_out, word, dtype_size(a->dtype), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HX_HIP(hipStreamSynchronize((hipStream_t)stream));
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_forasync_reduce(hclib_hip_atomic_t *a, const void *x, int dim, hclib_hip_loop_domain_t *domain,
                                         int mode, void *stream) {
    if (dim != 1) {
        set_error("hclib_hip_forasync_reduce: the built-in body x[i] is 1-D (dim %d)", dim);
        return HCLIB_HIP_EINVAL;
    }
    if (!a || !domain || (mode != 0 && mode != 1)) {
        set_error("hclib_hip_forasync_reduce: needs an atomic, a domain and mode FLAT or RECURSIVE");
        return HCLIB_HIP_EINVAL;
    }
    if (domain[0].stride < 1) {
        set_error("hclib_hip_forasync_reduce: stride must be >= 1");
        return HCLIB_HIP_EINVAL;
    }
    if (!x && domain[0].high > domain[0].low) {
        set_error("hclib_hip_forasync_reduce: NULL x");
        return HCLIB_HIP_EINVAL;
    }
    if (((uintptr_t)x & (dtype_size(a->dtype) - 1)) != 0) {
        set_error("hclib_hip_forasync_reduce: x is not aligned to its element size");
        return HCLIB_HIP_EINVAL;
    }
    HX_TRY(ensure_device());
    hclib_sets::resolve_tile(&domain[0].tile, domain[0].low, domain[0].high, hclib_hip_num_workers());
    const hclib_sets::Domain dd{domain[0].low, domain[0].high, domain[0].stride, domain[0].tile};
    const std::vector<hclib_sets::Run> runs = hclib_sets::runs(dd, 1, mode);
    if (hclib_sets::count(runs) == 0) return HCLIB_HIP_OK;
    if (!x) {
        set_error("hclib_hip_forasync_reduce: NULL x");
        return HCLIB_HIP_EINVAL;
    }
    if (runs.size() == 1 && runs[0].stride == 1)
        return dispatch<ReduceLaunch>(a->dtype, a->op, (const hclib_hip_atomic *)a, x,
                                      (const hclib_hip_sweep_plan_t *)nullptr, (int64_t)runs[0].first,
                                      (int64_t)runs[0].count, (hipStream_t)stream);
    hclib_hip_sweep_plan_t plan;
    HX_TRY(hclib_hip_forasync_plan(1, domain, mode, stream, &plan));
    const int rc = dispatch<ReduceLaunch>(a->dtype, a->op, (const hclib_hip_atomic *)a, x,
                                          (const hclib_hip_sweep_plan_t *)&plan, (int64_t)0, (int64_t)0,
                                          (hipStream_t)stream);
    const int rr = hclib_hip_forasync_plan_release(&plan, stream);
    return rc ? rc : rr;
}
