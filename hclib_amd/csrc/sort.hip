// sort.hip — BOTS sort (cilksort: test/performance-regression/full-apps/bots/
// sort, sort.ref.c:315-423 the algorithm, sort.c the HClib port) as a
// fork-join client of dynamic device dataflow (include/hclib_hip/hx_dyn.h):
// one device task per call of the reference's call tree, created on the
// device while the launch runs, with the reference's finish scopes as
// dyn_finish_open / _check_in / _check_out.
//
//   task                       does (reference lines)
//   SORT(lo, size, fin)        size < sort_cutoff: sort the keys in LDS and
//                              check out of fin (:390-394). Otherwise (:395-413)
//                              f1 = open(4), four SORT tasks into f1 (quarters
//                              A B C, D takes the remainder) and MERGE_PHASE
//                              awaiting f1; fin passes to the continuation
//   MERGE_PHASE(lo, size, fin) f2 = open(2), MERGE(A, B -> tmpA, f2) and
//                              MERGE(C, D -> tmpC, f2) (:415-420), and the third
//                              merge MERGE(tmpA.., tmpC.. -> A, fin) (:422, a plain
//                              call in the reference) awaiting f2
//   MERGE(r1, r2, dest, fin)   cilkmerge (:315-376): the larger range first;
//                              the smaller empty: copy; the smaller at most
//                              merge_cutoff keys: merge; otherwise split r1 at
//                              its middle, binsplit that key in r2, store it
//                              at its place in dest, check two tasks in to fin
//                              (no scope per split) and spawn the two halves
//
// The root SORT (fin = kDynOpen in its payload) opens the program's outer
// finish, so every task of the launch belongs to a scope.
//
// The empty-range copy moves high1 - low1 + 1 keys: the reference's memcpy
// (:344) is one key short, which mis-sorts e.g. descending input
// (DESIGN.md §11).
//
// Keys live in one buffer of 2 n int64: the array and the reference's tmp.
// Bodies are wave-wide (one task = one wave, 16 KB of LDS). Every key is
// stored write-through (agent scope, sc1) and drained by the task's check-out
// (dyn_finish_check_out<true>); keys are read with plain loads behind
// run_dyn_worker's acquire (kSc1Payload = false). The other valid form, plain
// stores released by a fence in every leaf's check-out, is kept behind
// HCLIB_HIP_SORT_SC1=0: 18.9 ms against 13.0 ms for 32 Mi keys.
#include <limits.h>
#include <string.h>

#include <map>
#include <vector>

#include "hx_client.h"

namespace hx {
namespace {

constexpr int kSortLdsKeys = 2048;             // 16 KB per wave
constexpr uint32_t kSortTile = kSortLdsKeys / 2;  // keys per output tile of a leaf merge (inputs + staged output)
constexpr uint32_t kSortPerLane = kSortTile / 64;
constexpr int kSortWords = 8;                  // payload words per task
constexpr int kSortWavesPerCu = 8;             // 8 x 16 KB of LDS per CU
enum : uint32_t { kSortTask = 0, kSortPhase = 1, kSortMerge = 2 };
enum : int { kCntSortLeaf = 0, kCntSortSplit = 1, kCntMergeLeaf = 2, kCntMergeSplit = 3, kCntMergeEmpty = 4, kCntPhase = 5,
             kCntKinds = 6 };

struct SortCtx {
    long long *keys;             // [2][n]: the array, tmp
    unsigned long long *counts;  // per task class (hx_client.h class_count)
    uint32_t n, merge_cutoff, sort_cutoff;
    uint32_t sc1;  // leaves store keys write-through (sc1) and check out with a drain instead of a release
};

__device__ __forceinline__ long long *sort_lds() {
    __shared__ __attribute__((aligned(16))) long long s[kSortLdsKeys];
    return s;
}

// a key a leaf writes: a plain store, released by the check-out's fence, or
// (sc1) a write-through store the check-out only drains
__device__ __forceinline__ void sort_store(long long *p, long long v, bool sc1) {
    if (sc1) st_agent(p, v);
    else *p = v;
}

__device__ __forceinline__ void sort_check_out(DynWave &w, uint32_t fin, bool sc1) {
    if (sc1) dyn_finish_check_out<true>(w, fin);
    else dyn_finish_check_out<false>(w, fin);
}

// seqquick's result (:197-208) for k[0 .. size), size < 2048: a bitonic network
// over the next power of two in LDS, the tail padded with the largest key (a
// real key of that value is equal to its padding; only `size` keys go back)
__device__ void sort_leaf(long long *k, uint32_t size, bool sc1) {
    long long *s = sort_lds();
    const uint32_t lane = (uint32_t)lane_id();
    uint32_t P = 2;
    while (P < size) P <<= 1;
    for (uint32_t x = lane; x < P; x += 64) s[x] = x < size ? k[x] : LLONG_MAX;
    __syncthreads();
    for (uint32_t kk = 2; kk <= P; kk <<= 1)
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < P / 2; t += 64) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const long long a = s[i], b = s[l];
                if ((a > b) == ((i & kk) == 0)) {
                    s[i] = b;
                    s[l] = a;
                }
            }
            __syncthreads();
        }
    for (uint32_t x = lane; x < size; x += 64) sort_store(&k[x], s[x], sc1);
}

// The merge-path split of diagonal d: how many of the first d merged keys come
// from A, where a key of A goes out only if it is smaller than B's (`a1 < a2`,
// :245: ties take B's first). lo / hi bracket the answer; every lo <= i < hi
// has A[i] and B[d - i - 1] in range.
template <class PA, class PB>
__device__ __forceinline__ uint32_t merge_path(PA A, PB B, uint32_t d, uint32_t lo, uint32_t hi) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (B[d - mid - 1] <= A[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// seqmerge's result (:210-282): A[0 .. nA) and B[0 .. nB) into D. Either run
// may be far longer than LDS (only the smaller is bounded, by merge_cutoff), so
// the output goes tile by tile: a merge-path split in global memory bounds the
// tile's inputs, which fit in half the LDS; each lane then finds its own
// split in LDS, merges 16 keys into the other half, and the tile goes out
// with coalesced stores.
__device__ void merge_leaf(const long long *A, uint32_t nA, const long long *B, uint32_t nB, long long *D,
                           bool sc1) {
    long long *s = sort_lds(), *out = s + kSortTile;
    const uint32_t lane = (uint32_t)lane_id(), total = nA + nB;
    uint32_t i0 = 0, j0 = 0;
    for (uint32_t o = 0; o < total; o += kSortTile) {
        const uint32_t tn = total - o < kSortTile ? total - o : kSortTile, d = o + tn;
        uint32_t i1 = nA;
        if (d < total) {
            const uint32_t lo = d > nB ? (d - nB > i0 ? d - nB : i0) : i0;
            const uint32_t hi = nA < d - j0 ? nA : d - j0;
            i1 = merge_path(A, B, d, lo, hi);
        }
        const uint32_t j1 = d - i1, a = i1 - i0, b = j1 - j0;  // a + b == tn
        for (uint32_t x = lane; x < tn; x += 64) s[x] = x < a ? A[i0 + x] : B[j0 + (x - a)];
        __syncthreads();
        const long long *sA = s, *sB = s + a;
        const uint32_t d0 = lane * kSortPerLane < tn ? lane * kSortPerLane : tn;
        uint32_t i = merge_path(sA, sB, d0, d0 > b ? d0 - b : 0u, a < d0 ? a : d0), j = d0 - i;
        for (uint32_t r = 0; r < kSortPerLane; ++r)
            if (d0 + r < tn) {
                const bool take_a = i < a && (j >= b || sA[i] < sB[j]);
                out[d0 + r] = take_a ? sA[i] : sB[j];
                i += take_a ? 1u : 0u;
                j += take_a ? 0u : 1u;
            }
        __syncthreads();
        for (uint32_t x = lane; x < tn; x += 64) sort_store(&D[o + x], out[x], sc1);
        __syncthreads();  // the next tile's loads overwrite s
        i0 = i1;
        j0 = j1;
    }
}

// binsplit (:292-312) over r[0 .. n), n >= 1: how many keys of r fall into the
// lower half, i.e. (the index it returns) + 1
__device__ __forceinline__ uint32_t sort_binsplit(long long val, const long long *r, uint32_t n) {
    uint32_t lo = 0, hi = n - 1;
    while (lo != hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (val <= r[mid]) hi = mid - 1;
        else lo = mid;
    }
    return r[lo] > val ? lo : lo + 1;
}

struct SortKind : TimedKind<SortKind, SortCtx> {
    static constexpr bool kSc1Payload = false;  // keys move by plain loads and stores
    // payload: SORT / MERGE_PHASE {kind, lo, size, fin}
    //          MERGE {kind | src << 8, l1, e1, l2, e2, ldest, fin}: ranges [l, e) of array `src`, into the other
    __device__ static void body(const Ctx &c, DynWave &w, const uint32_t *pay, int &which) {
        const uint32_t kind = pay[0] & 0xffu;
        const int lane = lane_id();
        if (kind != kSortMerge && (pay[2] == 0 || (unsigned long long)pay[1] + pay[2] > c.n)) {
            if (lane == 0) dev_error(dyn_err(w.v), kErrBadTask);
            return;
        }
        if (kind == kSortTask) {
            const uint32_t lo = pay[1], size = pay[2];
            // the root has no scope yet: it opens the program's outer finish, checked in once, for itself
            const uint32_t fin = pay[3] == kDynOpen ? dyn_finish_open(w, 1) : pay[3];
            if (size < c.sort_cutoff) {
                sort_leaf(c.keys + lo, size, c.sc1 != 0);
                which = kCntSortLeaf;
                sort_check_out(w, fin, c.sc1 != 0);
                return;
            }
            which = kCntSortSplit;
            const uint32_t q = size / 4, f1 = dyn_finish_open(w, 4);
            // lanes 0-3: SORT A, B, C, D into f1; lane 4: the continuation, awaiting f1
            uint32_t pl[kSortWords] = {kSortTask, lo + (uint32_t)lane * q, lane == 3 ? size - 3 * q : q, f1, 0, 0, 0, 0};
            uint32_t fut[1] = {kDynOpen};
            if (lane == 4) {
                pl[0] = kSortPhase, pl[1] = lo, pl[2] = size, pl[3] = fin;
                fut[0] = f1;
            }
            dyn_async_await<true>(w, lane < 5, pl, fut, 1);
            return;
        }
        if (kind == kSortPhase) {
            const uint32_t lo = pay[1], size = pay[2], fin = pay[3], q = size / 4;
            which = kCntPhase;
            const uint32_t f2 = dyn_finish_open(w, 2);
            // lane 0: A, B -> tmpA; lane 1: C, D -> tmpC; lane 2: tmpA.., tmpC.. -> A, awaiting f2
            uint32_t pl[kSortWords] = {kSortMerge, lo, lo + q, lo + q, lo + 2 * q, lo, f2, 0};
            uint32_t fut[1] = {kDynOpen};
            if (lane == 1) {
                pl[1] = lo + 2 * q, pl[2] = lo + 3 * q, pl[3] = lo + 3 * q, pl[4] = lo + size, pl[5] = lo + 2 * q;
            } else if (lane == 2) {
                pl[0] = kSortMerge | (1u << 8);
                pl[2] = lo + 2 * q, pl[3] = lo + 2 * q, pl[4] = lo + size, pl[6] = fin;
                fut[0] = f2;
            }
            dyn_async_await<true>(w, lane < 3, pl, fut, 1);
            return;
        }
        // MERGE
        const uint32_t src = (pay[0] >> 8) & 1u, ld = pay[5], fin = pay[6];
        uint32_t l1 = pay[1], e1 = pay[2], l2 = pay[3], e2 = pay[4];
        if (l1 > e1 || l2 > e2 || e1 > c.n || e2 > c.n || (unsigned long long)ld + (e1 - l1) + (e2 - l2) > c.n) {
            if (lane == 0) dev_error(dyn_err(w.v), kErrBadTask);
            return;
        }
        if (e2 - l2 > e1 - l1) {  // :338-341
            uint32_t t = l1;
            l1 = l2, l2 = t;
            t = e1, e1 = e2, e2 = t;
        }
        const uint32_t n1 = e1 - l1, n2 = e2 - l2;
        const long long *S = c.keys + (size_t)src * c.n;
        long long *D = c.keys + (size_t)(src ^ 1u) * c.n + ld;
        if (n2 == 0) {  // :342-346, all n1 keys
            for (uint32_t x = (uint32_t)lane; x < n1; x += 64) sort_store(&D[x], S[l1 + x], c.sc1 != 0);
            which = kCntMergeEmpty;
            sort_check_out(w, fin, c.sc1 != 0);
            return;
        }
        if (n2 - 1 < c.merge_cutoff) {  // :347-350
            merge_leaf(S + l1, n1, S + l2, n2, D, c.sc1 != 0);
            which = kCntMergeLeaf;
            sort_check_out(w, fin, c.sc1 != 0);
            return;
        }
        // :358-371
        which = kCntMergeSplit;
        const uint32_t h = n1 / 2;
        const long long val = S[l1 + h];
        const uint32_t cnt = sort_binsplit(val, S + l2, n2);  // r2's keys in the lower half
        if (lane == 0) st_agent(&D[h + cnt], val);
        dyn_finish_check_in(w, fin, 2);
        uint32_t pl[kSortWords] = {pay[0], l1, l1 + h, l2, l2 + cnt, ld, fin, 0};
        if (lane == 1) pl[1] = l1 + h + 1, pl[2] = e1, pl[3] = l2 + cnt, pl[4] = e2, pl[5] = ld + h + cnt + 1;
        dyn_async_await<true>(w, lane < 2, pl, nullptr, 0);
        dyn_finish_check_out<true>(w, fin);
    }
};

__global__ __launch_bounds__(64) void k_sort(SortCtx c, DynView v) { run_dyn_worker<SortKind>(c, v); }

ClassCounters<kCntKinds> g_sort;  // the last launch's

// ---------------------------------------------------------------- pool bound
// The sort tree depends on n and sort_cutoff alone, so its SORT and MERGE_PHASE
// tasks, its scopes (two per split, and the root's) and its wait nodes (one per
// split scope: its one awaiting continuation) are counted exactly. A merge root's tree depends on
// the keys. Its nodes are splits, leaves and empties, every split has two
// children, so nodes = 2 splits + 1. A split needs the smaller range to hold
// at least K = merge_cutoff + 1 keys, so the node at least 2 K; it puts one key
// and hands the rest to its children, and each child gets at least half of the
// larger range less one, that is at least H - 1 keys with H = ceil(K / 2). By
// induction a root of m keys has at most max(0, floor(m / H) - 1) splits: with
// no child that can split, 1 <= floor(m / H) - 1 as m >= 2 K >= 2 H; with one,
// of a keys, floor(a / H) - 1 + 1 <= floor(m / H) - 1 as m >= a + H; with two,
// floor(a / H) + floor(b / H) - 1 <= floor(m / H) - 1.
struct SortBound {
    unsigned long long tasks, scopes;
};

unsigned long long merge_nodes_bound(unsigned long long m, unsigned long long mc) {
    const unsigned long long K = mc + 1, H = (K + 1) / 2;
    if (m < 2 * K) return 1;
    return 2 * (m / H - 1) + 1;
}

SortBound sort_bound(unsigned long long size, unsigned long long mc, unsigned long long sc,
                     std::map<unsigned long long, SortBound> &memo) {
    if (size < sc) return {1, 0};
    auto it = memo.find(size);
    if (it != memo.end()) return it->second;
    const unsigned long long q = size / 4;
    const SortBound a = sort_bound(q, mc, sc, memo), d = sort_bound(size - 3 * q, mc, sc, memo);
    SortBound r;
    r.tasks = 2 + 3 * a.tasks + d.tasks + merge_nodes_bound(2 * q, mc) + merge_nodes_bound(size - 2 * q, mc) +
              merge_nodes_bound(size, mc);
    r.scopes = 2 + 3 * a.scopes + d.scopes;
    memo[size] = r;
    return r;
}

int sort_check_args(const char *who, bool keys_ok, int64_t n, int &merge_cutoff, int &sort_cutoff) {
    if (!keys_ok) {
        set_error("%s: keys must not be NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    if (n < 1 || n >= (1ll << 31)) {
        set_error("%s: n = %lld must be in 1 .. 2^31 - 1", who, (long long)n);
        return HCLIB_HIP_EINVAL;
    }
    if (merge_cutoff == 0) merge_cutoff = 2048;
    if (sort_cutoff == 0) sort_cutoff = 2048;
    if (merge_cutoff < 2) {  // sort.ref.c:456-459
        set_error("%s: merge_cutoff = %d can not be less than 2", who, merge_cutoff);
        return HCLIB_HIP_EINVAL;
    }
    if (sort_cutoff < 4 || sort_cutoff > kSortLdsKeys) {  // below 4 a quarter is empty and the recursion never ends
        set_error("%s: sort_cutoff = %d must be in 4 .. %d", who, sort_cutoff, kSortLdsKeys);
        return HCLIB_HIP_EINVAL;
    }
    return HCLIB_HIP_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_sort_bounds(int64_t n, int merge_cutoff, int sort_cutoff, uint64_t out[3]) {
    if (!out) {
        set_error("hclib_hip_sort_bounds: out must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    HX_TRY(sort_check_args("hclib_hip_sort_bounds", true, n, merge_cutoff, sort_cutoff));
    std::map<unsigned long long, SortBound> memo;
    const SortBound b = sort_bound((unsigned long long)n, (unsigned long long)merge_cutoff,
                                   (unsigned long long)sort_cutoff, memo);
    out[0] = b.tasks;
    out[1] = b.scopes + 1;  // promises: the scopes and the root's outer finish
    out[2] = b.scopes;  // wait nodes
    return HCLIB_HIP_OK;
}

extern "C" void hclib_hip_sort_last_ticks(uint64_t out[6]) {
    for (int k = 0; k < kCntKinds; ++k) out[k] = g_sort.ticks[k];
}

extern "C" int hclib_hip_sort_i64(int64_t *keys, int64_t n, int merge_cutoff, int sort_cutoff,
                                  hclib_hip_sort_result_t *result) {
    // argument errors first, before the device is touched
    HX_TRY(sort_check_args("hclib_hip_sort_i64", keys != nullptr, n, merge_cutoff, sort_cutoff));
    uint64_t cap[3];
    HX_TRY(hclib_hip_sort_bounds(n, merge_cutoff, sort_cutoff, cap));
    if (cap[0] >= 0xfffffff0ull) {
        set_error("hclib_hip_sort_i64: n = %lld at merge_cutoff = %d, sort_cutoff = %d may need %llu tasks (at most "
                  "2^32 - 17): use larger cutoffs", (long long)n, merge_cutoff, sort_cutoff,
                  (unsigned long long)cap[0]);
        return HCLIB_HIP_EINVAL;
    }
    HX_TRY(ensure_device());
    Module &m = mod();

    // [counts: a line per task class][array n][tmp n]
    const size_t hdr = g_sort.kBytes, kbytes = (size_t)n * sizeof(int64_t), bytes = hdr + 2 * kbytes;
    char *d = nullptr;
    HX_TRY(arena_reserve(kArenaSort, bytes, "hclib_hip_sort_i64", (void **)&d));
    // (`keys` outlives the copy: launch_dyn synchronises the stream)
    HX_HIP(hipMemcpyAsync(d + hdr, keys, kbytes, hipMemcpyHostToDevice, m.stream));

    SortCtx c;
    c.keys = (long long *)(d + hdr);
    c.counts = (unsigned long long *)d;
    c.n = (uint32_t)n;
    c.merge_cutoff = (uint32_t)merge_cutoff;
    c.sort_cutoff = (uint32_t)sort_cutoff;
    // (HCLIB_HIP_SORT_SC1=0: plain stores and a release fence per leaf, measured slower)
    c.sc1 = env_int("HCLIB_HIP_SORT_SC1", 1) ? 1u : 0u;
    const uint32_t root[kSortWords] = {kSortTask, 0u, (uint32_t)n, kDynOpen, 0, 0, 0, 0};
    // (HCLIB_HIP_SORT_WAVES_PER_CU: for measurements; 8 waves of 16 KB fill the LDS best)
    int wpc = env_int("HCLIB_HIP_SORT_WAVES_PER_CU", kSortWavesPerCu);
    wpc = wpc < 1 ? 1 : (wpc > kSortWavesPerCu ? kSortWavesPerCu : wpc);
    hclib_hip_dyn_stats_t st{};
    uint64_t fin[2] = {0, 0};
    const int rc = launch_dyn(kSortWords, root, cap[0], cap[1], cap[2], wpc, "hclib_hip_sort_i64", d, g_sort, &st, fin,
                              [&](int grid, const DynView &v) {
                                  hipLaunchKernelGGL(k_sort, dim3(grid), dim3(64), 0, m.stream, c, v);
                              });
    if (result) {
        result->tasks = st.tasks;
        result->sort_leaf = g_sort.tasks[kCntSortLeaf];
        result->sort_split = g_sort.tasks[kCntSortSplit];
        result->merge_leaf = g_sort.tasks[kCntMergeLeaf];
        result->merge_split = g_sort.tasks[kCntMergeSplit];
        result->merge_empty = g_sort.tasks[kCntMergeEmpty];
        result->finishes = fin[0];
        result->check_ins = fin[1];
        result->kernel_ms = st.kernel_ms;
        result->keys_per_s = st.kernel_ms > 0 ? (double)n / (st.kernel_ms * 1e-3) : 0.0;
    }
    if (rc) return rc;
    HX_HIP(hipMemcpy(keys, c.keys, kbytes, hipMemcpyDeviceToHost));
    return HCLIB_HIP_OK;
}
