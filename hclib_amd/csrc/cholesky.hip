// cholesky.hip — the reference's tiled Cholesky (test/cholesky) as one launch of
// the generic device promise DAG (include/hclib_hip/hx_dag.h, run_dag_group).
//
// The reference's item space lkji[j][i][k] holds single-assignment tile
// versions; its driver (test/cholesky/cholesky.cpp:80-124) walks k with two
// finish scopes per step. Here every tile version is one promise and every
// tile kernel one workgroup task:
//
//   task          awaits                      puts        restates
//   potrf(k)      (k,k,k)                     (k,k,k+1)   sequential_cholesky.cpp
//   trsm(k,j)     (j,k,k) (k,k,k+1)           (j,k,k+1)   trisolve.cpp
//   syrk(k,j)     (j,j,k) (j,k,k+1)           (j,j,k+1)   update_diagonal.cpp
//   gemm(k,j,i)   (j,i,k) (i,k,k+1) (j,k,k+1) (j,i,k+1)   update_nondiagonal.cpp
//
// Version-0 promises are left out of the awaits (the host uploaded them), so a
// task's one promise has the task's own id. Tiles are updated in place in one
// buffer of tile-major blocks: version k of a tile has exactly one reader (the
// task that makes version k+1), and a finished L tile is never written again.
//
// Exact mode keeps, for every element, the reference's sequence of rounded
// operations: its updates in ascending global k, each one unfused multiply and
// one unfused add (or subtract, inside potrf / trsm), then one IEEE divide or
// square root. The reference's potrf and trsm are right-looking; the panels
// below are left-looking, which reorders the work between elements but not the
// operations any one element sees, so the result is bit-identical for every
// tile size. (A second mode with the syrk / gemm updates on
// v_mfma_f64_16x16x4_f64 was measured and not kept: DESIGN.md §10.)
//
// Every tile access is an agent-scope (sc1) vector load or write-through store
// (never a scalar load: another task wrote the tile during this launch), the
// payload form run_dag_group hands from task to task behind a drain and a
// barrier, with no L2 write-back or invalidate per task (kSc1Payload; an agent
// release per task serialises in each XCD's L2: 10.9 ms against 8.3 ms for
// 4096 / 64). One workgroup per CU, as that form was measured.
#include <math.h>
#include <string.h>

#include <vector>

#include "hx_client.h"

namespace hx {
namespace {

constexpr int kCholThreads = 256;  // one task = one workgroup of four waves
constexpr int kCholMaxTile = 128;
constexpr int kCholKc = 16;   // k per staged chunk, and the panel width
constexpr int kCholBlk = 64;  // rows / columns of one register block (16 x 16 threads, 4 x 4 each)
constexpr int kCholLdB = kCholBlk + 1;      // padded LDS rows of the update's operands
constexpr int kCholLdP = kCholMaxTile + 1;  // ... of the panel's L rows
constexpr int kCholLdsDoubles = 2 * kCholKc * kCholLdB > kCholKc * kCholLdP ? 2 * kCholKc * kCholLdB
                                                                             : kCholKc * kCholLdP;
enum : uint32_t { kCholPotrf = 0, kCholTrsm = 1, kCholSyrk = 2, kCholGemm = 3 };

struct CholCtx {
    double *tiles;  // lower-triangular tile (j, i) at (j (j + 1) / 2 + i) T T, row-major inside
    int *fail;      // -1, or the first global column whose pivot was <= 0
    uint32_t *err;  // the launch's device error word
    int T;
};

__device__ __forceinline__ double *chol_tile(const CholCtx &c, uint32_t j, uint32_t i) {
    return c.tiles + ((size_t)j * (j + 1) / 2 + i) * (size_t)(c.T * c.T);
}

// every tile access: agent-scope (sc1) loads and write-through stores, the
// payload form run_dag_group hands between tasks without fences (kSc1Payload)
__device__ __forceinline__ double ldt(const double *p) { return ld_agent(p); }
__device__ __forceinline__ void stt(double *p, double v) { st_agent(p, v); }

__device__ __forceinline__ double *chol_lds() {
    __shared__ __attribute__((aligned(16))) double s[kCholLdsDoubles];
    return s;
}

// update_nondiagonal.cpp:11-17 / update_diagonal.cpp:10-16 (LOWER: iB >= jB
// only): A[iB][jB] += (0 - L2[jB][kB]) * L1[iB][kB], kB ascending. A thread
// owns a 4 x 4 register block (rows ty + 16 a, columns tx + 16 b of a 64 x 64
// block) and walks kB; the operand rows are staged 16 kB at a time.
template <bool LOWER>
__device__ void chol_update_exact(double *A, double *L1, double *L2, int T) {
    double *s1 = chol_lds(), *s2 = s1 + kCholKc * kCholLdB;
    const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int nb = (T + kCholBlk - 1) / kCholBlk;
    for (int bi = 0; bi < nb; ++bi)
        for (int bj = 0; bj < (LOWER ? bi + 1 : nb); ++bj) {
            const int r0 = bi * kCholBlk, c0 = bj * kCholBlk;
            double acc[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int iB = r0 + ty + 16 * a, jB = c0 + tx + 16 * b;
                    acc[a][b] = (iB < T && jB < T) ? ldt(&A[iB * T + jB]) : 0.0;
                }
            for (int k0 = 0; k0 < T; k0 += kCholKc) {
                const int kn = T - k0 < kCholKc ? T - k0 : kCholKc;
                __syncthreads();  // the previous chunk's readers are done
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int e = tid + kCholThreads * q, row = e >> 4, kk = e & 15;
                    const bool kin = k0 + kk < T;
                    s1[kk * kCholLdB + row] = (kin && r0 + row < T) ? ldt(&L1[(r0 + row) * T + k0 + kk]) : 0.0;
                    s2[kk * kCholLdB + row] = (kin && c0 + row < T) ? ldt(&L2[(c0 + row) * T + k0 + kk]) : 0.0;
                }
                __syncthreads();
                auto step = [&](int kk) {
                    double l1[4], t2[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) l1[a] = s1[kk * kCholLdB + ty + 16 * a];
#pragma unroll
                    for (int b = 0; b < 4; ++b) t2[b] = __dsub_rn(0.0, s2[kk * kCholLdB + tx + 16 * b]);
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[a][b] = __dadd_rn(acc[a][b], __dmul_rn(t2[b], l1[a]));
                };
                if (kn == kCholKc) {
#pragma unroll
                    for (int kk = 0; kk < kCholKc; ++kk) step(kk);
                } else {
                    for (int kk = 0; kk < kn; ++kk) step(kk);
                }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int iB = r0 + ty + 16 * a, jB = c0 + tx + 16 * b;
                    if (iB < T && jB < T && (!LOWER || iB >= jB)) stt(&A[iB * T + jB], acc[a][b]);
                }
        }
}

// lane `src` (wave-uniform) of a double to every lane: two v_readlane_b32, no
// LDS round trip (the potrf chain waits on it twice per column)
__device__ __forceinline__ double chol_bcast(double v, int src) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <bool POTRF>
__device__ void chol_panel(const CholCtx &c, double *A, double *Li, int T, int col0) {
    double *sLi = chol_lds();
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, row = tid;
    for (int p0 = 0; p0 < T; p0 += kCholKc) {
        const int w = T - p0 < kCholKc ? T - p0 : kCholKc;
        // the previous panel's LDS readers are done and (POTRF) its stores are
        // visible to the workgroup
        __syncthreads();
        const int nc = POTRF ? p0 : p0 + w;
        for (int e = tid; e < w * nc; e += kCholThreads) {
            const int r = e / nc, kB = e - r * nc;
            sLi[r * kCholLdP + kB] = ldt(&Li[(p0 + r) * T + kB]);
        }
        __syncthreads();
        const bool mine = row < T && (!POTRF || row >= p0);
        double x[kCholKc];
#pragma unroll
        for (int cc = 0; cc < kCholKc; ++cc) x[cc] = (mine && cc < w) ? ldt(&A[row * T + p0 + cc]) : 1.0;
        if (mine && p0) {
            // the row's finished columns 16 at a time, the next 16 in flight
            // while these are used (one memory latency per panel, not per kB)
            double cur[kCholKc], nxt[kCholKc];
#pragma unroll
            for (int q = 0; q < kCholKc; ++q) cur[q] = ldt(&A[row * T + q]);
            for (int k0 = 0; k0 < p0; k0 += kCholKc) {
                const bool more = k0 + kCholKc < p0;
#pragma unroll
                for (int q = 0; q < kCholKc; ++q) nxt[q] = more ? ldt(&A[row * T + k0 + kCholKc + q]) : 0.0;
#pragma unroll
                for (int q = 0; q < kCholKc; ++q)
#pragma unroll
                    for (int cc = 0; cc < kCholKc; ++cc)
                        x[cc] = __dsub_rn(x[cc], __dmul_rn(sLi[cc * kCholLdP + k0 + q], cur[q]));
#pragma unroll
                for (int q = 0; q < kCholKc; ++q) cur[q] = nxt[q];
            }
        }
        if (POTRF) {
            if (wave == (p0 >> 6)) {  // the wave that holds rows p0 .. p0 + 15
                const int b0 = p0 & 63, r = lane - b0;
#pragma unroll
                for (int kk = 0; kk < kCholKc; ++kk) {
                    if (kk < w) {
                        const double piv = chol_bcast(x[kk], b0 + kk);
                        if (piv <= 0 && lane == 0) {  // sequential_cholesky.cpp:11-12
                            int none = -1;
                            __hip_atomic_compare_exchange_strong(c.fail, &none, col0 + p0 + kk, __ATOMIC_RELAXED,
                                                                 __ATOMIC_RELAXED, HX_AGENT);
                            dev_error(c.err, kErrNotSpd);
                        }
                        const double d = __dsqrt_rn(piv);
                        x[kk] = r == kk ? d : __ddiv_rn(x[kk], d);
#pragma unroll
                        for (int cc = kk + 1; cc < kCholKc; ++cc) {
                            const double lc = chol_bcast(x[kk], b0 + cc);  // l[cc][kk]
                            x[cc] = __dsub_rn(x[cc], __dmul_rn(x[kk], lc));
                        }
                    }
                }
                // the lanes below the block (the wave's other rows) went through
                // the same steps, which are exactly their solve: l[iB][kk] =
                // a / l[kk][kk], then a[iB][cc] -= l[iB][kk] * l[cc][kk]
                if (r >= 0 && row < T) {
#pragma unroll
                    for (int cc = 0; cc < kCholKc; ++cc)
                        if (cc < w && (r >= w || cc <= r)) {
                            if (r < w) sLi[r * kCholLdP + p0 + cc] = x[cc];
                            stt(&A[row * T + p0 + cc], x[cc]);
                        }
                }
            }
            __syncthreads();  // the diagonal block is in LDS
        }
        if (mine && (!POTRF || (row >= p0 + w && wave != (p0 >> 6)))) {
#pragma unroll
            for (int kk = 0; kk < kCholKc; ++kk) {
                if (kk < w) {
                    x[kk] = __ddiv_rn(x[kk], sLi[kk * kCholLdP + p0 + kk]);
#pragma unroll
                    for (int cc = kk + 1; cc < kCholKc; ++cc)
                        x[cc] = __dsub_rn(x[cc], __dmul_rn(sLi[cc * kCholLdP + p0 + kk], x[kk]));
                }
            }
#pragma unroll
            for (int cc = 0; cc < kCholKc; ++cc)
                if (cc < w) stt(&A[row * T + p0 + cc], x[cc]);
        }
    }
}

struct CholKind : OnePromiseKind<CholCtx> {
    static constexpr bool kSc1Payload = true;  // tiles move by ld_agent / st_agent only (ldt / stt)
    __device__ static bool run_group(const Ctx &c, uint32_t, const uint32_t *pl, int) {
        const uint32_t kind = pl[0], k = pl[1], j = pl[2], i = pl[3];
        const int T = c.T;
        if (kind == kCholPotrf) {
            double *a = chol_tile(c, k, k);
            chol_panel<true>(c, a, a, T, (int)k * T);
        } else if (kind == kCholTrsm) {
            chol_panel<false>(c, chol_tile(c, j, k), chol_tile(c, k, k), T, 0);
        } else if (kind == kCholSyrk) {
            double *l = chol_tile(c, j, k);
            chol_update_exact<true>(chol_tile(c, j, j), l, l, T);
        } else {
            chol_update_exact<false>(chol_tile(c, j, i), chol_tile(c, j, k), chol_tile(c, i, k), T);
        }
        return true;
    }
};

__global__ __launch_bounds__(kCholThreads) void k_cholesky(CholCtx c, DagView v) {
    run_dag_group<CholKind>(c, v, nullptr);
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_cholesky(const double *a, int n, int tile, int mode, double *l,
                                  hclib_hip_cholesky_result_t *result) {
    // argument errors first, before the device is touched
    if (!a || !l) {
        set_error("hclib_hip_cholesky: a and l must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    if (n <= 0 || tile < 1) {
        set_error("hclib_hip_cholesky: matrix size %d and tile size %d must be positive", n, tile);
        return HCLIB_HIP_EINVAL;
    }
    if (n % tile != 0) {  // cholesky.cpp:26-29
        set_error("hclib_hip_cholesky: Incorrect tile size %d for the matrix of size %d", tile, n);
        return HCLIB_HIP_EINVAL;
    }
    if (tile > kCholMaxTile) {
        set_error("hclib_hip_cholesky: tile size %d is above the maximum of %d", tile, kCholMaxTile);
        return HCLIB_HIP_EINVAL;
    }
    if (mode != HCLIB_HIP_CHOL_EXACT) {
        set_error("hclib_hip_cholesky: unknown mode %d", mode);
        return HCLIB_HIP_EINVAL;
    }
    const uint64_t nt = (uint64_t)(n / tile);
    const uint64_t n_potrf = nt, n_trsm = nt * (nt - 1) / 2, n_gemm = nt * (nt - 1) * (nt - 2) / 6;
    const uint64_t ntasks = n_potrf + 2 * n_trsm + n_gemm;
    if (nt > 2048 || ntasks > (1ull << 26)) {
        set_error("hclib_hip_cholesky: %d / %d gives %llu tile tasks (at most 2^26): use a larger tile", n, tile,
                  (unsigned long long)ntasks);
        return HCLIB_HIP_EINVAL;
    }
    HX_TRY(ensure_device());
    Module &m = mod();

    // the graph, in the reference's program order (cholesky.cpp:80-124)
    const size_t T2 = (size_t)tile * tile, ntiles = (size_t)(nt * (nt + 1) / 2);
    auto tidx = [](uint64_t j, uint64_t i) { return (size_t)(j * (j + 1) / 2 + i); };
    VersionGraph g(ntiles);
    g.reserve(ntasks, 3);
    for (uint32_t k = 0; k < nt; ++k) {
        g.task(kCholPotrf, k, k, k, tidx(k, k), {tidx(k, k)});
        for (uint32_t j = k + 1; j < nt; ++j) g.task(kCholTrsm, k, j, k, tidx(j, k), {tidx(j, k), tidx(k, k)});
        for (uint32_t j = k + 1; j < nt; ++j) {
            for (uint32_t i = k + 1; i < j; ++i)
                g.task(kCholGemm, k, j, i, tidx(j, i), {tidx(j, i), tidx(i, k), tidx(j, k)});
            g.task(kCholSyrk, k, j, j, tidx(j, j), {tidx(j, j), tidx(j, k)});
        }
    }

    // tiles: the lower triangle of `a` (cholesky.cpp:63-74); the part of a
    // diagonal tile above the diagonal, which nothing reads, as zeros
    const size_t hdr = 256 / sizeof(double), ndoubles = hdr + ntiles * T2;
    std::vector<double> h(ndoubles, 0.0);
    int minus1 = -1;
    memcpy(h.data(), &minus1, sizeof(int));
    for (uint64_t j = 0; j < nt; ++j)
        for (uint64_t i = 0; i <= j; ++i) {
            double *t = h.data() + hdr + tidx(j, i) * T2;
            for (int r = 0; r < tile; ++r) {
                const double *src = a + (size_t)(j * tile + r) * n + i * tile;
                const int cols = i == j ? r + 1 : tile;
                memcpy(t + (size_t)r * tile, src, (size_t)cols * sizeof(double));
            }
        }
    const size_t bytes = ndoubles * sizeof(double);
    double *buf = nullptr;
    HX_TRY(arena_reserve(kArenaCholesky, bytes, "hclib_hip_cholesky", (void **)&buf));
    // (`h` outlives the copy: launch_dag_group synchronises the stream)
    HX_HIP(hipMemcpyAsync(buf, h.data(), bytes, hipMemcpyHostToDevice, m.stream));

    CholCtx c;
    c.tiles = buf + hdr;
    c.fail = (int *)buf;
    c.err = nullptr;
    c.T = tile;
    // one persistent workgroup per CU: the sc1 hand-off's measured form
    const int wgs = 1;
    hclib_hip_dag_stats_t st{};
    const int rc = launch_dag_group(g, wgs, (const void *)k_cholesky, kCholThreads, "hclib_hip_cholesky", &st,
                                    [&](int grid, const DagView &v) {
                                        c.err = v.err;
                                        hipLaunchKernelGGL(k_cholesky, dim3(grid), dim3(kCholThreads), 0, m.stream, c, v);
                                    });
    int fail_col = -1;
    if (rc == HCLIB_HIP_EDEVICE) (void)hipMemcpy(&fail_col, c.fail, sizeof(int), hipMemcpyDeviceToHost);
    if (result) {
        result->tasks = st.tasks;
        result->puts = st.puts;
        result->releases = st.releases;
        result->potrf = n_potrf;
        result->trsm = n_trsm;
        result->syrk = n_trsm;
        result->gemm = n_gemm;
        result->kernel_ms = st.kernel_ms;
        result->gflops = st.kernel_ms > 0 ? ((double)n * n * n / 3.0) / (st.kernel_ms * 1e6) : 0.0;
        result->fail_col = fail_col;
    }
    if (fail_col >= 0) {  // sequential_cholesky.cpp:11-12
        set_error("hclib_hip_cholesky: Not a symmetric positive definite (SPD) matrix (pivot <= 0 at column %d)",
                  fail_col);
        return HCLIB_HIP_EDEVICE;
    }
    if (rc) return rc;
    HX_HIP(hipMemcpy(h.data(), buf, bytes, hipMemcpyDeviceToHost));
    // the factor's lower triangle; the strict upper triangle as +0.0
    for (uint64_t j = 0; j < nt; ++j)
        for (int r = 0; r < tile; ++r) {
            double *dst = l + (size_t)(j * tile + r) * n;
            for (uint64_t i = 0; i <= j; ++i) {
                const double *t = h.data() + hdr + tidx(j, i) * T2 + (size_t)r * tile;
                const int cols = i == j ? r + 1 : tile;
                memcpy(dst + i * tile, t, (size_t)cols * sizeof(double));
            }
            const size_t diag = (size_t)(j * tile + r);
            for (size_t cc = diag + 1; cc < (size_t)n; ++cc) dst[cc] = 0.0;
        }
    return HCLIB_HIP_OK;
}
