// jacobi.hip — Kastors jacobi (test/performance-regression/full-apps/
// kastors-1.1/jacobi: src/jacobi-seq.c the rule, src/jacobi-block-task.c the
// blocked sweep(), src/poisson.c the driver) as one launch of the generic
// device promise DAG (include/hclib_hip/hx_dag.h, run_dag_group).
//
// The reference's sweep() runs, per iteration, a copy phase and a compute phase
// of one task per block, each closed by hclib_end_finish (jacobi-block-task.c
// :57-108). Here a task is one block of one superstep, it awaits its
// neighbours of the superstep before and nothing else, and a superstep is up to
// `fuse` iterations (hx_jacobi_plan.h has the graph and the argument that the
// same awaits order the overwrites of the two ping-pong buffers):
//
//   task (s, bx, by), t = t_s sweeps     awaits                     puts
//   reads  buffer s & 1, the block and   (s - 1, b') for b' = b     (s, b)
//          a halo t wide, clipped to     and its 4 (fuse = 1) or
//          the grid; f a halo t - 1      8 in-grid neighbours
//   writes buffer (s + 1) & 1, the block
//
// The body. One workgroup of four waves per task. It loads the clipped region
// of u and of f into LDS, runs t sweeps that ping-pong between two LDS images
// with a barrier between them, each sweep one ring narrower than the one
// before (sweep k of t computes the halo t - k, which needs the halo
// t - k + 1 of sweep k - 1), and the last sweep, which is the block itself,
// goes from registers to memory. A grid-boundary cell is f in every sweep.
// A cell's value at iteration k is a fixed expression of four values at
// iteration k - 1, whichever task evaluates it, so the recomputed overlap has
// the owner's bits and the result depends on neither block nor fuse.
//
// Arithmetic, jacobi-seq.c:24-26, every operation rounded on its own:
//   0.25 * ((((u[i-1][j] + u[i][j+1]) + u[i][j-1]) + u[i+1][j]) + (f[i][j] * dx) * dy)
// as __dadd_rn / __dmul_rn (no v_fma_f64), 0.25 a multiply as in the reference.
//
// Memory protocol. u is read and written by other tasks on other CUs during the
// launch: every access is an agent-scope (sc1) load or write-through store, the
// payload form run_dag_group hands from task to task behind a drain and a
// barrier (kSc1Payload, as cholesky.hip). f is uploaded before the launch and
// only read: plain loads. Lanes run along j, the contiguous axis; the block is
// stored 16 bytes per lane where its width is even.
//
// LDS layout: hx_jacobi_plan.h (lanes_j, pitch). The kernel comes in three
// forms that differ only in the static LDS they declare, 39, 79 and 159 KiB,
// so that small regions leave room for 4 or 2 workgroups per CU.
#include <string.h>

#include <vector>

#include "hx_client.h"
#include "hx_jacobi_plan.h"

namespace hx {
namespace {

constexpr int kJacThreads = 256;
constexpr int kJacCells = 4;  // cells a thread computes at a time in a sweep
// static LDS (doubles) of the three kernel forms and the workgroups per CU each leaves room for
constexpr int kJacLds4 = 39 * 1024 / 8, kJacLds2 = 79 * 1024 / 8, kJacLds1 = kJacobiLdsDoubles;

struct JacobiCtx {
    double *u[2];     // the ping-pong grids
    const double *f;
    uint32_t *err;    // the launch's device error word
    double dx, dy;
    int nx, ny, block, pitch, lanes_shift;
};

__device__ __forceinline__ int jmax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int jmin(int a, int b) { return a < b ? a : b; }

template <int LDS>
__device__ __forceinline__ double *jacobi_lds() {
    __shared__ __attribute__((aligned(16))) double s[LDS];
    return s;
}

template <int LDS, int STAGE>
__device__ bool jacobi_task(const JacobiCtx &c, const uint32_t *pl) {
    const int s = (int)pl[0], bx = (int)pl[1], by = (int)pl[2], t = (int)pl[3];
    const int B = c.block, nx = c.nx, ny = c.ny, P = c.pitch;
    // (workgroup-uniform) the block lies in the grid and the region's three images in this form's LDS
    if (t < 1 || t > B || (long long)(bx + 1) * B > nx || (long long)(by + 1) * B > ny || B + 2 * t > P ||
        3ll * (B + 2 * t) * P > LDS) {
        if (threadIdx.x == 0) dev_error(c.err, kErrBadTask);
        return false;
    }
    const int i0 = bx * B, j0 = by * B;
    // the region: the block and a halo t wide, clipped to the grid
    const int rlo = jmax(i0 - t, 0), rhi = jmin(i0 + B + t, nx), clo = jmax(j0 - t, 0), chi = jmin(j0 + B + t, ny);
    const int h = rhi - rlo, w = chi - clo;
    // f: the cells some sweep computes, a halo t - 1
    const int frlo = jmax(i0 - t + 1, 0), frhi = jmin(i0 + B + t - 1, nx);
    const int fclo = jmax(j0 - t + 1, 0), fchi = jmin(j0 + B + t - 1, ny);
    const double *src = c.u[s & 1];
    double *dst = c.u[(s + 1) & 1];
    double *cur = jacobi_lds<LDS>(), *nxt = cur + h * P, *fim = nxt + h * P;

    const int tid = (int)threadIdx.x, L = 1 << c.lanes_shift, tx = tid & (L - 1), ty = tid >> c.lanes_shift;
    const int TY = kJacThreads >> c.lanes_shift;

    // A thread walks its cells of a window [r_lo, r_hi) x [c_lo, c_hi), rows ty, ty + TY, ... and in each its
    // columns tx, tx + L, ...: `next` steps (r, cc) to the thread's next cell, past the window (r >= r_hi) at the
    // end. Every phase below takes a batch of cells at a time, all loads of the batch (memory, then LDS) ahead of
    // its stores: one wave per SIMD has nothing else to hide a load's latency behind
    auto first = [&](int &r, int &cc, int r_lo, int r_hi, int c_lo, int c_hi) {
        cc = c_lo + tx;
        r = cc < c_hi ? r_lo + ty : r_hi;
    };
    auto next = [&](int &r, int &cc, int c_lo, int c_hi) {
        cc += L;
        if (cc >= c_hi) {
            cc = c_lo + tx;
            r += TY;
        }
    };

    // stage u (sc1) and f: STAGE cells in flight per thread
    {
        int r, cc;
        first(r, cc, 0, h, 0, w);
        while (r < h) {
            double uu[STAGE], ff[STAGE];
            int at[STAGE];
#pragma unroll
            for (int k = 0; k < STAGE; ++k) {
                const bool ok = r < h;
                const int gi = rlo + r, gj = clo + cc;
                const size_t g = (size_t)gi * ny + gj;
                at[k] = ok ? r * P + cc : -1;
                uu[k] = ok ? ld_agent(&src[g]) : 0.0;
                ff[k] = (ok && gi >= frlo && gi < frhi && gj >= fclo && gj < fchi) ? c.f[g] : 0.0;
                next(r, cc, 0, w);
            }
#pragma unroll
            for (int k = 0; k < STAGE; ++k)
                if (at[k] >= 0) {
                    cur[at[k]] = uu[k];
                    fim[at[k]] = ff[k];
                }
        }
    }
    __syncthreads();

    const double dx = c.dx, dy = c.dy;
    // jacobi-seq.c:21-27 for the cell at LDS index `at`, grid (gi, gj)
    auto cell = [&](const double *u, int at, int gi, int gj) {
        const double fv = fim[at];
        if (gi == 0 || gj == 0 || gi == nx - 1 || gj == ny - 1) return fv;
        const double sum = __dadd_rn(__dadd_rn(__dadd_rn(u[at - P], u[at + 1]), u[at - 1]), u[at + P]);
        return __dmul_rn(0.25, __dadd_rn(sum, __dmul_rn(__dmul_rn(fv, dx), dy)));
    };

    // sweeps 1 .. t - 1: the halo t - k, from one LDS image into the other
    for (int k = 1; k < t; ++k) {
        const int hk = t - k;
        const int r_lo = jmax(i0 - hk, 0) - rlo, r_hi = jmin(i0 + B + hk, nx) - rlo;
        const int c_lo = jmax(j0 - hk, 0) - clo, c_hi = jmin(j0 + B + hk, ny) - clo;
        int r, cc;
        first(r, cc, r_lo, r_hi, c_lo, c_hi);
        while (r < r_hi) {
            double v[kJacCells];
            int at[kJacCells];
#pragma unroll
            for (int q = 0; q < kJacCells; ++q) {
                const bool ok = r < r_hi;
                at[q] = ok ? r * P + cc : -1;
                v[q] = ok ? cell(cur, r * P + cc, rlo + r, clo + cc) : 0.0;
                next(r, cc, c_lo, c_hi);
            }
#pragma unroll
            for (int q = 0; q < kJacCells; ++q)
                if (at[q] >= 0) nxt[at[q]] = v[q];
        }
        __syncthreads();
        double *sw = cur;
        cur = nxt;
        nxt = sw;
    }

    // sweep t: the block, from registers to memory (write-through)
    const int r_lo = i0 - rlo, c_lo = j0 - clo;
    if ((B & 1) == 0) {
        // two cells a lane, one 16-byte store: B even makes ny and j0 even, so (gi ny + gj) is even.
        // The thread's window is the block's pairs: column index pc, cell column c_lo + 2 pc
        int r, pc;
        first(r, pc, r_lo, r_lo + B, 0, B / 2);
        while (r < r_lo + B) {
            double v0[kJacCells], v1[kJacCells];
            size_t g[kJacCells];
            bool ok[kJacCells];
#pragma unroll
            for (int q = 0; q < kJacCells; ++q) {
                ok[q] = r < r_lo + B;
                const int cc = c_lo + 2 * pc, gi = rlo + r, gj = clo + cc, at = r * P + cc;
                g[q] = (size_t)gi * ny + gj;
                v0[q] = ok[q] ? cell(cur, at, gi, gj) : 0.0;
                v1[q] = ok[q] ? cell(cur, at + 1, gi, gj + 1) : 0.0;
                next(r, pc, 0, B / 2);
            }
#pragma unroll
            for (int q = 0; q < kJacCells; ++q)
                if (ok[q])
                    st_sc1_x4(&dst[g[q]], make_uint4((uint32_t)__double2loint(v0[q]), (uint32_t)__double2hiint(v0[q]),
                                                     (uint32_t)__double2loint(v1[q]), (uint32_t)__double2hiint(v1[q])));
        }
    } else {
        int r, cc;
        first(r, cc, r_lo, r_lo + B, c_lo, c_lo + B);
        while (r < r_lo + B) {
            const int gi = rlo + r, gj = clo + cc;
            st_agent(&dst[(size_t)gi * ny + gj], cell(cur, r * P + cc, gi, gj));
            next(r, cc, c_lo, c_lo + B);
        }
    }
    // (run_dag_group drains the stores and runs a barrier before the next task touches the LDS)
    return true;
}

template <int LDS>
struct JacobiKind : OnePromiseKind<JacobiCtx> {
    static constexpr bool kSc1Payload = true;  // the grids move by ld_agent / st_agent / st_sc1_x4 only
    __device__ static bool run_group(const JacobiCtx &c, uint32_t, const uint32_t *pl, int) {
        // the form with a CU to itself stages 16 cells a thread at a time, the others 8 (registers: four waves a SIMD)
        return jacobi_task<LDS, (LDS > kJacLds2 ? 16 : 8)>(c, pl);
    }
};

template <int LDS>
__global__ __launch_bounds__(kJacThreads) void k_jacobi(JacobiCtx c, DagView v) {
    run_dag_group<JacobiKind<LDS>>(c, v, nullptr);
}

int jacobi_args(const char *who, bool ptrs_ok, int nx, int ny, int &block, int niter, int &fuse, JacobiPlan &p) {
    if (!ptrs_ok) {
        set_error("%s: the arrays must not be NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    std::string err;
    if (jacobi_plan(nx, ny, block, niter, fuse, p, err)) {
        set_error("%s: %s", who, err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    return HCLIB_HIP_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_jacobi_rhs(int nx, int ny, double *f, double *unew0) {
    if (nx < 3 || ny < 3) {
        set_error("hclib_hip_jacobi_rhs: the grid must be at least 3 x 3");
        return HCLIB_HIP_EINVAL;
    }
    jacobi_rhs_fill(nx, ny, f, unew0);
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_jacobi_bounds(int nx, int ny, int block, int niter, int fuse, uint64_t out[4]) {
    JacobiPlan p;
    HX_TRY(jacobi_args("hclib_hip_jacobi_bounds", out != nullptr, nx, ny, block, niter, fuse, p));
    out[0] = p.tasks;
    out[1] = p.awaits;
    out[2] = p.supersteps;
    out[3] = p.bytes_moved;
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_jacobi(const double *f, const double *unew0, int nx, int ny, double dx, double dy, int block,
                                int niter, int fuse, double *unew, hclib_hip_jacobi_result_t *result) {
    // argument errors first, before the device is touched
    JacobiPlan p;
    HX_TRY(jacobi_args("hclib_hip_jacobi", f && unew0 && unew, nx, ny, block, niter, fuse, p));
    HX_TRY(ensure_device());
    Module &m = mod();
    // the kernel form whose LDS holds the region, and the workgroups per CU it leaves room for
    const int max_wgs = p.lds_doubles <= kJacLds4 ? 4 : p.lds_doubles <= kJacLds2 ? 2 : 1;
    // (HCLIB_HIP_JACOBI_WGS_PER_CU: for measurements)
    int wgs = env_int("HCLIB_HIP_JACOBI_WGS_PER_CU", max_wgs);
    wgs = wgs < 1 ? 1 : (wgs > max_wgs ? max_wgs : wgs);
    if (result) {
        memset(result, 0, sizeof(*result));
        result->supersteps = p.supersteps;
        result->bytes_moved = p.bytes_moved;
        result->block = block;
        result->fuse = fuse;
        result->wgs_per_cu = wgs;
    }
    const size_t cells = (size_t)nx * ny, gbytes = cells * sizeof(double);
    if (niter == 0) {  // nothing to launch
        memmove(unew, unew0, gbytes);
        return HCLIB_HIP_OK;
    }

    VersionGraph g;
    jacobi_graph(p, g);

    // [f][grid 0][grid 1], each on a 256-byte line
    const size_t stride = (gbytes + 255) & ~(size_t)255;
    char *d = nullptr;
    if (const int rc = arena_reserve(kArenaJacobi, 3 * stride, "hclib_hip_jacobi", (void **)&d)) {
        set_error("hclib_hip_jacobi: hipMalloc(%zu) failed (%d x %d: f and two grids of 8 bytes a cell)", 3 * stride, nx,
                  ny);
        return rc;
    }
    // (`f` and `unew0` outlive the copies: launch_dag_group synchronises the stream)
    HX_HIP(hipMemcpyAsync(d, f, gbytes, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(d + stride, unew0, gbytes, hipMemcpyHostToDevice, m.stream));

    JacobiCtx c;
    c.f = (const double *)d;
    c.u[0] = (double *)(d + stride);
    c.u[1] = (double *)(d + 2 * stride);
    c.err = nullptr;
    c.dx = dx;
    c.dy = dy;
    c.nx = nx;
    c.ny = ny;
    c.block = block;
    c.pitch = p.pitch;
    c.lanes_shift = p.lanes_j == 16 ? 4 : p.lanes_j == 32 ? 5 : 6;
    using Kern = void (*)(JacobiCtx, DagView);
    const Kern kern = max_wgs == 4 ? k_jacobi<kJacLds4> : max_wgs == 2 ? k_jacobi<kJacLds2> : k_jacobi<kJacLds1>;
    hclib_hip_dag_stats_t st{};
    const int rc = launch_dag_group(g, wgs, (const void *)kern, kJacThreads, "hclib_hip_jacobi", &st,
                                    [&](int grid, const DagView &v) {
                                        c.err = v.err;
                                        hipLaunchKernelGGL(kern, dim3(grid), dim3(kJacThreads), 0, m.stream, c, v);
                                    });
    if (result) {
        result->tasks = st.tasks;
        result->puts = st.puts;
        result->releases = st.releases;
        result->kernel_ms = st.kernel_ms;
        if (st.kernel_ms > 0) {
            result->gbytes_per_s = (double)p.bytes_moved / (st.kernel_ms * 1e6);
            result->gcells_per_s = (double)cells * niter / (st.kernel_ms * 1e6);
        }
    }
    if (rc) return rc;
    HX_HIP(hipMemcpy(unew, d + (p.supersteps & 1 ? 2 * stride : stride), gbytes, hipMemcpyDeviceToHost));
    return HCLIB_HIP_OK;
}
