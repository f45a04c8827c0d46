// srad.hip — Rodinia SRAD, speckle-reducing anisotropic diffusion
// (test/performance-regression/full-apps/rodinia/srad: srad.cpp the HClib port,
// srad.ref.cpp the arithmetic) as one launch of the generic device promise DAG
// (include/hclib_hip/hx_dag.h, run_dag_group).
//
// The port runs, per iteration, the float sums over the region of interest on
// the host thread (srad.ref.cpp:131-141), then two hclib_forasync_future sweeps
// with a hclib_future_wait after each (:145-176, :182-207). Here an iteration
// is one reduce task and one task per block, and nothing joins (hx_srad_plan.h
// has the graph and the argument that these awaits also order the overwrites
// of the two ping-pong grids):
//
//   task            reads                         awaits                puts
//   R(it)           grid it & 1, the ROI          T(it - 1, b), b in    R(it), datum
//                                                 the ROI's blocks      q0sqr(it)
//   T(it, b)        grid it & 1: the block, one   R(it); T(it - 1, b')  T(it, b)
//                   cell N and W, two S and E,    for b' = b and its 8
//                   clamped at the grid's edge    in-grid neighbours
//                   writes grid (it + 1) & 1, the block
//
// R. One wave (the workgroup's last, which also publishes the promise's
// datum). The two sums are in the reference's order, row-major over the ROI,
// one chain of __fadd_rn each: a float sum cannot be re-associated if the bits
// are to match. Lanes load 64 values at once and square them; the chains walk
// the 64 by v_readlane, interleaved, with the next 64 loads in flight. Its
// length is what it is: size_R dependent adds. Then meanROI, varROI and q0sqr,
// which becomes the promise's datum.
//
// T. One workgroup of four waves. It takes q0sqr(it) from R(it)'s datum
// (hclib_future_get), loads the (block + 3)^2 region of J into LDS with the
// row and column indices clamped to the grid (the reference's iN / iS / jW /
// jE tables: at the edge dN = J - J = +0.0), computes c over the block plus
// one row south and one column east into a second LDS image, and after a
// barrier the divergence and the new J, which re-derives the four derivatives
// from the J image; c[iS] of the grid's last row is the row's own c, likewise
// c[jE] of the last column. dN..dE and c never reach memory. The recomputed
// halo of c is the same pure function of five J cells and q0sqr as its owner's,
// so it has its owner's bits and the result depends on neither block nor form.
// At block 64 the images are 67^2 + 65^2 floats, 34 KiB: four workgroups a CU.
//
// Arithmetic: every operation rounded on its own, __f*_rn / __d*_rn and
// explicit conversions, in the reference's types (DESIGN.md §23 has the table):
// dN..dE, G2, L, qsqr, the second den and D float; num, the first den, c and
// the update computed in double from floats and rounded to float once.
// Saturation is the reference's `if (c < 0) c = 0; else if (c > 1) c = 1;`:
// a NaN and a -0.0 pass through.
//
// Memory protocol. The grids are written and read by different workgroups
// during the launch: every access is an agent-scope (sc1) load or write-through
// store, 16 bytes a lane (kSc1Payload, as jacobi.hip).
//
// The phases form runs the same two bodies as one reduce kernel (one wave) and
// one sweep kernel (a workgroup per block) per iteration, stream-ordered: the
// form with joins, for comparison. Same bits.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hx_client.h"
#include "hx_srad_plan.h"

namespace hx {
namespace {

constexpr int kSradThreads = 256;
constexpr int kSradStage = 6;  // cells a thread has in flight while it stages J (67^2 cells: three rounds)

struct SradCtx {
    float *J[2];                      // the ping-pong grids
    const unsigned long long *datum;  // q0sqr(it) is the low word of datum[it * dstride]
    unsigned long long *qout;         // phases form: where the reduce kernel leaves q0sqr(it)
    uint32_t *err;                    // the launch's device error word (dag form)
    double qlam;                      // 0.25 * (double)lambda
    int rows, cols, block, nbx, nby, niter, r1, r2, c1, c2;
    uint32_t dstride;                 // dag: nb + 1, the tasks of an iteration; phases: 1
};

__device__ __forceinline__ float fa(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float fs(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float fm(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float fdv(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float lane_of(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__device__ __forceinline__ float *srad_lds() {
    __shared__ __attribute__((aligned(16))) float s[srad_lds_floats(kSradMaxBlock)];
    return s;
}
// the bits of the q0sqr a workgroup's R task made, from its body to its put
__device__ __forceinline__ uint32_t *srad_q_lds() {
    __shared__ uint32_t q;
    return &q;
}

// R(it), one wave: srad.ref.cpp:131-141
__device__ __forceinline__ float srad_reduce(const SradCtx &c, int it) {
    const float *src = c.J[it & 1];
    const int w = c.c2 - c.c1 + 1, n = w * (c.r2 - c.r1 + 1), lane = lane_id();
    auto load = [&](int n0) {
        const int k = n0 + lane;
        float v = 0.0f;
        if (k < n && k >= 0) {
            const int i = k / w, j = k - i * w;
            v = ld_agent(&src[(size_t)(c.r1 + i) * c.cols + (c.c1 + j)]);
        }
        return v;
    };
    float sum = 0.0f, sum2 = 0.0f;
    float cur = load(0);
    for (int n0 = 0; n0 < n; n0 += 64) {
        const float nxt = n - n0 > 64 ? load(n0 + 64) : 0.0f;  // in flight under the chains
        const float sq = fm(cur, cur);
        const int cnt = n - n0 < 64 ? n - n0 : 64;
        if (cnt == 64) {
#pragma unroll
            for (int l = 0; l < 64; ++l) {
                sum = fa(sum, lane_of(cur, l));
                sum2 = fa(sum2, lane_of(sq, l));
            }
        } else {
            for (int l = 0; l < cnt; ++l) {
                sum = fa(sum, lane_of(cur, l));
                sum2 = fa(sum2, lane_of(sq, l));
            }
        }
        cur = nxt;
    }
    const float size_r = (float)n;
    const float mean = fdv(sum, size_r);
    const float var = fs(fdv(sum2, size_r), fm(mean, mean));
    return fdv(var, fm(mean, mean));
}

// T(it, (bi, bj)) at block B
template <int B>
__device__ __forceinline__ void srad_block(const SradCtx &c, int it, int bi, int bj) {
    constexpr int P = B + 3, Q = B + 1;
    float *jim = srad_lds(), *cim = jim + P * P;
    const float *src = c.J[it & 1];
    float *dst = c.J[(it + 1) & 1];
    const int rows = c.rows, cols = c.cols, i0 = bi * B, j0 = bj * B, tid = (int)threadIdx.x;
    // hclib_future_get of R(it): its datum is q0sqr
    const float q0 = __uint_as_float((uint32_t)ld_agent(&c.datum[(size_t)it * c.dstride]));

    // stage J (sc1): LDS (r, cc) is grid (i0 - 1 + r, j0 - 1 + cc), both clamped to the grid
    for (int k0 = tid; k0 < P * P; k0 += kSradThreads * kSradStage) {
        float v[kSradStage];
#pragma unroll
        for (int k = 0; k < kSradStage; ++k) {
            const int idx = k0 + k * kSradThreads;
            v[k] = 0.0f;
            if (idx < P * P) {
                const int r = idx / P, cc = idx - r * P;
                int gi = i0 - 1 + r, gj = j0 - 1 + cc;
                gi = gi < 0 ? 0 : (gi > rows - 1 ? rows - 1 : gi);
                gj = gj < 0 ? 0 : (gj > cols - 1 ? cols - 1 : gj);
                v[k] = ld_agent(&src[(size_t)gi * cols + gj]);
            }
        }
#pragma unroll
        for (int k = 0; k < kSradStage; ++k) {
            const int idx = k0 + k * kSradThreads;
            if (idx < P * P) jim[idx] = v[k];
        }
    }
    __syncthreads();

    // sweep 1 (:145-176) over the block, one row south and one column east
    const float q0den = fm(q0, fa(1.0f, q0));
    for (int idx = tid; idx < Q * Q; idx += kSradThreads) {
        const int r = idx / Q, cc = idx - r * Q, a = (r + 1) * P + (cc + 1);
        const float Jc = jim[a];
        const float dN = fs(jim[a - P], Jc), dS = fs(jim[a + P], Jc), dW = fs(jim[a - 1], Jc), dE = fs(jim[a + 1], Jc);
        const float G2 = fdv(fa(fa(fa(fm(dN, dN), fm(dS, dS)), fm(dW, dW)), fm(dE, dE)), fm(Jc, Jc));
        const float L = fdv(fa(fa(fa(dN, dS), dW), dE), Jc);
        const float num = __double2float_rn(__dsub_rn(__dmul_rn(0.5, (double)G2), __dmul_rn(1.0 / 16.0, (double)fm(L, L))));
        float den = __double2float_rn(__dadd_rn(1.0, __dmul_rn(.25, (double)L)));
        const float qsqr = fdv(num, fm(den, den));
        den = fdv(fs(qsqr, q0), q0den);
        float cv = __double2float_rn(__ddiv_rn(1.0, __dadd_rn(1.0, (double)den)));
        if (cv < 0) {
            cv = 0;
        } else if (cv > 1) {
            cv = 1;
        }
        cim[idx] = cv;
    }
    __syncthreads();

    // sweep 2 (:182-207): four cells a lane, one 16-byte write-through store (cols and j0 are multiples of 16)
    for (int idx = tid; idx < B * (B / 4); idx += kSradThreads) {
        const int r = idx / (B / 4), c4 = (idx - r * (B / 4)) * 4, gi = i0 + r;
        const int rs = gi == rows - 1 ? r : r + 1;  // iS
        uint32_t out[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cc = c4 + e, a = (r + 1) * P + (cc + 1);
            const int ce = j0 + cc == cols - 1 ? cc : cc + 1;  // jE
            const float Jc = jim[a];
            const float dN = fs(jim[a - P], Jc), dS = fs(jim[a + P], Jc), dW = fs(jim[a - 1], Jc), dE = fs(jim[a + 1], Jc);
            const float cN = cim[r * Q + cc], cS = cim[rs * Q + cc], cW = cN, cE = cim[r * Q + ce];
            const float D = fa(fa(fa(fm(cN, dN), fm(cS, dS)), fm(cW, dW)), fm(cE, dE));
            out[e] = __float_as_uint(__double2float_rn(__dadd_rn((double)Jc, __dmul_rn(c.qlam, (double)D))));
        }
        st_sc1_x4(&dst[(size_t)gi * cols + (j0 + c4)], make_uint4(out[0], out[1], out[2], out[3]));
    }
    // (the caller drains the stores; a barrier follows before the LDS is touched again)
}

// T(it, (bi, bj)): false (workgroup-uniform) where the task lies outside the plan
__device__ __forceinline__ bool srad_sweep(const SradCtx &c, int it, int bi, int bj) {
    if (it < 0 || it >= c.niter || bi < 0 || bi >= c.nbx || bj < 0 || bj >= c.nby) return false;
    if (c.block == 64) srad_block<64>(c, it, bi, bj);
    else if (c.block == 32) srad_block<32>(c, it, bi, bj);
    else if (c.block == 16) srad_block<16>(c, it, bi, bj);
    else return false;
    return true;
}

struct SradKind : OnePromiseKind<SradCtx> {
    static constexpr bool kSc1Payload = true;  // the grids move by ld_agent / st_sc1_x4 only
    // R(it) is task it * dstride: its promise carries q0sqr; a T's carries nothing
    __device__ static void datums(const SradCtx &c, uint32_t t, unsigned long long (&d)[1]) {
        d[0] = t % c.dstride == 0 ? (unsigned long long)*srad_q_lds() : 0ull;
    }
    __device__ static bool run_group(const SradCtx &c, uint32_t, const uint32_t *pl, int wave) {
        const int it = (int)pl[1];
        bool ok;
        if (pl[0] == 0u) {
            ok = it >= 0 && it < c.niter;
            // the last wave: the one that publishes the datum behind its body
            if (ok && wave == (int)(blockDim.x >> 6) - 1) *srad_q_lds() = __float_as_uint(srad_reduce(c, it));
        } else {
            ok = srad_sweep(c, it, (int)pl[2], (int)pl[3]);
        }
        if (!ok && threadIdx.x == 0) dev_error(c.err, kErrBadTask);
        return ok;
    }
};

__global__ __launch_bounds__(kSradThreads) void k_srad(SradCtx c, DagView v) { run_dag_group<SradKind>(c, v, nullptr); }

// the phases form: iteration `it`, the reduce (one wave) and the sweep (a workgroup per block)
__global__ __launch_bounds__(64) void k_srad_reduce(SradCtx c, int it) {
    const float q = srad_reduce(c, it);
    if (threadIdx.x == 0) st_agent(&c.qout[it], (unsigned long long)__float_as_uint(q));
}
__global__ __launch_bounds__(kSradThreads) void k_srad_sweep(SradCtx c, int it) {
    (void)srad_sweep(c, it, (int)blockIdx.x / c.nby, (int)blockIdx.x % c.nby);
}

int srad_args(const char *who, bool ptrs_ok, int rows, int cols, int r1, int r2, int c1, int c2, int niter, int &block,
              int form, SradPlan &p) {
    if (!ptrs_ok) {
        set_error("%s: the arrays must not be NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    std::string err;
    if (srad_plan(rows, cols, r1, r2, c1, c2, niter, block, form, p, err)) {
        set_error("%s: %s", who, err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    return HCLIB_HIP_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_srad_image(int rows, int cols, float *j0) {
    if (!j0 || rows < 1 || cols < 1 || (int64_t)rows * cols > INT32_MAX) {
        set_error("hclib_hip_srad_image: j0 must not be NULL and rows x cols must lie in [1, 2^31)");
        return HCLIB_HIP_EINVAL;
    }
    // random_matrix (:245-262), then `J[k] = (float)exp(I[k])` (:122-124): C++ on a float, so expf
    srand(7);
    for (int i = 0; i < rows; i++)
        for (int j = 0; j < cols; j++) j0[(size_t)i * cols + j] = rand() / (float)RAND_MAX;
    for (size_t k = 0; k < (size_t)rows * cols; k++) j0[k] = expf(j0[k]);
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_srad_bounds(int rows, int cols, int r1, int r2, int c1, int c2, int niter, int block,
                                     uint64_t out[6]) {
    SradPlan p;
    HX_TRY(srad_args("hclib_hip_srad_bounds", out != nullptr, rows, cols, r1, r2, c1, c2, niter, block, HCLIB_HIP_SRAD_DAG,
                     p));
    out[0] = p.tasks;
    out[1] = p.awaits;
    out[2] = (uint64_t)p.block;
    out[3] = p.max_waiters;
    out[4] = p.arena_bytes;
    out[5] = p.bytes_moved;
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_srad(const float *j0, int rows, int cols, int r1, int r2, int c1, int c2, float lambda, int niter,
                              int block, int form, float *j, float *q0sqr, hclib_hip_srad_result_t *result) {
    // argument errors first, before the device is touched
    SradPlan p;
    HX_TRY(srad_args("hclib_hip_srad", j0 && j, rows, cols, r1, r2, c1, c2, niter, block, form, p));
    if (result) {
        memset(result, 0, sizeof(*result));
        result->awaits = p.awaits;
        result->iterations = (uint64_t)niter;
        result->bytes_moved = p.bytes_moved;
        result->block = block;
        result->form = form;
    }
    HX_TRY(ensure_device());
    Module &m = mod();
    const size_t gbytes = (size_t)rows * cols * sizeof(float);
    if (niter == 0) {  // nothing to launch
        memmove(j, j0, gbytes);
        return HCLIB_HIP_OK;
    }

    // [grid 0][grid 1][the phases form's scalars], each on a 256-byte line
    const size_t stride = srad_up256(gbytes), qbytes = srad_up256((size_t)niter * 8);
    char *d = nullptr;
    if (const int rc = arena_reserve(kArenaSrad, 2 * stride + qbytes, "hclib_hip_srad", (void **)&d)) {
        set_error("hclib_hip_srad: hipMalloc(%zu) failed (%d x %d: two grids of 4 bytes a cell)", 2 * stride + qbytes, rows,
                  cols);
        return rc;
    }
    // (`j0` outlives the copy: every path below synchronises the stream)
    HX_HIP(hipMemcpyAsync(d, j0, gbytes, hipMemcpyHostToDevice, m.stream));

    SradCtx c;
    c.J[0] = (float *)d;
    c.J[1] = (float *)(d + stride);
    c.qout = (unsigned long long *)(d + 2 * stride);
    c.datum = c.qout;
    c.err = nullptr;
    c.qlam = 0.25 * (double)lambda;
    c.rows = rows, c.cols = cols, c.block = block, c.nbx = p.nbx, c.nby = p.nby, c.niter = niter;
    c.r1 = r1, c.r2 = r2, c.c1 = c1, c.c2 = c2;
    c.dstride = 1;

    hclib_hip_dag_stats_t st{};
    std::vector<uint64_t> datum;
    int rc = HCLIB_HIP_OK;
    if (form == HCLIB_HIP_SRAD_DAG) {
        VersionGraph g;
        srad_graph(p, g);
        if (q0sqr) datum.resize(g.ntasks());
        c.dstride = (uint32_t)p.nb + 1;
        // workgroups per CU: the LDS leaves room for 4 (HCLIB_HIP_SRAD_WGS_PER_CU: for measurements)
        int wgs = env_int("HCLIB_HIP_SRAD_WGS_PER_CU", 4);
        wgs = wgs < 1 ? 1 : (wgs > 4 ? 4 : wgs);
        rc = launch_dag_group(
            g, wgs, (const void *)k_srad, kSradThreads, "hclib_hip_srad", &st,
            [&](int grid, const DagView &v) {
                c.err = v.err;
                c.datum = v.datum;
                hipLaunchKernelGGL(k_srad, dim3(grid), dim3(kSradThreads), 0, m.stream, c, v);
            },
            q0sqr ? datum.data() : nullptr);
        if (rc == HCLIB_HIP_OK && q0sqr)
            for (int it = 0; it < niter; ++it) {
                const uint32_t b = (uint32_t)datum[(size_t)it * c.dstride];
                memcpy(&q0sqr[it], &b, 4);
            }
    } else {
        rc = hip_check(hipEventRecord(m.ev0, m.stream), "hipEventRecord");
        for (int it = 0; rc == HCLIB_HIP_OK && it < niter; ++it) {
            hipLaunchKernelGGL(k_srad_reduce, dim3(1), dim3(64), 0, m.stream, c, it);
            hipLaunchKernelGGL(k_srad_sweep, dim3((unsigned)p.nb), dim3(kSradThreads), 0, m.stream, c, it);
            rc = hip_check(hipGetLastError(), "hclib_hip_srad: the launch of an iteration");
        }
        if (rc == HCLIB_HIP_OK) rc = hip_check(hipEventRecord(m.ev1, m.stream), "hipEventRecord");
        const int rc_sync = hip_check(hipStreamSynchronize(m.stream), "hipStreamSynchronize");
        rc = rc ? rc : rc_sync;
        if (rc == HCLIB_HIP_OK) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, m.ev0, m.ev1);
            st.kernel_ms = ms;
            st.tasks = p.tasks;  // a wave per reduce and a workgroup per (iteration, block); no promises
            if (q0sqr) {
                std::vector<uint64_t> q((size_t)niter);
                HX_HIP(hipMemcpy(q.data(), c.qout, (size_t)niter * 8, hipMemcpyDeviceToHost));
                for (int it = 0; it < niter; ++it) {
                    const uint32_t b = (uint32_t)q[(size_t)it];
                    memcpy(&q0sqr[it], &b, 4);
                }
            }
        }
    }
    if (result) {
        result->tasks = st.tasks;
        result->puts = st.puts;
        result->releases = st.releases;
        result->kernel_ms = st.kernel_ms;
    }
    if (rc) return rc;
    HX_HIP(hipMemcpy(j, d + (niter & 1 ? stride : 0), gbytes, hipMemcpyDeviceToHost));
    return HCLIB_HIP_OK;
}
