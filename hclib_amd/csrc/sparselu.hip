// sparselu.hip — BOTS SparseLU (test/performance-regression/full-apps/bots/
// sparselu_single, sparselu_for: sparselu.ref.c, the HClib port sparselu.c) as
// one launch of the device promise DAG (include/hclib_hip/hx_dag.h,
// run_dag_group), its graph built by a symbolic pass over the block mask.
//
// The matrix is S x S blocks of B x B floats, each block present or absent.
// The reference's driver (sparselu.ref.c:300-322) walks kk and, per step,
// factors the diagonal block, solves the present blocks of row kk and column
// kk against it and updates every (ii, jj) whose (ii, kk) and (kk, jj) are
// present, allocating a zeroed block where (ii, jj) was absent (fill-in, :318).
// The HClib port closes two finish scopes per step (sparselu.c:331,348); here
// every block version is one promise and every block kernel one workgroup task:
//
//   task            awaits (last writer of)          writes    restates
//   lu0(kk)         (kk,kk)                          (kk,kk)   sparselu.ref.c:176-187
//   fwd(kk,jj)      (kk,jj) (kk,kk)                  (kk,jj)   :217-224
//   bdiv(ii,kk)     (ii,kk) (kk,kk)                  (ii,kk)   :192-202
//   bmod(ii,jj,kk)  (ii,jj) (ii,kk) (kk,jj)          (ii,jj)   :206-213
//
// The task set depends on the mask alone, so the host walks the reference's
// program order once (slu_plan): it marks fill-in, and per block remembers the
// task that made its newest version. A task awaits that task for the block it
// updates and for each block it reads; version 0 (uploaded by the host, or a
// zeroed fill-in block) is left out, so the one promise a task puts has the
// task's own id, and a task has at most 3 awaits.
//
// The in-place invariant. Every task writes exactly one block. Version v of a
// block is read only by the task that makes version v + 1. A block that is
// read as an operand is final and never written again: the diagonal after
// lu0, a row block after fwd, a column block after bdiv (every later step has
// kk' > kk and touches only blocks with ii, jj >= kk'). So blocks are updated
// in place in one device buffer; all blocks of the final mask are allocated up
// front and fill-ins are uploaded as +0.0.
//
// Arithmetic. Every element sees the reference's sequence of rounded
// operations: its updates in ascending k, each one f32 multiply rounded, then
// one f32 subtract rounded (never an FMA), then its IEEE divide where the
// reference has one. The reference's lu0 is right-looking and so is the one
// here; fwd and bdiv are left-looking over panels of 16 and bmod is
// register-blocked, which reorders work between elements but not the
// operations any one element sees: the result is bit-identical to the
// reference for every B in 1..128. There is no pivot check, as the reference
// has none: a zero pivot gives inf / NaN by IEEE rules and the call still
// returns HCLIB_HIP_OK. (The f32 MFMA is bitwise a chain of fmaf, which is not
// the reference's arithmetic: there is no MFMA or fused mode.)
//
// Every block access is an agent-scope (sc1) vector load or write-through
// store, the payload form run_dag_group hands from task to task behind a
// drain and a barrier (kSc1Payload), as in cholesky.hip.
#include <string.h>

#include <new>
#include <vector>

#include "hx_client.h"

namespace hx {
namespace {

constexpr int kSluThreads = 256;  // one task = one workgroup of four waves
constexpr int kSluMaxB = 128;
constexpr int kSluKc = 16;               // k per staged chunk of bmod, and the panel width of fwd / bdiv
constexpr int kSluLdS = kSluMaxB + 4;    // LDS row of bmod's staged operands (16 rows 4 words apart in the banks)
constexpr int kSluLdT = kSluMaxB + 1;    // LDS row of a whole block (lu0, fwd, bdiv)
constexpr int kSluLdsFloats = kSluMaxB * kSluLdT + kSluMaxB * kSluKc;  // a block and one operand panel
static_assert(2 * kSluKc * kSluLdS <= kSluLdsFloats, "bmod's two staged chunks fit");
enum : uint32_t { kSluLu0 = 0, kSluFwd = 1, kSluBdiv = 2, kSluBmod = 3 };

// workgroups per CU (HCLIB_HIP_SPARSELU_WGS overrides, 1 or 2). One: the default
// size is chain-bound and measured 1.3 % faster with one than with two
// (DESIGN.md §12); two give the bmod body alone 25 % more throughput.
constexpr int kSluWgsPerCu = 1;

struct SluCtx {
    float *blocks;    // block s at blocks + s B B, row-major inside
    const int *slot;  // [S S] a present block's position in `blocks` (written before the launch only)
    int S, B;
};

__device__ __forceinline__ float *slu_block(const SluCtx &c, uint32_t ii, uint32_t jj) {
    return c.blocks + (size_t)c.slot[ii * (uint32_t)c.S + jj] * (size_t)(c.B * c.B);
}

// every block access: agent-scope (sc1) loads and write-through stores
__device__ __forceinline__ float ldt(const float *p) { return ld_agent(p); }
__device__ __forceinline__ void stt(float *p, float v) { st_agent(p, v); }

__device__ __forceinline__ float *slu_lds() {
    __shared__ __attribute__((aligned(16))) float s[kSluLdsFloats];
    return s;
}

// sparselu.ref.c:206-213: inner[i][j] -= row[i][k] * col[k][j], k ascending.
// A thread owns an NB x NB register block (rows ty + 16 a, columns tx + 16 b;
// NB = ceil(B / 16), so the one code path covers every B with guarded edges)
// and walks k; the operands are staged through LDS 16 k at a time, the next
// chunk's loads in flight while this one is used.
template <int NB>
__device__ __forceinline__ void slu_bmod(const float *row, const float *col, float *inner, int B) {
    float *s1 = slu_lds(), *s2 = s1 + kSluKc * kSluLdS;
    const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    float acc[NB][NB];
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int i = ty + 16 * a, j = tx + 16 * b;
            acc[a][b] = (i < B && j < B) ? ldt(&inner[i * B + j]) : 0.0f;
        }
    // a chunk in registers: row[i][k0 + kk] (i = e / 16, kk = e % 16) and
    // col[k0 + kk][j] (kk = e / 128, j = e % 128), e = tid + 256 q
    constexpr int NQ = NB;  // i < 16 NB: q < NB covers every row of the block
    float r1[NQ], r2[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int e = tid + kSluThreads * q, i = e >> 4, k = k0 + (e & 15);
            r1[q] = (i < B && k < B) ? ldt(&row[i * B + k]) : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + kSluThreads * q, k = k0 + (e >> 7), j = e & 127;
            r2[q] = (j < B && k < B) ? ldt(&col[k * B + j]) : 0.0f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < B; k0 += kSluKc) {
        const int kn = B - k0 < kSluKc ? B - k0 : kSluKc;
        __syncthreads();  // the previous chunk's readers are done
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int e = tid + kSluThreads * q;
            s1[(e & 15) * kSluLdS + (e >> 4)] = r1[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + kSluThreads * q;
            s2[(e >> 7) * kSluLdS + (e & 127)] = r2[q];
        }
        __syncthreads();
        if (k0 + kSluKc < B) fetch(k0 + kSluKc);
        auto step = [&](int kk) {
            float l1[NB], t2[NB];
#pragma unroll
            for (int a = 0; a < NB; ++a) l1[a] = s1[kk * kSluLdS + ty + 16 * a];
#pragma unroll
            for (int b = 0; b < NB; ++b) t2[b] = s2[kk * kSluLdS + tx + 16 * b];
#pragma unroll
            for (int a = 0; a < NB; ++a)
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    float p = __fmul_rn(l1[a], t2[b]);
#if defined(HX_SLU_SCALAR) && HX_SLU_SCALAR
                    // one v_mul_f32 and one v_sub_f32 per element: the product is
                    // opaque to the compiler, which otherwise pairs neighbouring
                    // elements into v_pk_mul_f32 / v_pk_add_f32
                    asm("" : "+v"(p));
#endif
                    acc[a][b] = __fsub_rn(acc[a][b], p);
                }
        };
        if (kn == kSluKc) {
#pragma unroll 4
            for (int kk = 0; kk < kSluKc; ++kk) step(kk);
        } else {
            for (int kk = 0; kk < kn; ++kk) step(kk);
        }
    }
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int i = ty + 16 * a, j = tx + 16 * b;
            if (i < B && j < B) stt(&inner[i * B + j], acc[a][b]);
        }
}

__device__ __forceinline__ void slu_bmod_any(const float *row, const float *col, float *inner, int B) {
    switch ((B + 15) >> 4) {
        case 1: slu_bmod<1>(row, col, inner, B); break;
        case 2: slu_bmod<2>(row, col, inner, B); break;
        case 3: slu_bmod<3>(row, col, inner, B); break;
        case 4: slu_bmod<4>(row, col, inner, B); break;
        case 5: slu_bmod<5>(row, col, inner, B); break;
        case 6: slu_bmod<6>(row, col, inner, B); break;
        case 7: slu_bmod<7>(row, col, inner, B); break;
        default: slu_bmod<8>(row, col, inner, B); break;
    }
}

// a whole block between global memory and LDS, coalesced: T[r][c] = X[r][c],
// or transposed (T[c][r]); 16 loads in flight per thread (one memory latency
// per 32 rows, not per row)
template <bool TRANSPOSE>
__device__ __forceinline__ void slu_block_in(float *T, const float *X, int B) {
    const int c = (int)threadIdx.x & 127;
    for (int r0 = (int)threadIdx.x >> 7; r0 < B; r0 += 32) {
        float v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int r = r0 + 2 * q;
            v[q] = (c < B && r < B) ? ldt(&X[r * B + c]) : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int r = r0 + 2 * q;
            if (c < B && r < B) T[TRANSPOSE ? c * kSluLdT + r : r * kSluLdT + c] = v[q];
        }
    }
}
template <bool TRANSPOSE>
__device__ __forceinline__ void slu_block_out(float *X, const float *T, int B) {
    const int c = (int)threadIdx.x & 127;
    if (c < B)
        for (int r = (int)threadIdx.x >> 7; r < B; r += 2)
            stt(&X[r * B + c], T[TRANSPOSE ? c * kSluLdT + r : r * kSluLdT + c]);
}

// sparselu.ref.c:176-187, right-looking as the reference, the block in LDS.
// Step k in two phases: thread i > k divides diag[i][k] by the pivot (one
// divide sequence for the whole column); then a wave takes rows i > k four
// apart, four at a time, its lanes the columns j > k. Loads go to clamped
// addresses (the pad column, the last row) instead of branching; only the
// stores are predicated.
__device__ __forceinline__ void slu_lu0(float *diag, int B) {
    constexpr int R = 4;
    float *A = slu_lds();
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    slu_block_in<false>(A, diag, B);
    __syncthreads();
    for (int k = 0; k + 1 < B; ++k) {
        if (tid > k && tid < B) A[tid * kSluLdT + k] = __fdiv_rn(A[tid * kSluLdT + k], A[k * kSluLdT + k]);
        __syncthreads();  // column k holds L
        const int j0 = k + 1 + lane, j1 = j0 + 64;
        const bool c0 = j0 < B, c1 = j1 < B, two = k + 65 < B;  // `two`: some lane has a second column (wave-uniform)
        const int jc0 = c0 ? j0 : kSluMaxB, jc1 = c1 ? j1 : kSluMaxB;
        const float u0 = A[k * kSluLdT + jc0], u1 = A[k * kSluLdT + jc1];
        for (int i0 = k + 1 + wave; i0 < B; i0 += 4 * R) {
            float l[R], a0[R], a1[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = i0 + 4 * r < B ? i0 + 4 * r : B - 1;
                l[r] = A[i * kSluLdT + k];
                a0[r] = A[i * kSluLdT + jc0];
            }
            if (two) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int i = i0 + 4 * r < B ? i0 + 4 * r : B - 1;
                    a1[r] = A[i * kSluLdT + jc1];
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = i0 + 4 * r;
                if (i < B && c0) A[i * kSluLdT + j0] = __fsub_rn(a0[r], __fmul_rn(l[r], u0));
            }
            if (two) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int i = i0 + 4 * r;
                    if (i < B && c1) A[i * kSluLdT + j1] = __fsub_rn(a1[r], __fmul_rn(l[r], u1));
                }
            }
        }
        __syncthreads();  // row k + 1 and column k + 1 are complete
    }
    slu_block_out<false>(diag, A, B);
}

// fwd (sparselu.ref.c:217-224): col[i][j] -= diag[i][k] * col[k][j], k < i:
// thread t owns column t of `col`, its vector v[e] = col[e][t].
// bdiv (:192-202): row[i][j] takes row[i][k] * diag[k][j], k < j, then
// / diag[j][j]: thread t owns row t of `row`, v[e] = row[t][e].
// Left-looking over panels of 16 entries of v: the panel in registers takes
// the finished entries k < p0 in ascending k, then the panel's own triangle.
// op[k][c] is the diagonal block's operand of entry p0 + c at k:
// diag[p0 + c][k] (fwd), diag[k][p0 + c] (bdiv). A thread reads only its own
// column of V, so the panels need no barrier but the operand panel's; the next
// panel's operands are loaded while this one is solved.
template <bool FWD>
__device__ __forceinline__ void slu_solve(const float *diag, float *X, int B) {
    float *V = slu_lds(), *op = V + kSluMaxB * kSluLdT;
    const int tid = (int)threadIdx.x;
    // the operand panel of p0 in registers: op[k][c], k < p0 + w, e = k 16 + c
    float nxt[8];
    auto fetch = [&](int p0) {
        const int w = B - p0 < kSluKc ? B - p0 : kSluKc, nk = p0 + w;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + kSluThreads * q, k = e >> 4, c = e & 15;
            nxt[q] = (k < nk && c < w) ? ldt(FWD ? &diag[(p0 + c) * B + k] : &diag[k * B + p0 + c]) : 0.0f;
        }
    };
    fetch(0);
    slu_block_in<!FWD>(V, X, B);  // V[e][t]
    for (int p0 = 0; p0 < B; p0 += kSluKc) {
        const int w = B - p0 < kSluKc ? B - p0 : kSluKc;
        __syncthreads();  // the previous panel's readers are done (first: V is in place)
#pragma unroll
        for (int q = 0; q < 8; ++q) op[tid + kSluThreads * q] = nxt[q];
        __syncthreads();
        if (p0 + kSluKc < B) fetch(p0 + kSluKc);  // in flight while this panel is solved
        if (tid < B) {
            float x[kSluKc];
#pragma unroll
            for (int c = 0; c < kSluKc; ++c) x[c] = c < w ? V[(p0 + c) * kSluLdT + tid] : 0.0f;
#pragma unroll 4
            for (int k = 0; k < p0; ++k) {
                const float vk = V[k * kSluLdT + tid];
                const float4 *o4 = (const float4 *)(op + k * kSluKc);
                float u[kSluKc];
#pragma unroll
                for (int q = 0; q < kSluKc / 4; ++q) {
                    const float4 t = o4[q];
                    u[4 * q] = t.x, u[4 * q + 1] = t.y, u[4 * q + 2] = t.z, u[4 * q + 3] = t.w;
                }
#pragma unroll
                for (int c = 0; c < kSluKc; ++c)
                    x[c] = __fsub_rn(x[c], FWD ? __fmul_rn(u[c], vk) : __fmul_rn(vk, u[c]));
            }
#pragma unroll
            for (int kk = 0; kk < kSluKc; ++kk) {
                if (kk < w) {
                    const float *o = op + (p0 + kk) * kSluKc;
                    if (!FWD) x[kk] = __fdiv_rn(x[kk], o[kk]);
#pragma unroll
                    for (int c = kk + 1; c < kSluKc; ++c)
                        x[c] = __fsub_rn(x[c], FWD ? __fmul_rn(o[c], x[kk]) : __fmul_rn(x[kk], o[c]));
                }
            }
#pragma unroll
            for (int c = 0; c < kSluKc; ++c)
                if (c < w) V[(p0 + c) * kSluLdT + tid] = x[c];
        }
    }
    __syncthreads();
    slu_block_out<!FWD>(X, V, B);
}

struct SluKind : OnePromiseKind<SluCtx> {
    static constexpr bool kSc1Payload = true;  // blocks move by ld_agent / st_agent only (ldt / stt)
    __device__ static bool run_group(const Ctx &c, uint32_t, const uint32_t *pl, int) {
        const uint32_t kind = pl[0], kk = pl[1], ii = pl[2], jj = pl[3];
        const int B = c.B;
        if (kind == kSluLu0) slu_lu0(slu_block(c, kk, kk), B);
        else if (kind == kSluFwd) slu_solve<true>(slu_block(c, kk, kk), slu_block(c, kk, jj), B);
        else if (kind == kSluBdiv) slu_solve<false>(slu_block(c, kk, kk), slu_block(c, ii, kk), B);
        else slu_bmod_any(slu_block(c, ii, kk), slu_block(c, kk, jj), slu_block(c, ii, jj), B);
        return true;
    }
};

__global__ __launch_bounds__(kSluThreads, 2) void k_sparselu(SluCtx c, DagView v) {
    run_dag_group<SluKind>(c, v, nullptr);
}

// the bmod body alone on resident blocks: workgroup g repeats bmod on its own
// three blocks (the throughput floor of DESIGN.md §12)
__global__ __launch_bounds__(kSluThreads, 2) void k_sparselu_bmod_rate(float *buf, int B, int reps) {
    float *b = buf + (size_t)blockIdx.x * 3 * (size_t)(B * B);
    for (int r = 0; r < reps; ++r) {
        slu_bmod_any(b, b + B * B, b + 2 * B * B, B);
        __syncthreads();
    }
}

struct SluPlan {
    std::vector<uint8_t> mask;  // the final structure
    uint64_t counts[6] = {0, 0, 0, 0, 0, 0};  // lu0, fwd, bdiv, bmod, blocks in, blocks out
    VersionGraph graph;  // filled when `graph`
};

// The symbolic pass, in two parts. First the structure and the counts alone,
// on one bitset per block row: at step kk the present blocks of row kk right of
// the diagonal are OR-ed into every row ii > kk whose (ii, kk) is present (the
// fill-in of that step's bmods, sparselu.ref.c:318), and the step's tasks are
// counted from the two populations. A task count hclib_hip_dag_begin cannot take
// is rejected here, before any graph array grows. Then, if asked for, the graph
// in the reference's program order (sparselu.ref.c:300-322). Step kk only
// creates blocks with both indices above kk, so the blocks of row kk and of
// column kk that step kk meets are those of the final structure.
int slu_plan(const uint8_t *mask, int S, bool graph, SluPlan &p, const char *who) {
    if (!mask) {
        set_error("%s: mask must not be NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    if (S < 1) {
        set_error("%s: the matrix size %d (blocks per side) must be positive", who, S);
        return HCLIB_HIP_EINVAL;
    }
    try {
        const size_t n = (size_t)S, nn = n * n, W = (n + 63) / 64;
        std::vector<uint64_t> bits(n * W, 0), cb(W);
        for (size_t ii = 0; ii < n; ++ii)
            for (size_t jj = 0; jj < n; ++jj)
                if (mask[ii * n + jj]) {
                    bits[ii * W + jj / 64] |= 1ull << (jj % 64);
                    ++p.counts[4];
                }
        auto has = [&](size_t ii, size_t jj) { return (bits[ii * W + jj / 64] >> (jj % 64)) & 1ull; };
        for (size_t k = 0; k < n; ++k)
            if (!has(k, k)) {  // the reference's lu0 would dereference NULL
                set_error("%s: the diagonal block (%zu, %zu) is absent", who, k, k);
                return HCLIB_HIP_EINVAL;
            }
        uint64_t ntasks = 0;
        for (size_t kk = 0; kk < n; ++kk) {
            // row kk right of the diagonal
            const size_t w0 = (kk + 1) / 64;
            uint64_t ncols = 0, nrows = 0;
            for (size_t w = w0; w < W; ++w) {
                cb[w] = bits[kk * W + w];
                if (w == w0) cb[w] &= ~0ull << ((kk + 1) % 64);
                ncols += (uint64_t)__builtin_popcountll(cb[w]);
            }
            for (size_t ii = kk + 1; ii < n; ++ii)
                if (has(ii, kk)) {
                    ++nrows;
                    for (size_t w = w0; w < W; ++w) bits[ii * W + w] |= cb[w];
                }
            p.counts[kSluLu0] += 1;
            p.counts[kSluFwd] += ncols;
            p.counts[kSluBdiv] += nrows;
            p.counts[kSluBmod] += nrows * ncols;
            ntasks += 1 + ncols + nrows + nrows * ncols;
            // the limit of hclib_hip_dag_begin: task ids below 2^32 - 1
            if (ntasks >= (uint64_t)kDagEmpty) {
                set_error("%s: more than %u tasks, above what hclib_hip_dag_begin accepts", who, kDagEmpty - 1);
                return HCLIB_HIP_EINVAL;
            }
        }
        p.mask.resize(nn);
        for (size_t ii = 0; ii < n; ++ii)
            for (size_t jj = 0; jj < n; ++jj) p.counts[5] += p.mask[ii * n + jj] = (uint8_t)has(ii, jj);
        if (!graph) return HCLIB_HIP_OK;

        VersionGraph &g = p.graph = VersionGraph(nn);
        std::vector<uint32_t> rows, cols;
        g.reserve((size_t)ntasks, 0);  // (the awaits grow as they come: a plan may be all there is memory for)
        for (uint32_t kk = 0; kk < n; ++kk) {
            const size_t d = kk * n + kk;
            g.task(kSluLu0, kk, kk, kk, d, {d});
            rows.clear();
            cols.clear();
            for (uint32_t jj = kk + 1; jj < n; ++jj)
                if (p.mask[kk * n + jj]) {
                    g.task(kSluFwd, kk, kk, jj, kk * n + jj, {kk * n + jj, d});
                    cols.push_back(jj);
                }
            for (uint32_t ii = kk + 1; ii < n; ++ii)
                if (p.mask[ii * n + kk]) {
                    g.task(kSluBdiv, kk, ii, kk, ii * n + kk, {ii * n + kk, d});
                    rows.push_back(ii);
                }
            for (uint32_t ii : rows)
                for (uint32_t jj : cols) g.task(kSluBmod, kk, ii, jj, ii * n + jj, {ii * n + jj, ii * n + kk, kk * n + jj});
        }
    } catch (const std::bad_alloc &) {
        set_error("%s: out of host memory for the plan of %d x %d blocks", who, S, S);
        return HCLIB_HIP_ENOMEM;
    }
    return HCLIB_HIP_OK;
}

// the reference's operations per block kernel (divides and the multiply and
// subtract of every update, as sparselu.ref.c:176-224 execute them)
double slu_flops(const uint64_t counts[6], int B) {
    const double b = B;
    const double lu0 = b * (b - 1) / 2 + (b - 1) * b * (2 * b - 1) / 3;
    const double fwd = b * b * (b - 1), bdiv = b * b * b, bmod = 2 * b * b * b;
    return counts[0] * lu0 + counts[1] * fwd + counts[2] * bdiv + counts[3] * bmod;
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_sparselu_genmat(int S, int B, uint8_t *mask, float *blocks) {
    if (!mask) {
        set_error("hclib_hip_sparselu_genmat: mask must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    if (S < 1 || B < 1) {
        set_error("hclib_hip_sparselu_genmat: the matrix size %d and the block size %d must be positive", S, B);
        return HCLIB_HIP_EINVAL;
    }
    // The structure (sparselu.ref.c:94-106): the three central diagonals, and
    // off them the blocks whose indices are both even with the smaller one a
    // multiple of 3. The values (:117-125): one 16-bit multiplicative
    // congruential sequence (x 3125 mod 2^16, from 1325) through the present
    // blocks in row-major order, mapped to [-2, 2) in steps of 2^-14 (exact in
    // float).
    uint32_t state = 1325;
    float *dst = blocks;
    const size_t per_block = (size_t)B * B;
    for (int ii = 0; ii < S; ++ii)
        for (int jj = 0; jj < S; ++jj) {
            const int lo = ii < jj ? ii : jj, hi = ii < jj ? jj : ii;
            const bool present = hi - lo <= 1 || (ii % 2 == 0 && jj % 2 == 0 && lo % 3 == 0);
            mask[(size_t)ii * S + jj] = present ? 1 : 0;
            if (!present || !blocks) continue;
            for (size_t e = 0; e < per_block; ++e) {
                state = (state * 3125u) & 0xffffu;
                *dst++ = (float)((int)state - 32768) / 16384.0f;
            }
        }
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_sparselu_plan(const uint8_t *mask, int S, uint8_t *mask_out, uint64_t counts[6],
                                       uint32_t *payload, uint32_t *await_off, uint32_t *await_ids) {
    const bool graph = payload || await_off || await_ids;
    if (graph && !(payload && await_off && await_ids)) {
        set_error("hclib_hip_sparselu_plan: payload, await_off and await_ids go together (all or none)");
        return HCLIB_HIP_EINVAL;
    }
    SluPlan p;
    HX_TRY(slu_plan(mask, S, graph, p, "hclib_hip_sparselu_plan"));
    if (mask_out) memcpy(mask_out, p.mask.data(), p.mask.size());
    if (counts) memcpy(counts, p.counts, sizeof(p.counts));
    if (graph) {
        const VersionGraph &g = p.graph;
        memcpy(payload, g.payload.data(), g.payload.size() * sizeof(uint32_t));
        memcpy(await_off, g.off.data(), g.off.size() * sizeof(uint32_t));
        if (!g.ids.empty()) memcpy(await_ids, g.ids.data(), g.ids.size() * sizeof(uint32_t));
    }
    return HCLIB_HIP_OK;
}

static int slu_run(const uint8_t *mask, const float *blocks, int S, int B, uint8_t *mask_out, float *blocks_out,
                   hclib_hip_sparselu_result_t *result) {
    // argument errors first, before the device is touched
    if (!mask || !blocks || !mask_out || !blocks_out) {
        set_error("hclib_hip_sparselu: mask, blocks, mask_out and blocks_out must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    if (B < 1 || B > kSluMaxB) {
        set_error("hclib_hip_sparselu: the block size %d is outside 1 .. %d", B, kSluMaxB);
        return HCLIB_HIP_EINVAL;
    }
    SluPlan p;
    HX_TRY(slu_plan(mask, S, true, p, "hclib_hip_sparselu"));
    HX_TRY(ensure_device());
    Module &m = mod();

    // all blocks of the final mask, packed in row-major (ii, jj) order: the
    // input's blocks, and fill-ins as +0.0
    const size_t nn = (size_t)S * S, B2 = (size_t)B * B, nout = (size_t)p.counts[5];
    const size_t o_slot = (nout * B2 * sizeof(float) + 255) / 256 * 256, bytes = o_slot + nn * sizeof(int);
    std::vector<char> h(bytes, 0);
    float *hb = (float *)h.data();
    int *slot = (int *)(h.data() + o_slot);
    size_t in_pos = 0, out_pos = 0;
    for (size_t e = 0; e < nn; ++e) {
        slot[e] = p.mask[e] ? (int)out_pos : -1;
        if (mask[e]) memcpy(hb + out_pos * B2, blocks + in_pos++ * B2, B2 * sizeof(float));
        if (p.mask[e]) ++out_pos;
    }
    char *buf = nullptr;
    HX_TRY(arena_reserve(kArenaSparselu, bytes, "hclib_hip_sparselu", (void **)&buf));
    // (`h` outlives the copy: launch_dag_group synchronises the stream)
    HX_HIP(hipMemcpyAsync(buf, h.data(), bytes, hipMemcpyHostToDevice, m.stream));

    SluCtx c;
    c.blocks = (float *)buf;
    c.slot = (const int *)(buf + o_slot);
    c.S = S;
    c.B = B;
    int wgs = env_int("HCLIB_HIP_SPARSELU_WGS", kSluWgsPerCu);
    if (wgs < 1 || wgs > 2) wgs = kSluWgsPerCu;
    // never more workgroups than the kernel's LDS and registers let a CU hold
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_sparselu, kSluThreads, 0) == hipSuccess &&
        per_cu >= 1 && wgs > per_cu)
        wgs = per_cu;
    // (no body reports a device error of its own: the launch's error word,
    // run_dag_group's, is checked by hclib_hip_dag_end)
    hclib_hip_dag_stats_t st{};
    HX_TRY(launch_dag_group(p.graph, wgs, (const void *)k_sparselu, kSluThreads, "hclib_hip_sparselu", &st,
                            [&](int grid, const DagView &v) {
                                hipLaunchKernelGGL(k_sparselu, dim3(grid), dim3(kSluThreads), 0, m.stream, c, v);
                            }));
    HX_HIP(hipMemcpy(blocks_out, buf, nout * B2 * sizeof(float), hipMemcpyDeviceToHost));
    memcpy(mask_out, p.mask.data(), nn);
    if (result) {
        result->blocks_in = p.counts[4];
        result->blocks_out = p.counts[5];
        result->lu0 = p.counts[0];
        result->fwd = p.counts[1];
        result->bdiv = p.counts[2];
        result->bmod = p.counts[3];
        result->tasks = st.tasks;
        result->puts = st.puts;
        result->releases = st.releases;
        result->kernel_ms = st.kernel_ms;
        result->gflops = st.kernel_ms > 0 ? slu_flops(p.counts, B) / (st.kernel_ms * 1e6) : 0.0;
        result->wgs_per_cu = wgs;
    }
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_sparselu(const uint8_t *mask, const float *blocks, int S, int B, uint8_t *mask_out,
                                  float *blocks_out, hclib_hip_sparselu_result_t *result) {
    try {
        return slu_run(mask, blocks, S, B, mask_out, blocks_out, result);
    } catch (const std::bad_alloc &) {  // no exception crosses the C ABI
        set_error("hclib_hip_sparselu: out of host memory for %d x %d blocks of %d x %d", S, S, B, B);
        return HCLIB_HIP_ENOMEM;
    }
}

extern "C" int hclib_hip_sparselu_bmod_rate(int B, int wgs_per_cu, int reps, double *ms, double *gflops) {
    if (B < 1 || B > kSluMaxB || wgs_per_cu < 1 || wgs_per_cu > 2 || reps < 1 || !ms || !gflops) {
        set_error("hclib_hip_sparselu_bmod_rate: invalid arguments");
        return HCLIB_HIP_EINVAL;
    }
    HX_TRY(ensure_device());
    Module &m = mod();
    const int grid = m.num_cus * wgs_per_cu;
    const size_t B2 = (size_t)B * B, nfloats = (size_t)grid * 3 * B2;
    // operands of magnitude 1 / B, so that the repeated updates stay finite
    std::vector<float> h(nfloats);
    uint32_t x = 12345u;
    for (size_t e = 0; e < nfloats; ++e) {
        x = x * 1664525u + 1013904223u;
        h[e] = ((float)(x >> 8) / 8388608.0f - 1.0f) / (float)B;
    }
    float *buf = nullptr;
    HX_TRY(arena_reserve(kArenaSparselu, nfloats * sizeof(float), "hclib_hip_sparselu_bmod_rate", (void **)&buf));
    HX_HIP(hipMemcpy(buf, h.data(), nfloats * sizeof(float), hipMemcpyHostToDevice));
    HX_TRY(check_resident((const void *)k_sparselu_bmod_rate, grid, kSluThreads, 0, "hclib_hip_sparselu_bmod_rate"));
    hipLaunchKernelGGL(k_sparselu_bmod_rate, dim3(grid), dim3(kSluThreads), 0, m.stream, buf, B, 1);
    HX_HIP(hipEventRecord(m.ev0, m.stream));
    hipLaunchKernelGGL(k_sparselu_bmod_rate, dim3(grid), dim3(kSluThreads), 0, m.stream, buf, B, reps);
    HX_HIP(hipEventRecord(m.ev1, m.stream));
    HX_HIP(hipEventSynchronize(m.ev1));
    float t = 0;
    HX_HIP(hipEventElapsedTime(&t, m.ev0, m.ev1));
    *ms = t;
    *gflops = t > 0 ? 2.0 * B * B * B * (double)reps * grid / (t * 1e6) : 0.0;
    return HCLIB_HIP_OK;
}
