// strassen.hip — BOTS Strassen (test/performance-regression/full-apps/bots/
// strassen: strassen.ref.c the algorithm, strassen.c the HClib port) as a
// fork-join client of dynamic device dataflow (include/hclib_hip/hx_dyn.h):
// OptimizedStrassenMultiply(C, A, B, size, ldc, lda, ldb), C = A x B, as one
// launch of run_dyn_worker, every matrix bit-identical to the reference's.
//
//   task                       does (strassen.ref.c lines)
//   MUL(C, A, B, size, fin,    size <= cutoff (:421-424): a base of at most 64 is
//       level, path)           one wave's job, which checks out of fin; a larger
//                              base checks (size / 64)^2 - 1 more tasks in to fin
//                              and spawns one TILE per 64 x 64 output tile.
//                              Otherwise, with q = size / 2 and nb = ceil(q /
//                              band_rows): f0 = open(nb), nb PRE bands into f0 and
//                              FORK awaiting f0; fin passes to the continuations
//   PRE(rows of the S sweep)   :461-499, `rows` rows of S1 .. S8, checks out of f0
//   FORK                       f1 = open(7), the seven products (:501-520) as MUL
//                              children into f1 with the reference's row widths,
//                              and POST awaiting f1 (the port's seven asyncs and
//                              its taskwait, strassen.c:1331)
//   POST                       checks nb tasks in to fin, spawns nb COMBINE bands
//                              with fin, and checks out of fin itself
//   COMBINE(rows)              :527-577, `rows` rows of the combination sweep,
//                              checks out of fin
//   TILE(C, A, B, K, fin)      one 64 x 64 tile of a base larger than 64: the full
//                              k chain of its elements, checks out of fin
//
// The root MUL (fin = kDynOpen in its payload) opens the program's outer finish.
//
// Every element of a base product is the reference's chain (MultiplyByDivide-
// AndConquer and the two Fast*NaiveMatrixMultiply kernels, :104-384):
//   ((a[i][0] b[0][j]) + a[i][1] b[1][j]) + ... + a[i][size-1] b[size-1][j]
// k strictly ascending, each product rounded, then each sum rounded, starting
// from the FIRST PRODUCT and not from 0.0 (a zero row of A times a negative B
// gives -0.0). The bodies are plain VALU f64: v_mul_f64 and v_add_f64 under
// -ffp-contract=off, no v_fma_f64 and no f64 MFMA (whose internal rounding no
// document here states). Which lane computes which element is free: a lane
// holds an (T/8) x (T/8) block of accumulators of the T x T tile, A and B go
// through LDS 8 columns / rows of k at a time (A transposed, so that a lane's
// rows are contiguous).
//
// Workspace: no device allocator. The call tree depends on (n, cutoff) alone, so
// the eleven q x q temporaries of every call (S1 .. S8, M2, M5, T1sMULT, in that
// order, the reference's malloc :438) sit at a closed-form offset of one
// arena: one region per recursion level, the call's base-7 path its index in it,
// region[level] + path * 11 q^2. All calls can be live at once: nothing is
// reused. The arena is [A n^2][B n^2][C n^2][regions], and payloads carry u32
// element offsets into it (the host refuses an arena of 2^32 elements or more).
//
// Memory protocol. Every double a task writes is stored write-through (16-byte
// agent-scope sc1 stores, st_sc1_x4) and drained by the task's check-out
// (dyn_finish_check_out<true>); every double is read with plain loads behind
// run_dyn_worker's agent acquire (kSc1Payload = false). The other valid form,
// plain stores released by the fence of dyn_finish_check_out<false>, is kept
// behind HCLIB_HIP_STRASSEN_SC1=0 (DESIGN.md §14 has both, measured).
// The C quadrants are read, modified and written across CUs: a child writes a
// tile of C21 on one CU, and a COMBINE band of the parent on another computes
// C21 = -C21 + T2 in place. Why the band reads the child's values: the child's
// stores are out of its CU (write-through, or written back by the release
// fence) before its check-out's decrement of f1; the decrement that reaches
// zero comes after every other one and puts f1; POST is released by that put
// and creates the band after it; the band's wave acquires (invalidating its
// CU's L1 and the stale lines of its L2) after it has read its ready slot and
// before its first load. Nobody reads a C quadrant between the child's store
// and the band (the seven products of one call write disjoint quadrants and
// read only A, B and the S temporaries), and nobody but the band writes its
// rows afterwards until it has checked out of fin, whose put in turn orders
// the grandparent's band after it in the same way. Concurrent writers never
// share a 128-byte line: quadrant offsets and row widths are multiples of 16
// doubles, bands split by rows, tiles are 512 bytes wide.
#include <string.h>

#include "hx_client.h"

namespace hx {
namespace {

constexpr int kStrWords = 12;          // payload words per task
constexpr int kStrWavesPerCu = 8;      // 8 x 8.1 KB of LDS per CU
constexpr int kStrMaxLevels = 12;      // n <= 16384 and cutoff >= 16: at most 10
constexpr int kStrMaxN = 16384;
constexpr uint32_t kStrTile = 64;      // one wave's output tile edge
constexpr int kStrKc = 8;              // k per LDS stage
// Defaults by the size of the tree (measured): with fewer than kStrBigTree leaf multiplies the
// launch is bound by its span and by the waves that wait for work, and runs faster on fewer waves and
// smaller bands; from there on it is bound by throughput
constexpr unsigned long long kStrBigTree = 8192, kStrSmallTree = 1024;
constexpr int kStrBandSmall = 8, kStrBandBig = 16;  // rows per PRE / COMBINE band
enum : uint32_t { kStrMul = 0, kStrFork = 1, kStrPost = 2, kStrPre = 3, kStrCombine = 4, kStrTileTask = 5 };
enum : int { kCntBase = 0, kCntPre = 1, kCntCombine = 2, kCntSplit = 3, kCntFork = 4, kCntPost = 5, kCntTile = 6,
             kCntKinds = 7 };

struct StrCtx {
    double *m;                   // the arena: A, B, C, then the regions of temporaries
    unsigned long long *counts;  // per task class (hx_client.h class_count)
    unsigned long long total;    // elements of the arena
    unsigned long long region[kStrMaxLevels];  // element offset of each level's region
    uint32_t cutoff, band_rows;
};

__device__ __forceinline__ double *str_lds() {
    __shared__ __attribute__((aligned(16))) double s[kStrKc * (kStrTile + 2) + kStrKc * kStrTile];
    return s;
}

// two doubles at a 16-byte aligned address: a plain store, released by the
// check-out's fence, or (SC1) a write-through store the check-out only drains.
// The form is the kernel's template argument: a run-time flag put a branch
// around every store
template <bool SC1>
__device__ __forceinline__ void str_store2(double *p, double x, double y) {
    if (SC1) {
        st_sc1_x4(p, make_uint4((uint32_t)__double2loint(x), (uint32_t)__double2hiint(x), (uint32_t)__double2loint(y),
                                (uint32_t)__double2hiint(y)));
    } else {
        *(double2 *)p = make_double2(x, y);
    }
}

// C[T x T] = A[T x K] B[K x T], every element the reference's chain: k ascending,
// the first product its start, multiply and add rounded separately. Lane
// (ty, tx) of the 8 x 8 grid holds rows ty * M .. + M, columns tx * M .. + M.
template <int T, bool SC1>
__device__ __forceinline__ void str_mul(double *C, uint32_t ldc, const double *A, uint32_t lda, const double *B,
                                        uint32_t ldb, uint32_t K) {
    constexpr int M = T / 8;        // edge of a lane's block of accumulators
    constexpr int V = T / 16;       // 16-byte loads per lane, operand and stage: T * kStrKc / 2 / 64
    constexpr int LA = T + 2;       // row stride of the transposed A stage (spreads the banks, keeps 16-B alignment)
    double *As = str_lds(), *Bs = As + kStrKc * (kStrTile + 2);
    const int lane = lane_id(), ty = lane >> 3, tx = lane & 7;
    double acc[M][M];
    for (uint32_t k0 = 0; k0 < K; k0 += kStrKc) {
        if (k0) __syncthreads();  // the stage before has been read
#pragma unroll
        for (int x = 0; x < V; ++x) {
            const int v = lane + 64 * x;
            const int i = v >> 2, kk = (v & 3) * 2;
            const double2 a = *(const double2 *)(A + (size_t)i * lda + k0 + kk);
            As[kk * LA + i] = a.x;
            As[(kk + 1) * LA + i] = a.y;
            const int kr = v / (T / 2), j = (v % (T / 2)) * 2;
            *(double2 *)(Bs + kr * T + j) = *(const double2 *)(B + (size_t)(k0 + kr) * ldb + j);
        }
        __syncthreads();
        // (not unrolled: with two steps in flight the kernel needs more than the 256 registers that let two
        // waves share a SIMD)
#pragma unroll 1
        for (int kk = 0; kk < kStrKc; ++kk) {
            double a[M], b[M];
#pragma unroll
            for (int r = 0; r < M; r += 2) {
                const double2 t = *(const double2 *)(As + kk * LA + ty * M + r);
                a[r] = t.x, a[r + 1] = t.y;
            }
#pragma unroll
            for (int cc = 0; cc < M; cc += 2) {
                const double2 t = *(const double2 *)(Bs + kk * T + tx * M + cc);
                b[cc] = t.x, b[cc + 1] = t.y;
            }
            if (k0 == 0 && kk == 0) {
#pragma unroll
                for (int r = 0; r < M; ++r)
#pragma unroll
                    for (int cc = 0; cc < M; ++cc) acc[r][cc] = a[r] * b[cc];
            } else {
#pragma unroll
                for (int r = 0; r < M; ++r)
#pragma unroll
                    for (int cc = 0; cc < M; ++cc) {
                        const double p = a[r] * b[cc];  // rounded on its own: -ffp-contract=off
                        acc[r][cc] = acc[r][cc] + p;
                    }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
        for (int cc = 0; cc < M; cc += 2)
            str_store2<SC1>(C + (size_t)(ty * M + r) * ldc + tx * M + cc, acc[r][cc], acc[r][cc + 1]);
    __syncthreads();  // the next task's stage overwrites the LDS
}

__device__ __forceinline__ double2 str_ld2(const double *p) { return *(const double2 *)p; }

// rows [row0, row0 + rows) of the S sweep (:461-499), in the order of the
// reference's nested assignments; W is the call's S1
template <bool SC1>
__device__ __forceinline__ void str_pre(const double *A, uint32_t lda, const double *B, uint32_t ldb, double *W,
                                        uint32_t q, uint32_t row0, uint32_t rows) {
    const uint32_t hq = q >> 1, sh = (uint32_t)__builtin_ctz(hq), total = rows << sh;
    const size_t qq = (size_t)q * q;
    for (uint32_t v = (uint32_t)lane_id(); v < total; v += 64) {
        const uint32_t r = row0 + (v >> sh), cc = (v & (hq - 1)) * 2;
        const double *pa = A + (size_t)r * lda + cc, *pb = B + (size_t)r * ldb + cc;
        const double2 a11 = str_ld2(pa), a12 = str_ld2(pa + q), a21 = str_ld2(pa + (size_t)q * lda),
                      a22 = str_ld2(pa + (size_t)q * lda + q);
        const double2 b11 = str_ld2(pb), b12 = str_ld2(pb + q), b21 = str_ld2(pb + (size_t)q * ldb),
                      b22 = str_ld2(pb + (size_t)q * ldb + q);
        const double2 s1 = a21 + a22, s2 = s1 - a11, s4 = a12 - s2;
        const double2 s5 = b12 - b11, s6 = b22 - s5, s8 = s6 - b21;
        const double2 s3 = a11 - a21, s7 = b22 - b12;
        double *o = W + (size_t)r * q + cc;
        str_store2<SC1>(o, s1.x, s1.y);
        str_store2<SC1>(o + qq, s2.x, s2.y);
        str_store2<SC1>(o + 2 * qq, s3.x, s3.y);
        str_store2<SC1>(o + 3 * qq, s4.x, s4.y);
        str_store2<SC1>(o + 4 * qq, s5.x, s5.y);
        str_store2<SC1>(o + 5 * qq, s6.x, s6.y);
        str_store2<SC1>(o + 6 * qq, s7.x, s7.y);
        str_store2<SC1>(o + 7 * qq, s8.x, s8.y);
    }
}

// rows [row0, row0 + rows) of the combination sweep (:527-577); W is the call's S1
template <bool SC1>
__device__ __forceinline__ void str_combine(double *C, uint32_t ldc, const double *W, uint32_t q, uint32_t row0,
                                            uint32_t rows) {
    const uint32_t hq = q >> 1, sh = (uint32_t)__builtin_ctz(hq), total = rows << sh;
    const size_t qq = (size_t)q * q;
    for (uint32_t v = (uint32_t)lane_id(); v < total; v += 64) {
        const uint32_t r = row0 + (v >> sh), cc = (v & (hq - 1)) * 2;
        const double *t = W + (size_t)r * q + cc;
        double *p11 = C + (size_t)r * ldc + cc, *p12 = p11 + q, *p21 = p11 + (size_t)q * ldc, *p22 = p21 + q;
        const double2 m2 = str_ld2(t + 8 * qq), m5 = str_ld2(t + 9 * qq), t1m = str_ld2(t + 10 * qq);
        const double2 c11 = str_ld2(p11), c12 = str_ld2(p12), c21 = str_ld2(p21), c22 = str_ld2(p22);
        const double2 t1 = t1m + m2, t2 = c22 + t1;
        const double2 n11 = c11 + m2, n12 = c12 + (m5 + t1), n22 = m5 + t2;
        const double2 n21 = make_double2((-c21.x) + t2.x, (-c21.y) + t2.y);
        str_store2<SC1>(p11, n11.x, n11.y);
        str_store2<SC1>(p12, n12.x, n12.y);
        str_store2<SC1>(p22, n22.x, n22.y);
        str_store2<SC1>(p21, n21.x, n21.y);
    }
}

// a size x size operand at element offset `off` with row width `ld` lies in the arena
__device__ __forceinline__ bool str_in(const StrCtx &c, uint32_t off, uint32_t ld, uint32_t rows, uint32_t cols) {
    return rows && cols <= ld && (unsigned long long)off + (unsigned long long)(rows - 1) * ld + cols <= c.total &&
           ((off | ld) & 1u) == 0;
}

template <bool SC1>
struct StrKind : TimedKind<StrKind<SC1>, StrCtx> {
    using Ctx = StrCtx;
    static constexpr bool kSc1Payload = false;  // doubles move by plain loads behind the worker's acquire
    // payload: MUL / FORK / POST {kind, C, ldc, A, lda, B, ldb, size, fin, level, path}
    //          TILE              {kind, C, ldc, A, lda, B, ldb, K, fin}: 64 x 64 of C, all offsets the tile's
    //          PRE               {kind, A, lda, B, ldb, W, q, row0, rows, f0}
    //          COMBINE           {kind, C, ldc, W, q, row0, rows, fin}
    __device__ static void bad(DynWave &w) {
        if (lane_id() == 0) dev_error(dyn_err(w.v), kErrBadTask);
    }
    __device__ static void body(const Ctx &c, DynWave &w, const uint32_t *pay, int &which) {
        const uint32_t kind = pay[0];
        const uint32_t lane = (uint32_t)lane_id();
        if (kind == kStrPre) {
            const uint32_t q = pay[6], row0 = pay[7], rows = pay[8];
            if (q < 8 || (q & (q - 1)) || !rows || row0 + rows > q || !str_in(c, pay[1], pay[2], 2 * q, 2 * q) ||
                !str_in(c, pay[3], pay[4], 2 * q, 2 * q) || !str_in(c, pay[5], q, 8 * q, q))
                return bad(w);
            str_pre<SC1>(c.m + pay[1], pay[2], c.m + pay[3], pay[4], c.m + pay[5], q, row0, rows);
            which = kCntPre;
            dyn_finish_check_out<SC1>(w, pay[9]);
            return;
        }
        if (kind == kStrCombine) {
            const uint32_t q = pay[4], row0 = pay[5], rows = pay[6];
            if (q < 8 || (q & (q - 1)) || !rows || row0 + rows > q || !str_in(c, pay[1], pay[2], 2 * q, 2 * q) ||
                !str_in(c, pay[3], q, 11 * q, q))
                return bad(w);
            str_combine<SC1>(c.m + pay[1], pay[2], c.m + pay[3], q, row0, rows);
            which = kCntCombine;
            dyn_finish_check_out<SC1>(w, pay[7]);
            return;
        }
        if (kind > kStrTileTask) return bad(w);
        const uint32_t C = pay[1], ldc = pay[2], A = pay[3], lda = pay[4], B = pay[5], ldb = pay[6], size = pay[7];
        const uint32_t level = pay[9], path = pay[10];
        if (kind == kStrTileTask) {
            if (size < kStrTile || size % kStrKc || !str_in(c, C, ldc, kStrTile, kStrTile) ||
                !str_in(c, A, lda, kStrTile, size) || !str_in(c, B, ldb, size, kStrTile))
                return bad(w);
        } else if (size < 16 || (size & (size - 1)) || level >= (uint32_t)kStrMaxLevels ||
                   !str_in(c, C, ldc, size, size) || !str_in(c, A, lda, size, size) || !str_in(c, B, ldb, size, size)) {
            return bad(w);
        }
        const uint32_t q = size / 2;
        const uint32_t nb = (q + c.band_rows - 1) / c.band_rows;
        const unsigned long long ws64 = c.region[level < (uint32_t)kStrMaxLevels ? level : 0] +
                                        (unsigned long long)path * 11ull * q * q;
        if (kind == kStrMul || kind == kStrTileTask) {
            // the root has no scope yet: it opens the program's outer finish, checked in once, for itself
            const uint32_t fin = kind == kStrMul && pay[8] == kDynOpen ? dyn_finish_open(w, 1) : pay[8];
            if (kind == kStrTileTask || (size <= c.cutoff && size <= kStrTile)) {
                // one wave's product: a base of 16, 32 or 64, or a tile of a larger base over its whole k range
                which = kind == kStrTileTask ? kCntTile : kCntBase;
                if (size == 16) str_mul<16, SC1>(c.m + C, ldc, c.m + A, lda, c.m + B, ldb, size);
                else if (size == 32) str_mul<32, SC1>(c.m + C, ldc, c.m + A, lda, c.m + B, ldb, size);
                else str_mul<64, SC1>(c.m + C, ldc, c.m + A, lda, c.m + B, ldb, size);
                dyn_finish_check_out<SC1>(w, fin);
                return;
            }
            if (size <= c.cutoff) {
                // a base larger than a tile: its check-in passes to one tile, the others are checked in here
                which = kCntBase;
                const uint32_t nt = size / kStrTile, tiles = nt * nt;
                dyn_finish_check_in(w, fin, tiles - 1);
                for (uint32_t t0 = 0; t0 < tiles; t0 += 64) {
                    const uint32_t t = t0 + lane, ti = t / nt, tj = t % nt;
                    const uint32_t pl[kStrWords] = {kStrTileTask, C + ti * kStrTile * ldc + tj * kStrTile, ldc,
                                                    A + ti * kStrTile * lda, lda, B + tj * kStrTile, ldb, size, fin,
                                                    0, 0, 0};
                    dyn_async_await<true>(w, t < tiles, pl, nullptr, 0);
                }
                return;
            }
            if (ws64 + 11ull * q * q > c.total) return bad(w);
            which = kCntSplit;
            const uint32_t ws = (uint32_t)ws64;
            const uint32_t f0 = dyn_finish_open(w, nb);
            for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
                const uint32_t b = b0 + lane, row0 = b * c.band_rows;
                const uint32_t rows = row0 + c.band_rows <= q ? c.band_rows : q - row0;
                const uint32_t pl[kStrWords] = {kStrPre, A, lda, B, ldb, ws, q, row0, rows, f0, 0, 0};
                dyn_async_await<true>(w, b < nb, pl, nullptr, 0);
            }
            const uint32_t pl[kStrWords] = {kStrFork, C, ldc, A, lda, B, ldb, size, fin, level, path, 0};
            const uint32_t fut[1] = {f0};
            dyn_async_await<true>(w, lane == 0, pl, fut, 1);
            return;
        }
        if (ws64 + 11ull * q * q > c.total) return bad(w);
        const uint32_t ws = (uint32_t)ws64, fin = pay[8];
        const uint32_t qq = q * q;  // (q <= 8192 and the arena below 2^32 elements: no overflow where it is used)
        if (kind == kStrFork) {
            which = kCntFork;
            const uint32_t f1 = dyn_finish_open(w, 7);
            // lanes 0-6: the seven products in the reference's order; lane 7: the continuation, awaiting f1
            // M2 = A11 B11, M5 = S1 S5, T1sMULT = S2 S6, C22 = S3 S7, C11 = A12 B21, C12 = S4 B22, C21 = A22 S8
            // (temporary k of the call is at ws + k q^2: S1 .. S8 are 0 .. 7, M2, M5, T1sMULT 8 .. 10)
            uint32_t cc = ws + 8 * qq, cl = q, aa = A, al = lda, bb = B, bl = ldb;
            if (lane == 1) cc = ws + 9 * qq, aa = ws, al = q, bb = ws + 4 * qq, bl = q;
            else if (lane == 2) cc = ws + 10 * qq, aa = ws + qq, al = q, bb = ws + 5 * qq, bl = q;
            else if (lane == 3) cc = C + q * ldc + q, cl = ldc, aa = ws + 2 * qq, al = q, bb = ws + 6 * qq, bl = q;
            else if (lane == 4) cc = C, cl = ldc, aa = A + q, bb = B + q * ldb;
            else if (lane == 5) cc = C + q, cl = ldc, aa = ws + 3 * qq, al = q, bb = B + q * ldb + q;
            else if (lane == 6) cc = C + q * ldc, cl = ldc, aa = A + q * lda + q, bb = ws + 7 * qq, bl = q;
            uint32_t pl[kStrWords] = {kStrMul, cc, cl, aa, al, bb, bl, q, f1, level + 1, path * 7 + lane, 0};
            uint32_t fut[1] = {kDynOpen};
            if (lane == 7) {
                pl[0] = kStrPost, pl[1] = C, pl[2] = ldc, pl[3] = A, pl[4] = lda, pl[5] = B, pl[6] = ldb, pl[7] = size;
                pl[8] = fin, pl[9] = level, pl[10] = path;
                fut[0] = f1;
            }
            dyn_async_await<true>(w, lane < 8, pl, fut, 1);
            return;
        }
        // POST
        which = kCntPost;
        dyn_finish_check_in(w, fin, nb);
        for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
            const uint32_t b = b0 + lane, row0 = b * c.band_rows;
            const uint32_t rows = row0 + c.band_rows <= q ? c.band_rows : q - row0;
            const uint32_t pl[kStrWords] = {kStrCombine, C, ldc, ws, q, row0, rows, fin, 0, 0, 0, 0};
            dyn_async_await<true>(w, b < nb, pl, nullptr, 0);
        }
        dyn_finish_check_out<true>(w, fin);
    }
};

// two waves per SIMD, eight per CU: 256 registers each
template <bool SC1>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_strassen(StrCtx c, DynView v) {
    run_dyn_worker<StrKind<SC1>>(c, v);
}

ClassCounters<kCntKinds> g_str;  // the last launch's

// The call tree is a function of (n, cutoff, band_rows) alone: every count is exact.
struct StrPlan {
    unsigned long long splits = 0, bases = 0, tiles = 0, bands = 0, tasks = 0, scopes = 0, nodes = 0, check_ins = 0;
    unsigned long long ws = 0;  // elements of the temporaries
    unsigned long long region[kStrMaxLevels] = {};
    int levels = 0;
};

// the 64 x 64 (or smaller) products of the tree: bases, or the tiles of bases larger than a tile
unsigned long long str_leaves(int n, int cutoff) {
    unsigned long long size = (unsigned long long)n, calls = 1;
    for (; size > (unsigned long long)cutoff; size /= 2) calls *= 7;
    return size > kStrTile ? calls * (size / kStrTile) * (size / kStrTile) : calls;
}

int str_waves_per_cu(int n, int cutoff) {
    const unsigned long long leaves = str_leaves(n, cutoff);
    return leaves >= kStrBigTree ? kStrWavesPerCu : (leaves >= kStrSmallTree ? 2 : 1);
}

int str_check_args(const char *who, bool ptrs_ok, int n, int &cutoff, int &band_rows) {
    if (!ptrs_ok) {
        set_error("%s: a, b, c (and out) must not be NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    if (n < 16 || n > kStrMaxN || (n & (n - 1))) {
        set_error("%s: n = %d must be a power of two in 16 .. %d", who, n, kStrMaxN);
        return HCLIB_HIP_EINVAL;
    }
    if (cutoff == 0) cutoff = 64;  // app-desc.h BOTS_APP_DEF_ARG_CUTOFF
    if (cutoff < 16) {  // the naive kernels step 8 columns on an 8 x 8 quadrant at the least
        set_error("%s: cutoff = %d must be 0 (64) or at least 16", who, cutoff);
        return HCLIB_HIP_EINVAL;
    }
    if (band_rows < 0) {
        set_error("%s: band_rows = %d must not be negative", who, band_rows);
        return HCLIB_HIP_EINVAL;
    }
    if (band_rows == 0) band_rows = str_leaves(n, cutoff) >= kStrBigTree ? kStrBandBig : kStrBandSmall;
    return HCLIB_HIP_OK;
}

StrPlan str_plan(int n, int cutoff, int band_rows) {
    StrPlan p;
    unsigned long long size = (unsigned long long)n, calls = 1;
    while (size > (unsigned long long)cutoff) {
        const unsigned long long q = size / 2, nb = (q + band_rows - 1) / band_rows;
        p.splits += calls;
        p.bands += calls * nb;
        p.region[p.levels++] = 3ull * n * n + p.ws;
        p.ws += calls * 11 * q * q;
        calls *= 7;
        size = q;
    }
    p.bases = calls;
    const unsigned long long nt = size / kStrTile;
    p.tiles = size > kStrTile ? calls * nt * nt : 0;
    p.check_ins = p.bands + (size > kStrTile ? calls * (nt * nt - 1) : 0);
    p.tasks = p.splits + p.bases + p.tiles + 2 * p.bands + 2 * p.splits;  // MUL, TILE, PRE + COMBINE, FORK + POST
    p.scopes = 1 + 2 * p.splits;  // the outer finish, f0 and f1 of every split
    p.nodes = 2 * p.splits;       // FORK awaiting f0, POST awaiting f1
    return p;
}

int str_plan_checked(const char *who, int n, int cutoff, int band_rows, StrPlan &p) {
    p = str_plan(n, cutoff, band_rows);
    if (3ull * n * n + p.ws >= (1ull << 32) || p.tasks >= 0xfffffff0ull) {
        set_error("%s: n = %d at cutoff = %d, band_rows = %d needs %llu tasks (at most 2^32 - 17) and an arena of %llu "
                  "doubles (task payloads hold 32-bit element offsets): use a larger cutoff", who, n, cutoff, band_rows,
                  p.tasks, 3ull * n * n + p.ws);
        return HCLIB_HIP_EINVAL;
    }
    return HCLIB_HIP_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_strassen_bounds(int n, int cutoff, int band_rows, uint64_t out[4]) {
    HX_TRY(str_check_args("hclib_hip_strassen_bounds", out != nullptr, n, cutoff, band_rows));
    StrPlan p;
    HX_TRY(str_plan_checked("hclib_hip_strassen_bounds", n, cutoff, band_rows, p));
    out[0] = p.tasks;
    out[1] = p.scopes;
    out[2] = p.nodes;
    out[3] = p.ws * sizeof(double);
    return HCLIB_HIP_OK;
}

extern "C" void hclib_hip_strassen_last_ticks(uint64_t out[6]) {
    out[0] = g_str.ticks[kCntBase] + g_str.ticks[kCntTile];
    out[1] = g_str.ticks[kCntPre];
    out[2] = g_str.ticks[kCntCombine];
    out[3] = g_str.ticks[kCntSplit];
    out[4] = g_str.ticks[kCntFork];
    out[5] = g_str.ticks[kCntPost];
}

extern "C" int hclib_hip_strassen(const double *a, const double *b, double *c, int n, int cutoff, int band_rows,
                                  hclib_hip_strassen_result_t *result) {
    // argument errors first, before the device is touched
    HX_TRY(str_check_args("hclib_hip_strassen", a && b && c, n, cutoff, band_rows));
    StrPlan p;
    HX_TRY(str_plan_checked("hclib_hip_strassen", n, cutoff, band_rows, p));
    HX_TRY(ensure_device());
    Module &m = mod();

    // [counts: a line per task class][A][B][C][the temporaries, a region per level]
    const size_t hdr = g_str.kBytes, nn = (size_t)n * n, mbytes = nn * sizeof(double);
    const size_t bytes = hdr + (3 * nn + (size_t)p.ws) * sizeof(double);
    char *d = nullptr;
    if (const int rc = arena_reserve(kArenaStrassen, bytes, "hclib_hip_strassen", (void **)&d)) {
        set_error("hclib_hip_strassen: hipMalloc(%zu) failed (n = %d, cutoff = %d: %llu bytes of temporaries)", bytes, n,
                  cutoff, p.ws * 8ull);
        return rc;
    }
    // (`a` and `b` outlive the copies: launch_dyn synchronises the stream)
    HX_HIP(hipMemcpyAsync(d + hdr, a, mbytes, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(d + hdr + mbytes, b, mbytes, hipMemcpyHostToDevice, m.stream));

    StrCtx cx;
    cx.m = (double *)(d + hdr);
    cx.counts = (unsigned long long *)d;
    cx.total = 3ull * nn + p.ws;
    for (int l = 0; l < kStrMaxLevels; ++l) cx.region[l] = p.region[l];
    cx.cutoff = (uint32_t)cutoff;
    cx.band_rows = (uint32_t)band_rows;
    // (HCLIB_HIP_STRASSEN_SC1=0: plain stores and a release fence per check-out)
    const bool sc1 = env_int("HCLIB_HIP_STRASSEN_SC1", 1) != 0;
    const uint32_t un = (uint32_t)n;
    const uint32_t root[kStrWords] = {kStrMul, 2u * un * un, un, 0u, un, un * un, un, un, kDynOpen, 0u, 0u, 0u};
    // (HCLIB_HIP_STRASSEN_WAVES_PER_CU: for measurements)
    int wpc = env_int("HCLIB_HIP_STRASSEN_WAVES_PER_CU", str_waves_per_cu(n, cutoff));
    wpc = wpc < 1 ? 1 : (wpc > kStrWavesPerCu ? kStrWavesPerCu : wpc);
    hclib_hip_dyn_stats_t st{};
    uint64_t fin[2] = {0, 0};
    const int rc = launch_dyn(kStrWords, root, p.tasks, p.scopes, p.nodes ? p.nodes : 1, wpc, "hclib_hip_strassen", d,
                              g_str, &st, fin, [&](int grid, const DynView &v) {
                                  if (sc1) hipLaunchKernelGGL(k_strassen<true>, dim3(grid), dim3(64), 0, m.stream, cx, v);
                                  else hipLaunchKernelGGL(k_strassen<false>, dim3(grid), dim3(64), 0, m.stream, cx, v);
                              });
    if (result) {
        result->tasks = st.tasks;
        result->splits = g_str.tasks[kCntSplit];
        result->base = g_str.tasks[kCntBase];
        result->tiles = g_str.tasks[kCntTile];
        result->pre_bands = g_str.tasks[kCntPre];
        result->combine_bands = g_str.tasks[kCntCombine];
        result->finishes = fin[0];
        result->check_ins = fin[1];
        result->workspace_bytes = p.ws * sizeof(double);
        result->kernel_ms = st.kernel_ms;
        result->gflops = st.kernel_ms > 0 ? 2.0 * n * (double)n * n / (st.kernel_ms * 1e6) : 0.0;
    }
    if (rc) return rc;
    HX_HIP(hipMemcpy(c, cx.m + 2 * nn, mbytes, hipMemcpyDeviceToHost));
    return HCLIB_HIP_OK;
}
