// alignment.hip — BOTS alignment (test/performance-regression/full-apps/bots/
// alignment_for and alignment_single: alignment.ref.c the algorithm,
// alignment.c the HClib port, whose hclib_start_finish holds one hclib_async
// per sequence pair) as a client of dynamic device dataflow
// (include/hclib_hip/hx_dyn.h): all pairs of a Pearson file aligned by
// Myers-Miller in ONE launch of run_dyn_worker, every score and every
// intermediate of a pair the reference's, integer for integer. The two BOTS
// programs differ only in which host loop creates the pair tasks; on the
// device both are this program.
//
//   task                     does (alignment.ref.c lines)
//   ROOT                     a PAIR task per entry of the pair table the host
//                            uploaded (si, sj, g, gh; pairs with an empty
//                            sequence are not in it), 64 per dyn_async_await
//   PAIR(p)                  forward_pass (:204-241) and reverse_pass
//                            (:246-286), maxscore, se1, se2, sb1, sb2 into
//                            the pair's record, then the pair's root diff
//                            (:510) as below
//   DIFF(p, A, B, M, N,      diff (:291-417). A base case (N <= 0, M <= 0,
//        tb, te)             M == 1) is counted and done. Otherwise the two
//                            half sweeps and the midpoint (:330-399); with
//                            M * N <= cutoff the two halves go on a stack in
//                            LDS and this wave runs the whole recursion below,
//                            else they become two DIFF tasks (two active
//                            lanes, no futures)
// No finish scopes and no promises: the launch ends when `live` reaches 0.
// displ is not built. The score needs only the count of its zeros whose two
// residues are equal; a zero comes only from the M == 1 base case with
// midj > 0, and it stands for seq1[A + 1] against seq2[B + midj], A and B the
// call's own arguments. So the count is a sum over base cases in any order,
// and every task ends by adding its counts (matches, diff calls, type-2
// midpoints, tie-branch takes) to the pair's record with agent-scope atomics
// (DESIGN.md §18).
//
// A sweep is wave-wide and is the serial recurrence verbatim. Strips of 64
// rows, lane l on row base + l, skewed: at step t lane l is at column
// t - l + 1. hh and the horizontal gap state f stay in the lane's registers;
// HH and DD of the row above, and the residue code of the column, come from
// lane l - 1 by a DPP wave shift; lane 0 takes them from a 64-column chunk the
// wave loaded at once, every 64 steps, (the row buffer of the strip above, or the boundary
// formula in the first strip) by v_readlane. The strip's bottom lane stores
// the row buffer the next strip reads: it is 63 columns behind lane 0, so the
// buffer is updated in place. One routine serves the four sweeps (forward and
// reverse pass, the two halves of diff): they differ in the boundary values,
// the direction the sequences are read in, the clamp at 0 and what is tracked.
//
// Memory: the matrix (4 KB) and the stack in LDS; the row arrays HH, DD, RR,
// SS in LDS while the longest sequence has at most kAlLdsCols residues, else
// in this wave's slice of the arena; each task owns them from start to end.
// The only words two waves share are payloads (dyn_async_await) and the pair
// records (atomics; the five words of the passes are written by the one PAIR
// task and read by the host).
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "hx_align_host.h"
#include "hx_client.h"

namespace hx {
namespace {

constexpr int kAlWords = 6;  // payload: {kind | tb != 0 << 8 | te != 0 << 9, pair, A, B, M, N}
constexpr int kAlMaxWavesPerCu = 8;
constexpr int kAlStack = 40;  // records of six words: depth <= ceil(log2 4999) + 1 = 14, two pushed per pop
enum : uint32_t { kAlRoot = 0, kAlPair = 1, kAlDiff = 2 };
enum : int { kCntRoot = 0, kCntPair = 1, kCntSpawn = 2, kCntLeaf = 3 };
// a pair's record
enum : int { kRMax = 0, kRSe1 = 1, kRSe2 = 2, kRSb1 = 3, kRSb2 = 4, kRMatches = 5, kRDiffs = 6, kRType2 = 7, kRTies = 8 };
enum : int { kSwDiff = 0, kSwFwd = 1, kSwRev = 2 };
constexpr int kIntMin = -2147483647 - 1;
typedef __attribute__((address_space(3))) int32_t al_lds_i32;
typedef __attribute__((address_space(1))) int32_t al_glb_i32;

struct AlCtx {
    const int32_t *matrix;   // 32 x 32
    const uint32_t *seqtab;  // per sequence {offset into codes, length}
    const int32_t *pairtab;  // per pair {si, sj, g, gh}
    int32_t *rec;            // per pair kAlRecWords
    const uint8_t *codes;
    int32_t *rows;           // waves x 4 x rowlen, or null: the row arrays are in LDS
    unsigned long long *counts;  // per task class (hx_client.h class_count)
    uint32_t nseqs, npairs, rowlen, waves;
    int32_t cutoff;
};

__device__ __forceinline__ int32_t *al_lds_matrix() {
    __shared__ int32_t s[kAlCodes * kAlCodes];
    return s;
}
__device__ __forceinline__ int32_t *al_lds_rows() {
    __shared__ int32_t s[4 * (kAlLdsCols + 1)];
    return s;
}
__device__ __forceinline__ int32_t *al_lds_stack() {
    __shared__ int32_t s[kAlStack * 6];
    return s;
}

// lane l takes lane l - 1's x, lane 0 takes 0 (DPP wave_shr:1)
__device__ __forceinline__ int al_from_above(int x) {
    return __builtin_amdgcn_update_dpp(0, x, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ int al_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ int al_max(int a, int b) { return a > b ? a : b; }

// One sweep over logical rows 1..R and columns 1..C: row i is residue
// a[a0 + da * i], column j is b[b0 + da * j] (a and b such that x[k] is the
// reference's seq[k], k from 1). H[0][0] = 0; H[0][k] = H[k][0] = edge0 -
// k * egh for k >= 1; D[0][k] = H[0][k] - dgap and f starts at H[i][0] - dgap.
struct AlSweep {
    const uint8_t *a, *b;
    int a0, b0, da, R, C, edge0, egh, dgap, g, gh, target;
};
// kSwFwd and kSwRev: the first cell in row-major order with the largest value
// above 0 (bv, bi, bj). kSwRev: the first cell in that order whose value
// reaches target (found, fi, fj); the sweep stops after the strip that has it.
struct AlTrack {
    int bv = 0, bi = 0, bj = 0, found = 0, fi = 0, fj = 0;
};

// what one wave's stores to the row arrays mean to its other lanes' loads
__device__ __forceinline__ void al_rows_visible() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int MODE, class T>
__device__ __forceinline__ void al_sweep(const int32_t *mat, T *bh, T *bd, const AlSweep &s, AlTrack &tr) {
    const int lane = lane_id();
    const int ggh = s.g + s.gh;
    int bv = 0, bi = 0, bj = 0, found = 0, fi = 0, fj = 0;
    for (int base = 0; base < s.R; base += 64) {
        const int lrows = s.R - base < 64 ? s.R - base : 64;
        const int i = base + lane + 1;
        const bool rowok = lane < lrows;
        const int ai = rowok ? (int)s.a[s.a0 + s.da * i] & 31 : 0;
        const int32_t *mrow = mat + ai * kAlCodes;
        int hh = s.edge0 - i * s.egh;                        // H[i][0]
        int f = hh - s.dgap;
        int diag = i == 1 ? 0 : s.edge0 - (i - 1) * s.egh;   // H[i - 1][0]
        int out_h = 0, out_e = 0, code = 0, chunk_h = 0, chunk_d = 0, chunk_b = 0;
        const int steps = s.C + lrows - 1;
        for (int t0 = 0; t0 < steps; t0 += 64) {
            // the next 64 columns of lane 0: codes, and the row above the strip (loaded here, outside the step
            // loop, so that no step waits for memory: the bottom lane's stores drain behind the steps)
            {
                const int jc = t0 + 1 + lane;
                const bool ok = jc <= s.C;
                chunk_b = ok ? (int)s.b[s.b0 + s.da * jc] & 31 : 0;
                if (base > 0) {
                    chunk_h = ok ? bh[jc] : 0;
                    chunk_d = ok ? bd[jc] : 0;
                } else {
                    chunk_h = s.edge0 - jc * s.egh;
                    chunk_d = chunk_h - s.dgap;
                }
            }
            const int kend = steps - t0 < 64 ? steps - t0 : 64;
            for (int k = 0; k < kend; ++k) {
                int up_h = al_from_above(out_h), up_d = al_from_above(out_e), bc = al_from_above(code);
                const int h0 = __builtin_amdgcn_readlane(chunk_h, k), d0 = __builtin_amdgcn_readlane(chunk_d, k),
                          c0 = __builtin_amdgcn_readlane(chunk_b, k);
                if (lane == 0) up_h = h0, up_d = d0, bc = c0;
                code = bc;
                const int j = t0 + k - lane + 1;
                if (rowok && j >= 1 && j <= s.C) {
                    f = al_max(f - s.gh, hh - ggh);
                    const int e = al_max(up_d - s.gh, up_h - ggh);
                    int v = diag + mrow[bc & 31];
                    v = al_max(v, f);
                    v = al_max(v, e);
                    if (MODE == kSwFwd) v = al_max(v, 0);
                    hh = v;
                    diag = up_h;
                    out_h = v;
                    out_e = e;
                    if (MODE != kSwDiff && v > bv) bv = v, bi = i, bj = j;
                    if (MODE == kSwRev && !found && v >= s.target) found = 1, fi = i, fj = j;
                    if (lane == lrows - 1) {
                        bh[j] = v;
                        bd[j] = e;
                    }
                }
            }
        }
        al_rows_visible();  // the bottom lane's row, before the next strip's lanes load it
        if (MODE == kSwRev && __ballot(found != 0)) break;
    }
    if (MODE == kSwDiff) return;
    if (MODE == kSwRev) {
        const unsigned long long mf = __ballot(found != 0);
        tr.found = mf != 0;
        if (mf) {
            // one strip has it: its rows ascend with the lane
            const int l = __builtin_ctzll(mf);
            tr.fi = __builtin_amdgcn_readlane(fi, l);
            tr.fj = __builtin_amdgcn_readlane(fj, l);
        }
    }
    // the largest value, then the smallest row; a lane's rows and columns ascend, so it holds its first
    const unsigned long long key = ((unsigned long long)(uint32_t)bv << 32) | (uint32_t)(0x7fffffff - bi);
    const unsigned long long top = wave_max(key);
    const int l = __builtin_ctzll(__ballot(key == top));
    tr.bv = __builtin_amdgcn_readlane(bv, l);
    tr.bi = __builtin_amdgcn_readlane(bi, l);
    tr.bj = __builtin_amdgcn_readlane(bj, l);
}

struct AlCounts {
    int matches = 0, diffs = 0, type2 = 0, ties = 0;
};

// the M == 1 base case (:307-316): midj, the first j that beats both all-gap forms, or 0
__device__ __forceinline__ int al_base(const int32_t *mat, const uint8_t *s1, const uint8_t *s2, int A, int B, int N,
                                       int tb, int te, int gh) {
    const int lane = lane_id();
    const int tegN = te + gh * N, tbgN = tb + gh * N;  // (N >= 1)
    const int init = al_max(-(tb + gh) - tegN, -(te + gh) - tbgN);
    const int32_t *mrow = mat + ((int)s1[A + 1] & 31) * kAlCodes;
    int bv = kIntMin, bj = 0;
    for (int j = 1 + lane; j <= N; j += 64) {
        const int v = mrow[(int)s2[B + j] & 31] - (N - j <= 0 ? 0 : te + gh * (N - j)) - (j - 1 <= 0 ? 0 : tb + gh * (j - 1));
        if (v > bv) bv = v, bj = j;
    }
    const unsigned long long key = ((unsigned long long)((uint32_t)bv ^ 0x80000000u) << 32) | (uint32_t)(0x7fffffff - bj);
    const unsigned long long top = wave_max(key);
    const int l = __builtin_ctzll(__ballot(key == top));
    const int v = __builtin_amdgcn_readlane(bv, l), j = __builtin_amdgcn_readlane(bj, l);
    return v > init ? j : 0;
}

// the midpoint of a diff that is no base case (:330-399): midi = M / 2, and (midj, type)
template <class T>
__device__ __forceinline__ void al_midpoint(const int32_t *mat, T *rows, uint32_t rowlen, const uint8_t *s1,
                                            const uint8_t *s2, int A, int B, int M, int N, int tb, int te, int g, int gh,
                                            int &midj, int &type, AlCounts &cn) {
    const int lane = lane_id();
    const int midi = M / 2;
    T *bh = rows, *bd = rows + rowlen, *br = rows + 2 * rowlen, *bs = rows + 3 * rowlen;
    AlTrack tr;
    // HH, DD: rows 1 .. midi forward; RR[j], SS[j] = br, bs[N - j]: rows M .. midi + 1 and the columns backward
    const AlSweep fw = {s1, s2, A, B, 1, midi, N, -tb, gh, g, g, gh, 0};
    al_sweep<kSwDiff>(mat, bh, bd, fw, tr);
    const AlSweep bw = {s1, s2, A + M + 1, B + N + 1, -1, M - midi, N, -te, gh, g, g, gh, 0};
    al_sweep<kSwDiff>(mat, br, bs, bw, tr);
    if (lane == 0) {
        bh[0] = bd[0] = -tb - midi * gh;        // HH[0], DD[0] = HH[0] (:343, :358)
        br[0] = bs[0] = -te - (M - midi) * gh;  // RR[N], SS[N] = RR[N] (:368, :383)
    }
    al_rows_visible();
    // pass 1: the largest HH[j] + RR[j] and DD[j] + SS[j] + g, and the tie-branch takes: a j whose sum equals
    // the running midh (the largest sum before it, the sum of j = 0 at j = 0) and has HH != DD && RR == SS
    int carry = kIntMin, mx2 = kIntMin, ties = 0;
    for (int j0 = 0; j0 <= N; j0 += 64) {
        const int j = j0 + lane;
        const bool ok = j <= N;
        const int h = ok ? bh[j] : 0, d = ok ? bd[j] : 0, r = ok ? br[N - j] : 0, ss = ok ? bs[N - j] : 0;
        const int sum = ok ? h + r : kIntMin;
        int inc = wave_incl_max_scan(sum);
        inc = al_max(inc, carry);
        int ex = al_from_above(inc);
        if (lane == 0) ex = j0 == 0 ? sum : carry;
        ties += __popcll(__ballot(ok && sum == ex && h != d && r == ss));
        carry = __builtin_amdgcn_readlane(inc, 63);
        if (ok) mx2 = al_max(mx2, d + ss + g);
    }
    const int mx = carry;
    mx2 = wave_max(mx2);
    // pass 2: the first j with the largest sum, the last one with it and the condition, the last j of type 2
    int first = 0x7fffffff, lastc = -1, last2 = -1;
    for (int j0 = 0; j0 <= N; j0 += 64) {
        const int j = j0 + lane;
        if (j > N) continue;
        const int h = bh[j], d = bd[j], r = br[N - j], ss = bs[N - j];
        if (h + r == mx) {
            if (j < first) first = j;
            if (h != d && r == ss) lastc = j;
        }
        if (d + ss + g == mx2) last2 = j;
    }
    first = -wave_max(-first);
    lastc = wave_max(lastc);
    last2 = wave_max(last2);
    type = 1;
    midj = lastc >= 0 ? lastc : first;
    if (mx2 > mx) type = 2, midj = last2;
    cn.ties += ties;
    cn.type2 += type == 2 ? 1 : 0;
    al_rows_visible();  // (the next sweep overwrites what other lanes just read)
}

// diff(A, B, M, N, tb, te) and everything below it that this task runs; true when it spawned its halves
template <class T>
__device__ __forceinline__ bool al_diff(const AlCtx &c, DynWave &w, const int32_t *mat, T *rows, uint32_t pair,
                                        const uint8_t *s1, const uint8_t *s2, int A, int B, int M, int N, int tb, int te,
                                        int g, int gh, AlCounts &cn) {
    const int lane = lane_id();
    int32_t *stack = al_lds_stack();
    int sp = 0;
    bool spawned = false;
    while (true) {
        cn.diffs += 1;
        if (N > 0 && M == 1) {
            const int midj = al_base(mat, s1, s2, A, B, N, tb, te, gh);
            if (midj > 0) {
                const int c1 = s1[A + 1], c2 = s2[B + midj];
                cn.matches += (c1 != kAlGap1 && c1 != kAlGap2 && c1 == c2) ? 1 : 0;
            }
        } else if (N > 0 && M > 1) {
            int midj, type;
            al_midpoint(mat, rows, c.rowlen, s1, s2, A, B, M, N, tb, te, g, gh, midj, type, cn);
            const int midi = M / 2;
            // (:402-409)
            const int k1[6] = {A, B, type == 1 ? midi : midi - 1, midj, tb, type == 1 ? g : 0};
            const int k2[6] = {type == 1 ? A + midi : A + midi + 1, B + midj, type == 1 ? M - midi : M - midi - 1, N - midj,
                               type == 1 ? g : 0, te};
            if ((long long)M * N > (long long)c.cutoff) {
                const bool second = lane == 1;
                const uint32_t ktb = second ? k2[4] : k1[4], kte = second ? k2[5] : k1[5];
                const uint32_t pl[kAlWords] = {kAlDiff | (ktb ? 1u << 8 : 0u) | (kte ? 1u << 9 : 0u), pair,
                                               (uint32_t)(second ? k2[0] : k1[0]), (uint32_t)(second ? k2[1] : k1[1]),
                                               (uint32_t)(second ? k2[2] : k1[2]), (uint32_t)(second ? k2[3] : k1[3])};
                dyn_async_await<true>(w, lane < 2, pl, nullptr, 0);  // (the halves read nothing this task wrote)
                spawned = true;
            } else if (sp + 2 > kAlStack) {
                if (lane == 0) dev_error(dyn_err(w.v), kErrStackOverflow);
                return spawned;
            } else {
                // the second half below the first: the first is popped first, as the reference calls it first
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) stack[sp * 6 + k] = k2[k], stack[(sp + 1) * 6 + k] = k1[k];
                }
                sp += 2;
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (sp == 0) return spawned;
        sp -= 1;
        A = al_uniform(stack[sp * 6]), B = al_uniform(stack[sp * 6 + 1]), M = al_uniform(stack[sp * 6 + 2]);
        N = al_uniform(stack[sp * 6 + 3]), tb = al_uniform(stack[sp * 6 + 4]), te = al_uniform(stack[sp * 6 + 5]);
        __builtin_amdgcn_wave_barrier();
    }
}

struct AlKind : TimedKind<AlKind, AlCtx> {
    using Ctx = AlCtx;
    static constexpr bool kSc1Payload = true;  // no task reads what another task wrote
    __device__ static void bad(DynWave &w) {
        if (lane_id() == 0) dev_error(dyn_err(w.v), kErrBadTask);
    }
    template <class T>
    __device__ __forceinline__ static void task(T *rows, const Ctx &c, DynWave &w, const uint32_t *pay, int &which,
                                                const uint8_t *s1, const uint8_t *s2, int n, int m, int g, int gh) {
        const uint32_t kind = pay[0] & 0xffu, pair = pay[1];
        const int lane = lane_id();
        const int32_t *mat = al_lds_matrix();
        int32_t *rec = c.rec + (size_t)pair * kAlRecWords;
        AlCounts cn;
        bool spawned;
        if (kind == kAlPair) {
            which = kCntPair;
            AlTrack tr;
            const AlSweep fw = {s1, s2, 0, 0, 1, n, m, 0, 0, g, g, gh, 0};
            al_sweep<kSwFwd>(mat, rows, rows + c.rowlen, fw, tr);
            const int maxscore = tr.bv, se1 = tr.bi, se2 = tr.bj;
            int sb1 = 1, sb2 = 1;
            if (maxscore > 0) {
                al_rows_visible();
                const AlSweep rv = {s1, s2, se1 + 1, se2 + 1, -1, se1, se2, -1, 0, 0, g, gh, maxscore};
                AlTrack rt;
                al_sweep<kSwRev>(mat, rows, rows + c.rowlen, rv, rt);
                // (:278-281: the cell that reaches maxscore, else the first cell with the largest value above 0)
                if (rt.found) sb1 = se1 + 1 - rt.fi, sb2 = se2 + 1 - rt.fj;
                else if (rt.bv > 0) sb1 = se1 + 1 - rt.bi, sb2 = se2 + 1 - rt.bj;
                al_rows_visible();
            }
            if (lane == 0) rec[kRMax] = maxscore, rec[kRSe1] = se1, rec[kRSe2] = se2, rec[kRSb1] = sb1, rec[kRSb2] = sb2;
            spawned = al_diff(c, w, mat, rows, pair, s1, s2, sb1 - 1, sb2 - 1, se1 - sb1 + 1, se2 - sb2 + 1, 0, 0, g, gh, cn);
        } else {
            const int A = (int)pay[2], B = (int)pay[3], M = (int)pay[4], N = (int)pay[5];
            if (A < 0 || B < 0 || M < 0 || N < 0 || A + M > n || B + N > m) return bad(w);
            spawned = al_diff(c, w, mat, rows, pair, s1, s2, A, B, M, N, (pay[0] >> 8 & 1u) ? g : 0,
                              (pay[0] >> 9 & 1u) ? g : 0, g, gh, cn);
            which = spawned ? kCntSpawn : kCntLeaf;
        }
        if (lane == 0) {
            if (cn.matches) add_agent(&rec[kRMatches], cn.matches);
            add_agent(&rec[kRDiffs], cn.diffs);
            if (cn.type2) add_agent(&rec[kRType2], cn.type2);
            if (cn.ties) add_agent(&rec[kRTies], cn.ties);
        }
    }
    __device__ static void body(const Ctx &c, DynWave &w, const uint32_t *pay, int &which) {
        const uint32_t kind = pay[0] & 0xffu, pair = pay[1];
        const int lane = lane_id();
        if (kind == kAlRoot) {
            which = kCntRoot;
            for (uint32_t p0 = 0; p0 < c.npairs; p0 += kAlPairsPerSpawn) {
                const uint32_t pl[kAlWords] = {kAlPair, p0 + (uint32_t)lane, 0u, 0u, 0u, 0u};
                dyn_async_await<true>(w, p0 + (uint32_t)lane < c.npairs, pl, nullptr, 0);
            }
            return;
        }
        if (kind > kAlDiff || pair >= c.npairs || blockIdx.x >= c.waves) return bad(w);
        const int32_t *pt = c.pairtab + (size_t)pair * 4;
        const uint32_t si = (uint32_t)al_uniform(pt[0]), sj = (uint32_t)al_uniform(pt[1]);
        const int g = al_uniform(pt[2]), gh = al_uniform(pt[3]);
        if (si >= c.nseqs || sj >= c.nseqs) return bad(w);
        const int n = al_uniform((int)c.seqtab[si * 2 + 1]), m = al_uniform((int)c.seqtab[sj * 2 + 1]);
        if (n < 1 || m < 1 || (uint32_t)m + 1 > c.rowlen) return bad(w);
        // s1[k], s2[k]: the reference's seq_array[..][k], k from 1
        const uint8_t *s1 = c.codes + al_uniform((int)c.seqtab[si * 2]) - 1;
        const uint8_t *s2 = c.codes + al_uniform((int)c.seqtab[sj * 2]) - 1;
        // the row arrays through pointers of their own address space: a generic pointer makes every access a FLAT
        // operation, whose store the sweep's next LDS load of the matrix then has to wait for (lgkmcnt)
        if (c.rows) task((al_glb_i32 *)(c.rows + (size_t)blockIdx.x * 4 * c.rowlen), c, w, pay, which, s1, s2, n, m, g, gh);
        else task((al_lds_i32 *)al_lds_rows(), c, w, pay, which, s1, s2, n, m, g, gh);
    }
};

__global__ __launch_bounds__(64) void k_alignment(AlCtx c, DynView v) {
    int32_t *mat = al_lds_matrix();
    for (int k = (int)threadIdx.x; k < kAlCodes * kAlCodes; k += 64) mat[k] = c.matrix[k];
    __syncthreads();
    run_dyn_worker<AlKind>(c, v);
}

ClassCounters<kAlClasses> g_al;  // the last launch's

int al_check_input(const char *who, const hclib_hip_alignment_input_t *in, std::vector<int> &len) {
    if (!in || in->nseqs < 1 || !in->length || !in->offset || (!in->codes && in->total > 0) || in->total < 0) {
        set_error("%s: input must not be NULL and must hold at least one sequence with its length, offset and codes", who);
        return HCLIB_HIP_EINVAL;
    }
    len.assign(in->length, in->length + in->nseqs);
    for (int i = 0; i < in->nseqs; ++i) {
        if (len[i] < 0 || len[i] > kAlMaxLen) {
            set_error("%s: sequence %d has %d residues; the reference's MAX_ALN_LENGTH arrays hold at most %d", who, i + 1,
                      len[i], kAlMaxLen);
            return HCLIB_HIP_EINVAL;
        }
        if (in->offset[i] < 0 || (long long)in->offset[i] + len[i] > in->total) {
            set_error("%s: sequence %d lies outside the %d codes", who, i + 1, in->total);
            return HCLIB_HIP_EINVAL;
        }
        for (int k = 0; k < len[i]; ++k)
            if (in->codes[in->offset[i] + k] >= kAlCodes) {
                set_error("%s: sequence %d has residue code %d (at most %d)", who, i + 1, in->codes[in->offset[i] + k],
                          kAlCodes - 1);
                return HCLIB_HIP_EINVAL;
            }
    }
    return HCLIB_HIP_OK;
}

int al_cutoff(const char *who, int cutoff, int &out) {
    if (cutoff < 0) {
        set_error("%s: cutoff = %d must be at least 1 cell, or 0 for the default %d", who, cutoff, kAlDefaultCutoff);
        return HCLIB_HIP_EINVAL;
    }
    out = cutoff ? cutoff : kAlDefaultCutoff;
    return HCLIB_HIP_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_alignment_read_input(const char *path, hclib_hip_alignment_input_t *out) {
    if (!path || !out) {
        set_error("hclib_hip_alignment_read_input: path and out must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    memset(out, 0, sizeof(*out));
    std::vector<AlSeq> seqs;
    std::string err;
    if (al_read_input(path, seqs, err)) {
        set_error("hclib_hip_alignment_read_input: %s", err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    size_t total = 0;
    for (const AlSeq &q : seqs) total += q.codes.size();
    const size_t ns = seqs.size();
    out->length = (int32_t *)calloc(ns, 4);
    out->offset = (int32_t *)calloc(ns, 4);
    out->codes = (uint8_t *)calloc(total + 1, 1);
    out->names = (char *)calloc(ns, kAlMaxName + 1);
    if (!out->length || !out->offset || !out->codes || !out->names) {
        hclib_hip_alignment_free_input(out);
        set_error("hclib_hip_alignment_read_input: out of host memory");
        return HCLIB_HIP_ENOMEM;
    }
    size_t at = 0;
    for (size_t i = 0; i < ns; ++i) {
        out->length[i] = (int32_t)seqs[i].codes.size();
        out->offset[i] = (int32_t)at;
        if (!seqs[i].codes.empty()) memcpy(out->codes + at, seqs[i].codes.data(), seqs[i].codes.size());
        memcpy(out->names + i * (kAlMaxName + 1), seqs[i].name.c_str(), seqs[i].name.size());
        at += seqs[i].codes.size();
    }
    out->nseqs = (int32_t)ns;
    out->total = (int32_t)total;
    return HCLIB_HIP_OK;
}

extern "C" void hclib_hip_alignment_free_input(hclib_hip_alignment_input_t *in) {
    if (!in) return;
    free(in->length), free(in->offset), free(in->codes), free(in->names);
    memset(in, 0, sizeof(*in));
}

extern "C" int hclib_hip_alignment_read_matrix(const char *path, hclib_hip_alignment_matrix_t *out) {
    if (!path || !out) {
        set_error("hclib_hip_alignment_read_matrix: path and out must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    AlMatrix m;
    std::string err;
    if (al_read_matrix(path, m, err)) {
        set_error("hclib_hip_alignment_read_matrix: %s", err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    out->avscore = m.avscore;
    memcpy(out->score, m.score, sizeof(m.score));
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_alignment_bounds(const hclib_hip_alignment_input_t *input, int cutoff, uint64_t out[6]) {
    if (!out) {
        set_error("hclib_hip_alignment_bounds: out must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    std::vector<int> len;
    int cut;
    HX_TRY(al_check_input("hclib_hip_alignment_bounds", input, len));
    HX_TRY(al_cutoff("hclib_hip_alignment_bounds", cutoff, cut));
    AlBounds b;
    std::string err;
    if (al_bounds(len.data(), (int)len.size(), cut, kAlMaxWaves, b, err)) {
        set_error("hclib_hip_alignment_bounds: %s", err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    out[0] = b.pairs, out[1] = b.tasks, out[2] = b.spawns, out[3] = b.diffs, out[4] = b.arena_bytes, out[5] = b.row_bytes;
    return HCLIB_HIP_OK;
}

extern "C" void hclib_hip_alignment_last_ticks(uint64_t out[4]) {
    for (int k = 0; k < kAlClasses; ++k) out[k] = g_al.ticks[k];
}

extern "C" int hclib_hip_alignment(const hclib_hip_alignment_input_t *input, const hclib_hip_alignment_matrix_t *matrix,
                                   int cutoff, hclib_hip_alignment_result_t *result, hclib_hip_alignment_pair_t *pairs) {
    const char *who = "hclib_hip_alignment";
    // argument errors first, before the device is touched
    if (!matrix || !result || !result->scores) {
        set_error("%s: matrix, result and result->scores must not be NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    std::vector<int> len;
    int cut;
    HX_TRY(al_check_input(who, input, len));
    HX_TRY(al_cutoff(who, cutoff, cut));
    const int ns = input->nseqs;
    AlBounds b;
    std::string err;
    if (al_bounds(len.data(), ns, cut, 1, b, err)) {
        set_error("%s: %s", who, err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    HX_TRY(ensure_device());
    Module &m = mod();
    // (HCLIB_HIP_ALIGNMENT_WAVES_PER_CU: for measurements)
    int wpc = env_int("HCLIB_HIP_ALIGNMENT_WAVES_PER_CU", 4);
    wpc = wpc < 1 ? 1 : (wpc > kAlMaxWavesPerCu ? kAlMaxWavesPerCu : wpc);
    const long long waves = (long long)m.num_cus * wpc;
    if (waves > kAlMaxWaves || al_bounds(len.data(), ns, cut, (int)waves, b, err)) {
        set_error("%s: %lld resident waves, the bounds allow %d", who, waves, kAlMaxWaves);
        return HCLIB_HIP_EINVAL;
    }
    const size_t P = (size_t)b.pairs, total = (size_t)input->total;

    // the pair table in the reference's (si, sj) order, and the scores that need no task (:478-479)
    std::vector<int32_t> pt(P * 4 + 4), lens(ns);
    std::vector<uint32_t> seqtab((size_t)ns * 2);
    int32_t *scores = result->scores;
    int kernel_cutoff = cut;
    memset(scores, 0, (size_t)ns * ns * sizeof(int32_t));
    for (int i = 0; i < ns; ++i) {
        seqtab[(size_t)i * 2] = (uint32_t)input->offset[i], seqtab[(size_t)i * 2 + 1] = (uint32_t)len[i];
        lens[i] = al_len(input->codes + input->offset[i], len[i]);
    }
    size_t np = 0;
    for (int i = 0; i < ns; ++i)
        for (int j = i + 1; j < ns; ++j) {
            if (len[i] == 0 || len[j] == 0) {
                scores[(size_t)i * ns + j] = 1;
                continue;
            }
            int g, gh;
            al_gaps(len[i], len[j], matrix->avscore, g, gh);
            pt[np * 4] = i, pt[np * 4 + 1] = j, pt[np * 4 + 2] = g, pt[np * 4 + 3] = gh;
            ++np;
        }
    for (size_t p = 0; p < np; ++p)
        if (pt[p * 4 + 2] < 0 || pt[p * 4 + 3] < 0) {
            set_error("%s: avscore = %d gives a negative gap penalty", who, matrix->avscore);
            return HCLIB_HIP_EINVAL;
        }

    memset(result, 0, sizeof(*result));
    result->scores = scores;
    result->pairs = P;
    result->cutoff = kernel_cutoff;
    result->cells = b.cells;
    if (P == 0) {
        g_al = ClassCounters<kAlClasses>();
        return HCLIB_HIP_OK;
    }

    // [counts: a line per task class][matrix][seqtab][pair table][records][codes][row slices]
    char *d = nullptr;
    if (const int rc = arena_reserve(kArenaAlignment, (size_t)b.arena_bytes, who, (void **)&d)) {
        set_error("%s: hipMalloc(%llu) failed (%zu pairs, longest sequence %d)", who, b.arena_bytes, P, b.longest);
        return rc;
    }
    const size_t o_mat = g_al.kBytes, o_seq = o_mat + sizeof(matrix->score);
    const size_t o_pt = o_seq + (((size_t)ns * 8 + 255) & ~(size_t)255);
    const size_t o_rec = o_pt + ((P * 16 + 255) & ~(size_t)255);
    const size_t o_codes = o_rec + P * kAlRecWords * 4;
    const size_t o_rows = o_codes + ((total + 64 + 255) & ~(size_t)255);
    AlCtx cx;
    cx.counts = (unsigned long long *)d;
    cx.matrix = (const int32_t *)(d + o_mat);
    cx.seqtab = (const uint32_t *)(d + o_seq);
    cx.pairtab = (const int32_t *)(d + o_pt);
    cx.rec = (int32_t *)(d + o_rec);
    cx.codes = (const uint8_t *)(d + o_codes);
    cx.rows = b.row_bytes ? (int32_t *)(d + o_rows) : nullptr;
    cx.nseqs = (uint32_t)ns, cx.npairs = (uint32_t)P, cx.waves = (uint32_t)waves;
    cx.rowlen = b.row_bytes ? (uint32_t)b.longest + 1 : (uint32_t)kAlLdsCols + 1;
    cx.cutoff = kernel_cutoff;
    // (the host vectors outlive the copies: every path below synchronises the stream)
    HX_HIP(hipMemcpyAsync(d + o_mat, matrix->score, sizeof(matrix->score), hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(d + o_seq, seqtab.data(), (size_t)ns * 8, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(d + o_pt, pt.data(), P * 16, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemsetAsync(d + o_rec, 0, P * kAlRecWords * 4, m.stream));
    if (total) HX_HIP(hipMemcpyAsync(d + o_codes, input->codes, total, hipMemcpyHostToDevice, m.stream));

    hclib_hip_dyn_stats_t st{};
    uint64_t fin[2] = {0, 0};
    const uint32_t root[kAlWords] = {kAlRoot, 0u, 0u, 0u, 0u, 0u};
    const int rc = launch_dyn(kAlWords, root, b.tasks, 0, 0, wpc, who, d, g_al, &st, fin,
                              [&](int grid, const DynView &v) {
                                  hipLaunchKernelGGL(k_alignment, dim3(grid), dim3(64), 0, m.stream, cx, v);
                              });
    result->tasks = st.tasks;
    result->created = st.created;
    result->promises = st.promises;
    result->pair_tasks = g_al.tasks[kCntPair];
    result->spawn_tasks = g_al.tasks[kCntSpawn];
    result->leaf_tasks = g_al.tasks[kCntLeaf];
    result->kernel_ms = st.kernel_ms;
    result->cells_per_s = st.kernel_ms > 0 ? (double)b.cells / (st.kernel_ms * 1e-3) : 0.0;
    if (rc) return rc;

    std::vector<int32_t> rec(P * kAlRecWords);
    HX_HIP(hipMemcpy(rec.data(), d + o_rec, rec.size() * 4, hipMemcpyDeviceToHost));
    for (size_t p = 0; p < P; ++p) {
        const int32_t *r = &rec[p * kAlRecWords];
        const int i = pt[p * 4], j = pt[p * 4 + 1];
        scores[(size_t)i * ns + j] = al_score(r[kRMatches], lens[i], lens[j]);
        result->matches += (uint64_t)r[kRMatches], result->diff_calls += (uint64_t)r[kRDiffs];
        result->type2 += (uint64_t)r[kRType2], result->ties += (uint64_t)r[kRTies];
        if (pairs) {
            hclib_hip_alignment_pair_t &q = pairs[p];
            q.si = i, q.sj = j, q.g = pt[p * 4 + 2], q.gh = pt[p * 4 + 3];
            q.maxscore = r[kRMax], q.se1 = r[kRSe1], q.se2 = r[kRSe2], q.sb1 = r[kRSb1], q.sb2 = r[kRSb2];
            q.matches = r[kRMatches], q.diff_calls = r[kRDiffs], q.type2 = r[kRType2], q.ties = r[kRTies];
        }
    }
    return HCLIB_HIP_OK;
}
