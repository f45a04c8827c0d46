// fft.hip — BOTS fft (test/performance-regression/full-apps/bots/fft: fft.ref.c
// the algorithm, fft.c the HClib port) as a fork-join client of dynamic device
// dataflow (include/hclib_hip/hx_dyn.h): fft_seq(n, in, out), the Cilk
// mixed-radix transform, as one launch of run_dyn_worker, every output
// bit-identical to the reference's given the reference's twiddle table.
//
//   task                    does (fft.ref.c lines)
//   CALL(s, src, dst,       fft_aux(s, src, dst) (:4653-4747). s <= cutoff (every
//        depth, fin)        base is): a LEAF, the whole sub-transform in this one
//                           task, pass by pass, then checks out of fin. Otherwise,
//                           with r = factors[depth], m = s / r, nb = ceil(m / band):
//                           f0 = open(nb), nb UNSH bands into f0, FORK awaiting f0
//                           (the unshuffle and its taskwait, :4691-4709). Where
//                           r = s (a prime above the cutoff) there is nothing to
//                           unshuffle and it does what POST does
//   UNSH(columns)           dst[j m + i] = src[i r + j] for its columns i, checks
//                           out of f0
//   FORK                    f1 = open(r), the r children CALL(m, dst + k m,
//                           src + k m, depth + 1, f1): the two buffers' roles
//                           swapped (:4712-4716), and POST awaiting f1
//   POST                    checks nbt tasks in to fin, spawns nbt TWID bands with
//                           fin, and checks out of fin itself (:4723-4743)
//   TWID(columns)           fft_twiddle_R (R = 2, 4, 8, 16): lane = column i, R
//                           strided 16-byte loads, the twiddles W[j l1], the
//                           butterfly in registers, R stores. The general radix
//                           (fft_twiddle_gen1 :194-221): a lane-item is one output
//                           (k, i), so that m = 1 still fills a wave; a band is
//                           `band` outputs, nbt = ceil(r m / band). Checks out of
//                           fin
//
// The root CALL (fin = kDynOpen in its payload) opens the program's outer finish.
//
// The codelets are one rule: fft_base_N and the column of
// fft_twiddle_R are the recursive radix-2 decimation-in-time butterfly, out[k] =
// E[k] + t, out[k + N/2] = E[k] - t with t = w^k O[k] formed by fft_tw below,
// whose constants are the codelets' 12-digit decimals and not the nearest
// doubles. Every product is rounded, then every sum: plain VALU f64 under
// -ffp-contract=off, no v_fma_f64 and no MFMA (DESIGN.md §14 has the reason).
// The general radix sums over j ascending from +0.0 and wraps its table index
// with `l0 > nW`: W[nW] is a real entry.
//
// A LEAF runs all calls of one depth of its subtree together, lanes over
// (call, column): the unshuffles down to the bases (a lane per base) or to a
// prime (general radix, m = 1), then the twiddle sweeps back up. Between two
// passes the wave drains its stores and acquires at agent scope: a pass reads
// what other lanes of this wave stored write-through in the pass before, at
// addresses this CU's L1 may hold from the pass before that (the buffers
// ping-pong), and the acquire invalidates them.
//
// Memory protocol. Every pair a task writes is one 16-byte write-through store
// (st_sc1_x4) drained by the task's check-out (dyn_finish_check_out<true>);
// every pair is read with plain loads behind run_dyn_worker's agent acquire
// (kSc1Payload = false). Both buffers are rewritten at every level by tasks on
// other CUs; DESIGN.md §19 walks one region through a level. The arena is
// [A n][B n][W n + 1] pairs; payloads carry u32 pair offsets into it, and every
// task checks them before it touches memory.
#include <string.h>

#include <vector>

#include "hx_client.h"
#include "hx_fft_host.h"

namespace hx {
namespace {

constexpr int kFftWords = 8;        // payload words per task
constexpr int kFftWavesPerCu = 8;
enum : uint32_t { kFftCall = 0, kFftFork = 1, kFftPost = 2, kFftUnsh = 3, kFftTwid = 4 };
enum : int { kCntLeaf = 0, kCntUnsh = 1, kCntTwid = 2, kCntCall = 3, kCntFork = 4, kCntPost = 5, kCntKinds = 6 };

struct FftCtx {
    double *m;                   // the arena: A, B, W as (re, im) pairs
    const uint32_t *fac;         // the factor list
    unsigned long long *counts;  // per task class (hx_client.h class_count)
    uint32_t n, nfac, cutoff, band;
};

__device__ __forceinline__ double2 fft_ld(const double *base, uint32_t pair) {
    return *(const double2 *)(base + 2 * (size_t)pair);
}
__device__ __forceinline__ void fft_st(double *base, uint32_t pair, double re, double im) {
    st_sc1_x4(base + 2 * (size_t)pair, make_uint4((uint32_t)__double2loint(re), (uint32_t)__double2hiint(re),
                                                  (uint32_t)__double2loint(im), (uint32_t)__double2hiint(im)));
}

// |cos(pi q / 16)|, q = 0 .. 8, as the codelets spell them
__device__ constexpr double fft_c32(int q) {
    return q == 0 ? 1.0
         : q == 1 ? 0.980785280403
         : q == 2 ? 0.923879532511
         : q == 3 ? 0.831469612303
         : q == 4 ? 0.707106781187
         : q == 5 ? 0.55557023302
         : q == 6 ? 0.382683432365
         : q == 7 ? 0.195090322016
                  : 0.0;
}

// t = w^K (a, b) of the N-point butterfly, the codelets' way
template <int N, int K>
__device__ __forceinline__ void fft_tw(double a, double b, double &tr, double &ti) {
    if constexpr (K == 0) {
        tr = a, ti = b;
    } else if constexpr (4 * K == N) {
        tr = b, ti = -a;
    } else if constexpr (8 * K == N) {
        tr = fft_c32(4) * (a + b), ti = fft_c32(4) * (b - a);
    } else if constexpr (8 * K == 3 * N) {
        tr = fft_c32(4) * (b - a), ti = -(fft_c32(4) * (a + b));
    } else if constexpr (4 * K < N) {
        constexpr int q = K * (32 / N);
        constexpr double c = fft_c32(q), s = fft_c32(8 - q);
        tr = c * a + s * b, ti = c * b - s * a;
    } else {
        constexpr int q = K * (32 / N);
        constexpr double c = fft_c32(16 - q), s = fft_c32(q - 8);
        tr = s * b - c * a, ti = -(s * a + c * b);
    }
}

template <int N, int K>
__device__ __forceinline__ void fft_bf_out(double *re, double *im, const double *er, const double *ei, const double *xr,
                                           const double *xi) {
    if constexpr (K < N / 2) {
        double tr, ti;
        fft_tw<N, K>(xr[K], xi[K], tr, ti);
        re[K] = er[K] + tr, im[K] = ei[K] + ti;
        re[K + N / 2] = er[K] - tr, im[K + N / 2] = ei[K] - ti;
        fft_bf_out<N, K + 1>(re, im, er, ei, xr, xi);
    }
}

// the N-point butterfly in place, natural order in and out; every index is a
// compile-time constant, so the arrays are registers
template <int N>
__device__ __forceinline__ void fft_bf(double *re, double *im) {
    if constexpr (N > 1) {
        double er[N / 2], ei[N / 2], xr[N / 2], xi[N / 2];
#pragma unroll
        for (int k = 0; k < N / 2; ++k) er[k] = re[2 * k], ei[k] = im[2 * k], xr[k] = re[2 * k + 1], xi[k] = im[2 * k + 1];
        fft_bf<N / 2>(er, ei);
        fft_bf<N / 2>(xr, xi);
        fft_bf_out<N, 0>(re, im, er, ei, xr, xi);
    }
}

// columns [u0, u1) of the unshuffle of a batch of calls of s = r m points each,
// call c at src + c s and dst + c s: dst[j m + i] = src[i r + j]. A lane reads
// its column's r contiguous pairs; the wave's stores are contiguous for each j
__device__ __forceinline__ void fft_unsh(const double *src, double *dst, uint32_t s, uint32_t r, uint32_t m, uint32_t u0,
                                         uint32_t u1) {
    for (uint32_t u = u0 + (uint32_t)lane_id(); u < u1; u += 64) {
        const uint32_t c = u / m, i = u - c * m, sp = c * s + i * r, dp = c * s + i;
        uint32_t j = 0;
        for (; j + 4 <= r; j += 4) {  // four loads in flight
            const double2 x0 = fft_ld(src, sp + j), x1 = fft_ld(src, sp + j + 1), x2 = fft_ld(src, sp + j + 2),
                          x3 = fft_ld(src, sp + j + 3);
            fft_st(dst, dp + j * m, x0.x, x0.y);
            fft_st(dst, dp + (j + 1) * m, x1.x, x1.y);
            fft_st(dst, dp + (j + 2) * m, x2.x, x2.y);
            fft_st(dst, dp + (j + 3) * m, x3.x, x3.y);
        }
        for (; j < r; ++j) {
            const double2 x = fft_ld(src, sp + j);
            fft_st(dst, dp + j * m, x.x, x.y);
        }
    }
}

// columns [u0, u1) of fft_twiddle_R over the same batch: column i of call c is
// src[c s + i + j m], input j != 0 times W[j l1], l1 = nWdn i
template <int R>
__device__ __forceinline__ void fft_twid(const double *src, double *dst, const double *W, uint32_t s, uint32_t m,
                                         uint32_t nwdn, uint32_t u0, uint32_t u1) {
    for (uint32_t u = u0 + (uint32_t)lane_id(); u < u1; u += 64) {
        const uint32_t c = u / m, i = u - c * m, at = c * s + i, l1 = nwdn * i;
        double re[R], im[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {
            // (radix 16 in two halves: with all 31 loads in flight the kernel does not fit 256 registers)
            if (R == 16 && j == 8) __builtin_amdgcn_sched_barrier(0);
            const double2 x = fft_ld(src, at + (uint32_t)j * m);
            if (j == 0) {
                re[0] = x.x, im[0] = x.y;
            } else {
                const double2 t = fft_ld(W, (uint32_t)j * l1);
                re[j] = t.x * x.x - t.y * x.y;
                im[j] = t.y * x.x + t.x * x.y;
            }
        }
        fft_bf<R>(re, im);
#pragma unroll
        for (int k = 0; k < R; ++k) fft_st(dst, at + (uint32_t)k * m, re[k], im[k]);
    }
}

// outputs [v0, v1) of fft_twiddle_gen1 over the same batch: output q = k m + i
// of call c, l1 = nWdn (i + m k) = nWdn q
__device__ __forceinline__ void fft_gen(const double *src, double *dst, const double *W, uint32_t s, uint32_t r, uint32_t m,
                                        uint32_t nwdn, uint32_t nw, uint32_t v0, uint32_t v1) {
    for (uint32_t v = v0 + (uint32_t)lane_id(); v < v1; v += 64) {
        const uint32_t c = v / s, q = v - c * s, i = q % m, l1 = nwdn * q, at = c * s + i;
        double r0 = 0.0, i0 = 0.0;
        uint32_t l0 = 0;
        for (uint32_t j = 0; j < r; ++j) {
            const double2 t = fft_ld(W, l0), x = fft_ld(src, at + j * m);
            r0 = r0 + (x.x * t.x - x.y * t.y);
            i0 = i0 + (x.x * t.y + x.y * t.x);
            l0 += l1;
            if (l0 > nw) l0 -= nw;
        }
        fft_st(dst, c * s + q, r0, i0);
    }
}

// the last stage of the N-point butterfly, each output stored as it is formed
template <int N, int K>
__device__ __forceinline__ void fft_bf_store(double *dst, uint32_t at, const double *er, const double *ei, const double *xr,
                                             const double *xi) {
    if constexpr (K < N / 2) {
        double tr, ti;
        fft_tw<N, K>(xr[K], xi[K], tr, ti);
        fft_st(dst, at + K, er[K] + tr, ei[K] + ti);
        fft_st(dst, at + K + N / 2, er[K] - tr, ei[K] - ti);
        fft_bf_store<N, K + 1>(dst, at, er, ei, xr, xi);
    }
}

// fft_base_N of calls [c0, c1) of the batch, a call per lane: the transform of
// the even inputs, then of the odd ones, then the last stage. The scheduling
// barrier keeps the odd half's loads behind the even half's butterfly: with all
// 32 pairs of a 32-point base loaded at once the kernel does not fit the 256
// registers that let two waves share a SIMD
template <int N>
__device__ __forceinline__ void fft_base(const double *src, double *dst, uint32_t c0, uint32_t c1) {
    for (uint32_t c = c0 + (uint32_t)lane_id(); c < c1; c += 64) {
        // (one 64-bit pointer per call: the pairs' offsets are immediates of the loads and stores)
        const double *in = src + 2 * (size_t)(c * N);
        double er[N / 2], ei[N / 2], xr[N / 2], xi[N / 2];
#pragma unroll
        for (int k = 0; k < N / 2; ++k) {
            const double2 x = fft_ld(in, 2 * k);
            er[k] = x.x, ei[k] = x.y;
        }
        fft_bf<N / 2>(er, ei);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < N / 2; ++k) {
            const double2 x = fft_ld(in, 2 * k + 1);
            xr[k] = x.x, xi[k] = x.y;
        }
        fft_bf<N / 2>(xr, xi);
        fft_bf_store<N, 0>(dst + 2 * (size_t)(c * N), 0, er, ei, xr, xi);
    }
}

__device__ __forceinline__ bool fft_codelet(uint32_t r) { return r == 2 || r == 4 || r == 8 || r == 16; }
__device__ __forceinline__ bool fft_base_size(uint32_t s) { return s == 2 || s == 4 || s == 8 || s == 16 || s == 32; }

// items [u0, u1) of the twiddle sweep of a batch: columns, or outputs of the general radix
__device__ __forceinline__ void fft_sweep(const FftCtx &c, const double *src, double *dst, uint32_t s, uint32_t r,
                                          uint32_t u0, uint32_t u1) {
    const double *W = c.m + 4 * (size_t)c.n;
    const uint32_t m = s / r, nwdn = c.n / s;
    if (r == 16) fft_twid<16>(src, dst, W, s, m, nwdn, u0, u1);
    else if (r == 8) fft_twid<8>(src, dst, W, s, m, nwdn, u0, u1);
    else if (r == 4) fft_twid<4>(src, dst, W, s, m, nwdn, u0, u1);
    else if (r == 2) fft_twid<2>(src, dst, W, s, m, nwdn, u0, u1);
    else fft_gen(src, dst, W, s, r, m, nwdn, c.n, u0, u1);
}

// between two passes of a leaf: this wave's write-through stores are out, and
// no line of this CU's L1 survives into the next pass
__device__ __forceinline__ void fft_pass_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    acquire_agent();
}

// fft_aux(s0, a, b) with factors[depth ..], all calls of a depth as one batch:
// depth e reads buffer (e even ? a : b) and writes the other
__device__ __forceinline__ void fft_leaf(const FftCtx &c, uint32_t s0, uint32_t a, uint32_t b, uint32_t depth) {
    double *pa = c.m + 2 * (size_t)a, *pb = c.m + 2 * (size_t)b;
    uint32_t s = s0, e = 0;
    while (!fft_base_size(s) && depth + e < c.nfac && c.fac[depth + e] < s) {
        const uint32_t r = c.fac[depth + e], m = s / r;
        fft_unsh(e & 1 ? pb : pa, e & 1 ? pa : pb, s, r, m, 0, s0 / r);  // (s0 / s) calls of m columns
        fft_pass_sync();
        s = m;
        ++e;
    }
    {
        const double *in = e & 1 ? pb : pa;
        double *out = e & 1 ? pa : pb;
        const uint32_t calls = s0 / s;
        if (s == 32) fft_base<32>(in, out, 0, calls);
        else if (s == 16) fft_base<16>(in, out, 0, calls);
        else if (s == 8) fft_base<8>(in, out, 0, calls);
        else if (s == 4) fft_base<4>(in, out, 0, calls);
        else if (s == 2) fft_base<2>(in, out, 0, calls);
        else fft_sweep(c, in, out, s, s, 0, s0);  // r = s: a prime, or n = 1
    }
    while (e) {
        --e;
        const uint32_t r = c.fac[depth + e];
        s *= r;
        fft_pass_sync();
        fft_sweep(c, e & 1 ? pb : pa, e & 1 ? pa : pb, s, r, 0, fft_codelet(r) ? s0 / r : s0);
    }
}

struct FftKind : TimedKind<FftKind, FftCtx> {
    using Ctx = FftCtx;
    static constexpr bool kSc1Payload = false;  // pairs move by plain loads behind the worker's acquire
    // payload: {kind, s, src, dst, depth, fin, u0, cnt}: the call's size, its two buffers (pair offsets), its index in
    // the factor list, the scope it (or for UNSH / TWID the band) checks out of, and a band's items
    __device__ static void bad(DynWave &w) {
        if (lane_id() == 0) dev_error(dyn_err(w.v), kErrBadTask);
    }
    __device__ static void body(const Ctx &c, DynWave &w, const uint32_t *pay, int &which) {
        const uint32_t kind = pay[0], s = pay[1], src = pay[2], dst = pay[3], depth = pay[4], u0 = pay[6], cnt = pay[7];
        const uint32_t lane = (uint32_t)lane_id();
        // both buffers of the call lie in [A, B] (2 n pairs) and do not overlap; s divides n, so that every
        // table index nWdn * (an index below s) is below n
        if (kind > kFftTwid || s == 0 || s > c.n || c.n % s || src > 2 * c.n - s || dst > 2 * c.n - s ||
            (src < dst ? dst - src : src - dst) < s || depth >= c.nfac)
            return bad(w);
        const uint32_t r = c.fac[depth];
        if (r == 0 || s % r) return bad(w);
        const uint32_t m = s / r;
        const uint32_t items = fft_codelet(r) ? m : s;  // of the twiddle sweep
        if (kind == kFftUnsh) {
            if (r >= s || cnt == 0 || u0 >= m || cnt > m - u0) return bad(w);
            fft_unsh(c.m + 2 * (size_t)src, c.m + 2 * (size_t)dst, s, r, m, u0, u0 + cnt);
            which = kCntUnsh;
            dyn_finish_check_out<true>(w, pay[5]);
            return;
        }
        if (kind == kFftTwid) {
            if (cnt == 0 || u0 >= items || cnt > items - u0) return bad(w);
            fft_sweep(c, c.m + 2 * (size_t)src, c.m + 2 * (size_t)dst, s, r, u0, u0 + cnt);
            which = kCntTwid;
            dyn_finish_check_out<true>(w, pay[5]);
            return;
        }
        uint32_t fin = pay[5];
        if (kind == kFftCall) {
            // the root has no scope yet: it opens the program's outer finish, checked in once, for itself
            if (fin == kDynOpen) fin = dyn_finish_open(w, 1);
            if (s <= c.cutoff) {
                fft_leaf(c, s, src, dst, depth);
                which = kCntLeaf;
                dyn_finish_check_out<true>(w, fin);
                return;
            }
            which = kCntCall;
            if (r < s) {
                const uint32_t nb = (m + c.band - 1) / c.band;
                const uint32_t f0 = dyn_finish_open(w, nb);
                for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
                    const uint32_t b = b0 + lane, i0 = b * c.band;
                    const uint32_t pl[kFftWords] = {kFftUnsh, s, src, dst, depth, f0, i0, i0 + c.band <= m ? c.band : m - i0};
                    dyn_async_await<true>(w, b < nb, pl, nullptr, 0);
                }
                const uint32_t pl[kFftWords] = {kFftFork, s, src, dst, depth, fin, 0, 0};
                const uint32_t fut[1] = {f0};
                dyn_async_await<true>(w, lane == 0, pl, fut, 1);
                return;
            }
            // r = s: straight to the sweep, as POST below
        } else if (r >= s) {
            return bad(w);
        }
        if (kind == kFftFork) {
            which = kCntFork;
            const uint32_t f1 = dyn_finish_open(w, r);
            for (uint32_t k0 = 0; k0 < r; k0 += 64) {
                const uint32_t k = k0 + lane;
                const uint32_t pl[kFftWords] = {kFftCall, m, dst + k * m, src + k * m, depth + 1, f1, 0, 0};
                dyn_async_await<true>(w, k < r, pl, nullptr, 0);
            }
            const uint32_t pl[kFftWords] = {kFftPost, s, src, dst, depth, fin, 0, 0};
            const uint32_t fut[1] = {f1};
            dyn_async_await<true>(w, lane == 0, pl, fut, 1);
            return;
        }
        // POST, or a CALL whose factor is its size
        if (kind == kFftPost) which = kCntPost;
        const uint32_t nbt = (items + c.band - 1) / c.band;
        dyn_finish_check_in(w, fin, nbt);
        for (uint32_t b0 = 0; b0 < nbt; b0 += 64) {
            const uint32_t b = b0 + lane, i0 = b * c.band;
            const uint32_t pl[kFftWords] = {kFftTwid, s, src, dst, depth, fin, i0, i0 + c.band <= items ? c.band : items - i0};
            dyn_async_await<true>(w, b < nbt, pl, nullptr, 0);
        }
        dyn_finish_check_out<true>(w, fin);
    }
};

// two waves per SIMD, eight per CU: 256 registers each (the 32-point base holds 64 doubles)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_fft(FftCtx c, DynView v) {
    run_dyn_worker<FftKind>(c, v);
}

ClassCounters<kCntKinds> g_fft;  // the last launch's

int fft_args(const char *who, bool ptrs_ok, int n, int &cutoff, int &band, FftPlan &p) {
    if (!ptrs_ok) {
        set_error("%s: in, out (and the output array) must not be NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    std::string err;
    if (fft_check_args(n, cutoff, band, err) || fft_plan(n, cutoff, band, p, err)) {
        set_error("%s: %s", who, err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    return HCLIB_HIP_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_fft_factors(int n, int out[40]) {
    if (!out) {
        set_error("hclib_hip_fft_factors: out must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    std::string err;
    const int cnt = fft_factors(n, out, err);
    if (cnt < 0) {
        set_error("hclib_hip_fft_factors: %s", err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    return cnt;
}

extern "C" int hclib_hip_fft_twiddles(int n, double *w) {
    if (!w || n < 1 || n > kFftMaxN) {
        set_error("hclib_hip_fft_twiddles: w must not be NULL and n = %d must be in 1 .. 2^26", n);
        return HCLIB_HIP_EINVAL;
    }
    fft_twiddles(n, w);
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_fft_bounds(int n, int cutoff, int band, uint64_t out[6]) {
    FftPlan p;
    HX_TRY(fft_args("hclib_hip_fft_bounds", out != nullptr, n, cutoff, band, p));
    out[0] = p.tasks;
    out[1] = p.scopes;
    out[2] = p.nodes;
    out[3] = p.leaves;
    out[4] = p.bands;
    out[5] = p.bytes;
    return HCLIB_HIP_OK;
}

extern "C" void hclib_hip_fft_last_ticks(uint64_t out[6]) {
    for (int k = 0; k < kCntKinds; ++k) out[k] = g_fft.ticks[k];
}

extern "C" int hclib_hip_fft(const double *in, double *out, int n, const double *w, int cutoff, int band,
                             hclib_hip_fft_result_t *result) {
    // argument errors first, before the device is touched
    FftPlan p;
    HX_TRY(fft_args("hclib_hip_fft", in && out, n, cutoff, band, p));
    HX_TRY(ensure_device());
    Module &m = mod();

    // [counts: a line per task class][the factor list][A][B][W]
    const size_t hdr = g_fft.kBytes + 256, nbytes = (size_t)n * 16, wbytes = ((size_t)n + 1) * 16;
    const size_t bytes = hdr + 2 * nbytes + wbytes;
    char *d = nullptr;
    if (const int rc = arena_reserve(kArenaFft, bytes, "hclib_hip_fft", (void **)&d)) {
        set_error("hclib_hip_fft: hipMalloc(%zu) failed (n = %d: two buffers and the table of 16 n bytes each)", bytes, n);
        return rc;
    }
    uint32_t fac[64] = {};
    for (int k = 0; k < p.nfactors; ++k) fac[k] = (uint32_t)p.factors[k];
    std::vector<double> table;
    if (!w) {
        table.resize(2 * ((size_t)n + 1));
        fft_twiddles(n, table.data());
        w = table.data();
    }
    // (`in`, `w` and `fac` outlive the copies: launch_dyn synchronises the stream)
    HX_HIP(hipMemcpyAsync(d + g_fft.kBytes, fac, 256, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(d + hdr, in, nbytes, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(d + hdr + 2 * nbytes, w, wbytes, hipMemcpyHostToDevice, m.stream));

    FftCtx cx;
    cx.m = (double *)(d + hdr);
    cx.fac = (const uint32_t *)(d + g_fft.kBytes);
    cx.counts = (unsigned long long *)d;
    cx.n = (uint32_t)n;
    cx.nfac = (uint32_t)p.nfactors;
    cx.cutoff = (uint32_t)cutoff;
    cx.band = (uint32_t)band;
    const uint32_t root[kFftWords] = {kFftCall, (uint32_t)n, 0u, (uint32_t)n, 0u, kDynOpen, 0u, 0u};
    // (HCLIB_HIP_FFT_WAVES_PER_CU: for measurements)
    int wpc = env_int("HCLIB_HIP_FFT_WAVES_PER_CU", fft_default_waves(n));
    wpc = wpc < 1 ? 1 : (wpc > kFftWavesPerCu ? kFftWavesPerCu : wpc);
    hclib_hip_dyn_stats_t st{};
    uint64_t fin[2] = {0, 0};
    const int rc = launch_dyn(kFftWords, root, p.tasks, p.scopes, p.nodes ? p.nodes : 1, wpc, "hclib_hip_fft", d, g_fft, &st,
                              fin, [&](int grid, const DynView &v) {
                                  hipLaunchKernelGGL(k_fft, dim3(grid), dim3(64), 0, m.stream, cx, v);
                              });
    if (result) {
        memset(result, 0, sizeof(*result));
        result->tasks = st.tasks;
        result->leaves = g_fft.tasks[kCntLeaf];
        result->calls = g_fft.tasks[kCntCall];
        result->unsh_bands = g_fft.tasks[kCntUnsh];
        result->twid_bands = g_fft.tasks[kCntTwid];
        result->finishes = fin[0];
        result->check_ins = fin[1];
        result->bytes_moved = p.bytes;
        result->nfactors = p.nfactors;
        for (int k = 0; k < p.nfactors; ++k) result->factors[k] = p.factors[k];
        result->cutoff = cutoff;
        result->band = band;
        result->kernel_ms = st.kernel_ms;
        result->gbytes_per_s = st.kernel_ms > 0 ? (double)p.bytes / (st.kernel_ms * 1e6) : 0.0;
    }
    if (rc) return rc;
    HX_HIP(hipMemcpy(out, d + hdr + nbytes, nbytes, hipMemcpyDeviceToHost));
    return HCLIB_HIP_OK;
}
