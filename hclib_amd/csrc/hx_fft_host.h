// hx_fft_host.h — the host half of BOTS fft (fft.hip) in plain C++: no HIP and
// no getenv, so a host program can check it under sanitizers
// (tests/cpp/fft_host.cpp). The reference's factor() and factor list
// (bots/fft/fft.ref.c:110-126, :4886-4890), the twiddle table's formula and
// write order (compute_w_coefficients :60-84), the argument checks, and the
// plan: the closed-form counts every pool of a launch is sized from
// (DESIGN.md §19).
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

namespace hx {

constexpr int kFftMaxN = 1 << 26;       // twice the reference's default, inside its int index arithmetic (31 l1)
constexpr int kFftMaxPrime = 512;       // the general radix costs r terms per output
constexpr int kFftMaxFactors = 40;      // the reference's factors[40]
constexpr int kFftMinCutoff = 32;       // every base (2 .. 32 points) is a leaf
constexpr int kFftDefaultCutoff = 8192; // 16 x 16 x 32: every pass of such a leaf has at least 256 lane-items
// columns (general radix: outputs) per UNSH / TWID band, and persistent waves per CU, by the size of the
// transform (measured at 2^13 .. 2^25): a small graph is bound by its span and by the waves that
// start, poll and leave, a large one by throughput
constexpr int kFftBigN = 1 << 22;
constexpr int kFftBandSmall = 256, kFftBandBig = 1024;
constexpr int kFftWavesSmall = 1, kFftWavesBig = 4;
inline int fft_default_band(int n) { return n > kFftBigN ? kFftBandBig : kFftBandSmall; }
inline int fft_default_waves(int n) { return n > kFftBigN ? kFftWavesBig : kFftWavesSmall; }
constexpr int kFftEinval = -2;          // HCLIB_HIP_EINVAL

// factor(), with the odd search cut at kFftMaxPrime: 0 where the smallest odd
// factor is larger (the transform is refused)
inline int fft_factor(int n) {
    if (n < 2) return 1;
    if (n == 64 || n == 128 || n == 256 || n == 1024 || n == 2048 || n == 4096) return 8;
    if ((n & 15) == 0) return 16;
    if ((n & 7) == 0) return 8;
    if ((n & 3) == 0) return 4;
    if ((n & 1) == 0) return 2;
    for (int r = 3; r < n && r <= kFftMaxPrime; r += 2)
        if (n % r == 0) return r;
    return n <= kFftMaxPrime ? n : 0;
}

inline bool fft_is_base(uint32_t n) { return n == 2 || n == 4 || n == 8 || n == 16 || n == 32; }
inline bool fft_is_codelet(uint32_t r) { return r == 2 || r == 4 || r == 8 || r == 16; }

// fft_seq's factor list; the count, or kFftEinval with `err` set
inline int fft_factors(int n, int out[kFftMaxFactors], std::string &err) {
    if (n < 1 || n > kFftMaxN) {
        err = "n = " + std::to_string(n) + " must be in 1 .. 2^26";
        return kFftEinval;
    }
    int cnt = 0, l = n;
    do {
        const int r = fft_factor(l);
        if (r == 0) {
            err = "n = " + std::to_string(n) + " has a prime factor above " + std::to_string(kFftMaxPrime);
            return kFftEinval;
        }
        out[cnt++] = r;  // (2^26 has 7 factors, 3^16 sixteen: far below 40)
        l /= r;
    } while (l > 1);
    return cnt;
}

// compute_w_coefficients: n + 1 (re, im) pairs, k = 0 .. n / 2 ascending,
// W[k] = (c, -s) and then W[n - k] = (c, s). W[0].im is -0.0, W[n].im +0.0, and
// for even n the second write leaves W[n / 2].im = +sin. The reference's
// binary takes both values of one argument from one sincos call, whose sine
// can differ from sin's by an ulp: this table is a convenience, the
// reference's own is an input.
inline void fft_twiddles(int n, double *w) {
    const double two_pi_over_n = 2.0 * 3.1415926535897932384626434 / n;
    for (int k = 0; k <= n / 2; ++k) {
        const double c = cos(two_pi_over_n * k), s = sin(two_pi_over_n * k);
        w[2 * (size_t)k] = w[2 * (size_t)(n - k)] = c;
        w[2 * (size_t)k + 1] = -s;
        w[2 * (size_t)(n - k) + 1] = s;
    }
}

inline int fft_check_args(int n, int &cutoff, int &band, std::string &err) {
    int fl[kFftMaxFactors];
    if (fft_factors(n, fl, err) < 0) return kFftEinval;
    if (cutoff == 0) cutoff = kFftDefaultCutoff;
    if (cutoff < kFftMinCutoff) {
        err = "cutoff = " + std::to_string(cutoff) + " must be 0 (8192) or at least 32";
        return kFftEinval;
    }
    if (band == 0) band = fft_default_band(n);
    if (band < 0 || band % 64) {
        err = "band = " + std::to_string(band) + " must be 0 (the default) or a multiple of 64";
        return kFftEinval;
    }
    return 0;
}

// bands of the twiddle sweep of a call of r x m points: a band is `band`
// columns, or for the general radix `band` outputs (k, i)
inline uint64_t fft_twid_bands(uint64_t r, uint64_t m, uint64_t band) {
    return ((fft_is_codelet((uint32_t)r) ? m : r * m) + band - 1) / band;
}

// The graph is a function of (n, cutoff, band) alone: every count is exact.
struct FftPlan {
    int factors[kFftMaxFactors] = {};
    int nfactors = 0;
    uint64_t tasks = 0, scopes = 0, nodes = 0, leaves = 0, bands = 0, bytes = 0, check_ins = 0;
    uint64_t calls = 0;  // CALL tasks that are not leaves
};

// (arguments as fft_check_args leaves them)
inline int fft_plan(int n, int cutoff, int band, FftPlan &p, std::string &err) {
    p = FftPlan();
    p.nfactors = fft_factors(n, p.factors, err);
    if (p.nfactors < 0) return kFftEinval;
    uint64_t size = (uint64_t)n, calls = 1, passes = 0;
    int d = 0;
    p.scopes = 1;  // the outer finish
    while (size > (uint64_t)cutoff) {
        const uint64_t r = (uint64_t)p.factors[d], m = size / r, nbt = fft_twid_bands(r, m, (uint64_t)band);
        p.calls += calls;
        if (r == size) {  // a prime above the cutoff: nothing to unshuffle, CALL goes straight to its sweep
            p.tasks += calls * (1 + nbt);
            p.bands += calls * nbt;
            p.check_ins += calls * nbt;
            passes += 1;
            size = 0;
            break;
        }
        const uint64_t nb = (m + band - 1) / band;
        p.tasks += calls * (3 + nb + nbt);  // CALL, FORK, POST and the two sweeps' bands
        p.bands += calls * (nb + nbt);
        p.check_ins += calls * nbt;
        p.scopes += 2 * calls;  // f0 and f1
        p.nodes += 2 * calls;   // FORK awaiting f0, POST awaiting f1
        passes += 2;
        calls *= r;
        size = m;
        ++d;
    }
    if (size) {
        p.leaves = calls;
        p.tasks += calls;
        // a leaf's passes: unshuffles down, the bases or a last general sweep, twiddles up
        uint64_t s = size;
        while (!fft_is_base((uint32_t)s) && (uint64_t)p.factors[d] < s) {
            passes += 2;
            s /= (uint64_t)p.factors[d];
            ++d;
        }
        passes += 1;
    }
    p.bytes = 32ull * (uint64_t)n * passes;  // every pass reads and writes all n pairs once
    if (p.tasks >= 0xfffffff0ull) {
        err = "n = " + std::to_string(n) + " needs " + std::to_string(p.tasks) + " tasks (at most 2^32 - 17)";
        return kFftEinval;
    }
    return 0;
}

}  // namespace hx
