// hx_uts_host.h — the host side of the UTS tree rules in plain C++ (no HIP):
// the reference's per-node formula evaluated with libm, the integer rule and
// threshold tables the device reads instead, the bucket bytes of the
// fixed-shape lookup and the host mirrors of both lookups. uts.hip uploads
// the tables; hx_uts_plan.h sizes a launch from them; tests/cpp/uts_plan.cpp
// builds them without a GPU.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/hclib_hip.h"

namespace hx {

// ------------------------------------------------------------- SHA-1
#define HX_ROTL(x, n) (((x) << (n)) | ((x) >> (32 - (n))))
#define HX_RND(f, k, wi)                                \
    {                                                   \
        uint32_t t_ = HX_ROTL(a, 5) + (f) + e + (k) + (wi); \
        e = d;                                          \
        d = c;                                          \
        c = HX_ROTL(b, 30);                             \
        b = a;                                          \
        a = t_;                                         \
    }
#define HX_F1 (d ^ (b & (c ^ d)))
#define HX_F2 (b ^ c ^ d)
#define HX_F3 ((b & c) | (d & (b ^ c)))
#define HX_W(i) \
    (w[(i) & 15] = HX_ROTL(w[((i) + 13) & 15] ^ w[((i) + 8) & 15] ^ w[((i) + 2) & 15] ^ w[(i) & 15], 1))

// A depth rule, read as an int4 on the device (uts.hip asserts the layout).
// x: 0 = constant y children; 1 = BIN: rand < y ? m : 0;
//    2 = GEO: threshold table z (128 words, entries 1..100)
struct UtsRule {
    int x, y, z, w;
};

constexpr size_t kUtsLdsRules = 64;     // depth rules cached in LDS per wave
constexpr size_t kUtsLdsThr = 4 * 128;  // up to 4 GEO threshold tables
// kUtsGeoFixed: 1024 buckets of rand (2^21 wide), one byte each, kept in
// s_thr words 128..383 (a fixed-shape tree has one table: the rest is free)
constexpr int kUtsBuckets = 1024, kUtsBucketShift = 21;

// ------------------------------------------------------ host: rules/tables
// The reference's per-node formula, uts.c:143-222, evaluated with libm.
inline int cvt_int_x86(double x) {
    // (int) conversion as x86-64 cvttsd2si: NaN / out of range -> INT_MIN
    if (!(x >= -2147483648.0 && x < 2147483648.0)) return (int)0x80000000u;
    return (int)x;
}

inline double geo_bi(const hclib_hip_uts_params_t &p, int depth) {
    double b_i = p.b_0;
    if (depth > 0) {
        switch (p.shape_fn) {
        case 1: b_i = p.b_0 * pow((double)depth, -log(p.b_0) / log((double)p.gen_mx)); break;
        case 2:
            if (depth > 5 * p.gen_mx) { b_i = 0.0; break; }
            b_i = pow(p.b_0, sin(2.0 * 3.141592653589793 * (double)depth / (double)p.gen_mx));
            break;
        case 3: b_i = (depth < p.gen_mx) ? p.b_0 : 0; break;
        default: b_i = p.b_0 * (1.0 - (double)depth / (double)p.gen_mx); break;
        }
    }
    return b_i;
}

inline int geo_n(double prob, uint32_t h) {
    double u = (double)(int)h / 2147483648.0;
    return cvt_int_x86(floor(log(1 - u) / log(1 - prob)));
}

// The children of a BIN-rule node that spawns (uts.c:162-168 return m; the
// caller, uts.c:225-274, then truncates every node but a BIN root and every
// tree but BALANCED to MAXNUMCHILDREN = 100, uts.h:31): -m above 100 gives
// 100 children, on the device (UtsCtx::m) and in the host mirror (host_nc)
constexpr int kUtsMaxChildren = 100;
inline int bin_rule_m(const hclib_hip_uts_params_t &p) {
    return p.non_leaf_bf > kUtsMaxChildren ? kUtsMaxChildren : p.non_leaf_bf;
}

// Expected node count of a GEO / HYBRID tree (sum over depths of the product
// of the mean branching factors above it) — a launch-shape heuristic only:
// T1 1.4 M, T2 0.8 M, T4 3.3 M, T5 3.8 M, T1L 89 M, T2L 184 M
inline double uts_expected_nodes(const hclib_hip_uts_params_t &p) {
    double tot = 0.0, prod = 1.0;
    for (int d = 0; d < 10 * p.gen_mx + 10 && prod > 1e-9 && tot < 1e13; ++d) {
        tot += prod;
        const bool bin_level = p.type == 0 ? d > 0 : (p.type == 2 && d >= p.shift_depth * p.gen_mx);
        const double mu = bin_level ? p.non_leaf_prob * bin_rule_m(p) : geo_bi(p, d);
        prod *= mu > 0.0 ? mu : 0.0;
    }
    return tot;
}

struct UtsTables {
    std::vector<UtsRule> rules;
    std::vector<uint32_t> thr;  // 128 words per geo table
    int stationary = 1;
    int root_nc = 0;
    uint32_t root[5];
};

inline void sha1_host(uint32_t w[16], uint32_t h[5]) {
    uint32_t a = 0x67452301u, b = 0xefcdab89u, c = 0x98badcfeu, d = 0x10325476u, e = 0xc3d2e1f0u;
    for (int i = 0; i < 80; ++i) {
        uint32_t wi = (i < 16) ? w[i] : HX_W(i);
        if (i < 20) HX_RND(HX_F1, 0x5a827999u, wi)
        else if (i < 40) HX_RND(HX_F2, 0x6ed9eba1u, wi)
        else if (i < 60) HX_RND(HX_F3, 0x8f1bbcdcu, wi)
        else HX_RND(HX_F2, 0xca62c1d6u, wi)
    }
    h[0] = 0x67452301u + a;
    h[1] = 0xefcdab89u + b;
    h[2] = 0x98badcfeu + c;
    h[3] = 0x10325476u + d;
    h[4] = 0xc3d2e1f0u + e;
}

// Build the geo table for b_i; returns table index (deduplicated) or -1 for
// "always 0 children"; -2 if the formula is not monotone in rand (unsupported).
inline int geo_table(UtsTables &T, double b_i) {
    const double prob = 1.0 / (1.0 + b_i);
    uint32_t thr[128];
    thr[0] = 0;
    bool any = false;
    const int nmax = geo_n(prob, 0x7fffffffu);
    for (int k = 1; k <= 100; ++k) {
        if (nmax < k) {  // never reached (INT_MIN / capped by the range end)
            thr[k] = 0x80000000u;
            continue;
        }
        uint32_t lo = 0, hi = 0x7fffffffu;  // smallest h with n(h) >= k
        while (lo < hi) {
            uint32_t mid = lo + (hi - lo) / 2;
            if (geo_n(prob, mid) >= k) hi = mid;
            else lo = mid + 1;
        }
        thr[k] = lo;
        any = true;
    }
    for (int k = 101; k < 128; ++k) thr[k] = 0x80000000u;
    if (!any) return -1;
    // spot-verify monotonicity / table agreement around every threshold
    for (int k = 1; k <= 100; ++k) {
        if (thr[k] == 0x80000000u) break;
        for (int dlt = -2; dlt <= 2; ++dlt) {
            int64_t hh = (int64_t)thr[k] + dlt;
            if (hh < 0 || hh > 0x7fffffff) continue;
            int n = geo_n(prob, (uint32_t)hh);
            int want = n < 0 ? 0 : (n > 100 ? 100 : n);
            int got = 0;
            for (int q = 1; q <= 100; ++q) got += thr[q] <= (uint32_t)hh;
            if (got != want) return -2;
        }
    }
    const size_t nt = T.thr.size() / 128;
    if (nt && !memcmp(&T.thr[(nt - 1) * 128], thr, sizeof(thr))) return (int)(nt - 1);
    T.thr.insert(T.thr.end(), thr, thr + 128);
    return (int)nt;
}

inline int bin_threshold(double q) {
    // smallest h with h/2^31 >= q; rand < thr  <=>  d < q (uts.c:162-168)
    uint32_t lo = 0, hi = 0x80000000u;
    while (lo < hi) {
        uint32_t mid = lo + (hi - lo) / 2;
        if (((double)(int)mid) / 2147483648.0 >= q) hi = mid;
        else lo = mid + 1;
    }
    return (int)lo;
}

// HCLIB_HIP_OK, or HCLIB_HIP_EINVAL with the reason in `err`
inline int build_tables(const hclib_hip_uts_params_t &p, UtsTables &T, std::string &err) {
    T.rules.clear();
    T.thr.clear();
    auto geo_rule = [&](int d) -> UtsRule {
        int t = geo_table(T, geo_bi(p, d));
        if (t == -1) return UtsRule{0, 0, 0, 0};
        if (t == -2) return UtsRule{-1, 0, 0, 0};
        return UtsRule{2, 0, t, 0};
    };
    int D = 0;
    switch (p.type) {
    case 0:  // BIN
        T.rules.push_back(UtsRule{0, 0, 0, 0});  // root handled by root_nc
        T.rules.push_back(UtsRule{1, bin_threshold(p.non_leaf_prob), 0, 0});
        T.stationary = 1;
        break;
    case 1:  // GEO
        if (p.shape_fn == 3 || p.shape_fn == 0) { D = p.gen_mx + 1; T.stationary = 1; }
        else if (p.shape_fn == 2) { D = 5 * p.gen_mx + 2; T.stationary = 1; }
        else { D = 4096; T.stationary = 0; }
        for (int d = 0; d < D; ++d) T.rules.push_back(geo_rule(d));
        if (T.stationary) T.rules.push_back(UtsRule{0, 0, 0, 0});
        break;
    case 2: {  // HYBRID: geo below shift_depth*gen_mx, bin after
        int d = 0;
        for (; d < p.shift_depth * p.gen_mx; ++d) T.rules.push_back(geo_rule(d));
        T.rules.push_back(UtsRule{1, bin_threshold(p.non_leaf_prob), 0, 0});
        T.stationary = 1;
        break;
    }
    case 3:  // BALANCED
        for (int d = 0; d < p.gen_mx; ++d) T.rules.push_back(UtsRule{0, (int)p.b_0, 0, 0});
        T.rules.push_back(UtsRule{0, 0, 0, 0});
        T.stationary = 1;
        break;
    default:
        err = "uts: unknown tree type " + std::to_string(p.type);
        return HCLIB_HIP_EINVAL;
    }
    for (auto &r : T.rules)
        if (r.x == -1) {
            err = "uts: numChildren is not monotone in rand for these parameters";
            return HCLIB_HIP_EINVAL;
        }
    if (T.thr.empty()) T.thr.assign(128, 0x80000000u);
    // the root (uts_initRoot uts.c:151-159 + uts_numChildren at height 0)
    uint32_t w[16] = {0};
    w[4] = (uint32_t)p.root_id;
    w[5] = 0x80000000u;
    w[15] = 160;
    sha1_host(w, T.root);
    const uint32_t r = T.root[4] & 0x7fffffffu;
    int nc = 0;
    switch (p.type) {
    case 0: nc = (int)floor(p.b_0); break;
    case 1: nc = geo_n(1.0 / (1.0 + geo_bi(p, 0)), r); break;
    case 2: nc = (0 < p.shift_depth * p.gen_mx) ? geo_n(1.0 / (1.0 + geo_bi(p, 0)), r)
                                               : ((((double)(int)r) / 2147483648.0 < p.non_leaf_prob) ? p.non_leaf_bf : 0);
            break;
    case 3: nc = (0 < p.gen_mx) ? (int)p.b_0 : 0; break;
    }
    if (p.type == 0) {
        int root_bf = (int)ceil(p.b_0);
        if (nc > root_bf) nc = root_bf;
    } else if (p.type != 3 && nc > 100) {
        nc = 100;
    }
    T.root_nc = nc;
    return HCLIB_HIP_OK;
}

// table 0's bucket bytes (kUtsGeoFixed, uts_nc): per bucket
// [b 2^21, (b+1) 2^21) of rand, n_lo = #{k : thr[k] <= b 2^21} and 0x80 when
// more than two thresholds lie strictly inside it
inline void build_buckets(const uint32_t *t0, uint8_t nb[kUtsBuckets]) {
    for (int b = 0; b < kUtsBuckets; ++b) {
        const uint64_t lo = (uint64_t)b << kUtsBucketShift, hi = (uint64_t)(b + 1) << kUtsBucketShift;
        int nlo = 0, inside = 0;
        for (int k = 1; k <= 100; ++k) {
            nlo += t0[k] <= lo;
            inside += t0[k] > lo && t0[k] < hi;
        }
        nb[b] = (uint8_t)(nlo | (inside > 2 ? 0x80 : 0));
    }
}

// the device lookup of uts_nc<kUtsGeoFixed> (below the depth cut), on the
// host: bucket byte, two compares, binary search in a dense bucket
inline int bucket_nc(const uint32_t *t0, const uint8_t *nb, uint32_t r) {
    const uint32_t e = nb[r >> kUtsBucketShift], nlo = e & 0x7fu;
    uint32_t n = nlo + (t0[nlo + 1] <= r ? 1u : 0u) + (t0[nlo + 2] <= r ? 1u : 0u);
    if (e & 0x80u) {
        int lo = (int)nlo, hi = 100;
        for (int s = 0; s < 7; ++s) {
            const int mid = (lo + hi + 1) >> 1;
            if (lo < hi) {
                if (t0[mid] <= r) lo = mid;
                else hi = mid - 1;
            }
        }
        n = (uint32_t)lo;
    }
    return (int)n;
}

inline int host_nc(const hclib_hip_uts_params_t &p, const UtsTables &T, int d, uint32_t r) {
    int ri = d < (int)T.rules.size() ? d : (int)T.rules.size() - 1;
    UtsRule rule = T.rules[ri];
    if (rule.x == 0) return rule.y;
    if (rule.x == 1) return r < (uint32_t)rule.y ? bin_rule_m(p) : 0;
    int n = 0;
    for (int k = 1; k <= 100; ++k) n += T.thr[(size_t)rule.z * 128 + k] <= r;
    return n;
}

}  // namespace hx
