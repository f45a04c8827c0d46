// hx_uts_plan.h — the launch shape of a UTS search and everything its launches
// differ in, in plain C++: no HIP and no getenv, so a host program can check
// every decision (tests/cpp/uts_plan.cpp). hclib_hip_uts_search (uts.hip)
// reads the environment into UtsKnobs, plans, and carries the plan out.
#pragma once

#include <stdarg.h>
#include <stdio.h>

#include "hx_uts_host.h"

namespace hx {

// numChildren lookup modes (the kernel is instantiated per mode)
enum UtsMode : int {
    kUtsRulesGlobal = 0,  // depth rules in device memory (large tables)
    kUtsRulesLds = 1,     // depth rules cached in LDS
    kUtsBin = 2,          // BIN tree: one rule for every depth >= 1 (no lookup at all)
    kUtsGeoFixed = 3,     // GEO tree with one table above a depth and leaves below
                          // (shape -a 3: T1, T1L, T1XL): no rule lookup, the first 16
                          // thresholds in registers, the rest (P(n > 16) = 0.8^17 at
                          // b = 4) binary-searched in LDS
};

// the seeding expands at most this many levels (hx_sched.h kSeedMaxLevels;
// uts.hip asserts they agree)
constexpr int kUtsSeedMaxLevels = 24;

// The environment knobs' values (uts.hip's uts_knobs() reads them): member
// <name> is HCLIB_HIP_<NAME>, and a member's default is the knob's. kUnset: the
// default depends on the plan (uts_plan).
struct UtsKnobs {
    static constexpr int kUnset = -0x7fffffff;
    int grid = 0;                // workers; 0: num_cus x waves_per_cu
    int waves_per_cu = kUnset;   // 2, 4 or 8 by tree class and size
    int wpg = 4;                 // worker waves per workgroup (BIN trees): 1, 2 or 4
    int uts_ring = kUnset;       // whole fixed-shape trees: 256, 512 or 1024 items per wave
    int uts_geo_fixed = 1;       // 0: fixed-shape GEO trees search through the rule tables
    int uts_seed = 1;            // 0: every search starts from the root
    int uts_trace = 0;           // 1 depth trace, 2 chain stamps (with a histogram array only)
    int uts_dual = 1;
    int deques = 128, deque_cap = 4096, chunk = 64;
    int spill_hi = 512;
    int spill_lo = kUnset;       // 66 BIN, 128 / 224 GEO, 336 / 448 seeded
    int seed_per_wave = kUnset;  // 16, or 32 from 3e7 expected nodes
    bool seed_per_wave_set = false;  // the variable exists: its refusals apply only then
    int seed_levels = 20, seed_solo = 128;
    int hunger = kUnset;         // 32, 64 on BIN trees, 128 on large fixed-shape ones
    int spin_limit_ms = 20000, stamps = 0, carry = 2, backoff = 16, defer = 1, spills_per_batch = 0;
    int narrow_shed = 1, narrow_shed_sibs = 3;
    // the hand-off wave of a BIN workgroup and the users of its outbox (bits:
    // 1 the give-away loop, 2 narrow_shed's leftovers, 4 the wave's redirect
    // to a sibling gone idle; 0: no such wave, workgroups of 64 x wpg threads).
    // 2: T3L 25.60 -> 24.59 ms against 0, medians of six interleaved rounds; 1
    // alone 25.82, 3 24.54, 6 24.65, 7 24.65 (profiles/r23/ab_comm_knob_t3l.log):
    // bits 1 and 4 show no gain and stay off
    int uts_comm = 2;
};

// waves in a workgroup of k_uts_search<..., global, wpg> at most: the worker
// waves and, where the kernel can run one, the hand-off wave
constexpr int uts_block_waves(int wpg, bool global) { return wpg + (wpg > 1 && !global ? 1 : 0); }

// HCLIB_HIP_UTS_COMM is a set of three bits
inline bool uts_comm_valid(int comm, std::string &err) {
    if (comm >= 0 && comm <= 7) return true;
    char buf[160];
    snprintf(buf, sizeof(buf),
             "hclib_hip_uts_search: HCLIB_HIP_UTS_COMM=%d is not a set of the outbox's users (0..7: 1 give-away, 2 "
             "narrow shed, 4 redirect)", comm);
    err = buf;
    return false;
}

struct UtsPlan {
    int status = HCLIB_HIP_OK;  // HCLIB_HIP_EINVAL: a knob or the trace was refused (`err` says why)
    // tree class
    bool bin = false, geo_fixed = false;
    int geo_depth = 0;   // kUtsGeoFixed: depths 1..geo_depth-1 use table 0, deeper nodes are leaves
    int lds_tables = 0;  // rules / thr fit the per-wave LDS cache
    uint32_t bin_thr = 0;
    // the kernel: k_uts_search<mode, feat, ring, global, wpg>
    int mode = 0;
    int feat = 0;  // 0 plain; 1 shard filter and / or histogram; 2 depth trace; 3 chain stamps
    bool global = false;
    int ring = 512, wpg = 1, grid = 0, waves_per_cu = 0;
    // chunk deques (make_pool)
    uint32_t nq = 0, deque_cap = 0, chunk = 0;
    // SchedConfig, member by member
    uint32_t spill_hi = 0, spill_lo = 0, spin_limit = 0, nwaves = 0, stamps = 0, hunger = 0, backoff = 0, carry = 0,
             defer = 0, dual = 0, spills = 0, hunger_init_full = 0, narrow_shed = 0;
    // ... with `comm` in bits 16..18 of its narrow_shed: the hand-off wave's
    // users (UtsKnobs::uts_comm), 0 where the launch has no such wave; `block`
    // = the threads of a workgroup, 64 x (wpg + 1) with the wave and 64 x wpg
    // without (grid and wpg count worker waves either way)
    uint32_t comm = 0;
    int block = 64;
    // SeedCfg (target 0: unseeded)
    uint32_t seed_target = 0, seed_max_levels = 0, seed_min_levels = 0, seed_solo_cap = 0;
    // what hclib_hip_uts_last_launch reports
    hclib_hip_uts_launch_t launch = {-1, 0, 0, 0, 0, 0, 0, 0, 0};
};

namespace uts_detail {
// a refusal: the message into `err`, HCLIB_HIP_EINVAL as the plan's status
__attribute__((format(printf, 2, 3))) inline int refuse(std::string &err, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return HCLIB_HIP_EINVAL;
}
}  // namespace uts_detail

// `global_attached`: the rank holds a cross-GPU region (hclib_hip_global_attach).
inline UtsPlan uts_plan(const hclib_hip_uts_params_t &p, const UtsTables &T, int num_cus, int shard, int nshards,
                        int split_depth, int max_levels, bool global_attached, const UtsKnobs &kn, std::string &err) {
    using uts_detail::refuse;
    constexpr int U = UtsKnobs::kUnset;
    (void)shard;  // every shard of a search takes the same shape
    UtsPlan P;
    if (!uts_comm_valid(kn.uts_comm, err)) {
        P.status = HCLIB_HIP_EINVAL;
        return P;
    }
    const int trace_kind = max_levels > 0 ? kn.uts_trace : 0;
    const bool trace = trace_kind != 0;

    // ---------------------------------------------------------- tree class
    P.lds_tables = (T.rules.size() <= kUtsLdsRules && T.thr.size() <= kUtsLdsThr) ? 1 : 0;
    // one GEO table for depths 1..D-1, constant 0 children from D on
    {
        const int nr = (int)T.rules.size();
        int d = 1;
        while (d < nr && T.rules[d].x == 2 && T.rules[d].z == 0) ++d;
        bool rest_zero = d > 1 && T.stationary;
        for (int e = d; e < nr && rest_zero; ++e) rest_zero = T.rules[e].x == 0 && T.rules[e].y == 0;
        if (rest_zero && T.thr.size() >= 128) P.geo_depth = d;
    }
    const bool bin = p.type == 0 && T.rules.size() == 2 && T.rules[1].x == 1 && T.stationary;
    const bool geo_fixed = !bin && P.geo_depth > 0 && kn.uts_geo_fixed;
    P.bin = bin;
    P.geo_fixed = geo_fixed;
    if (bin) P.bin_thr = (uint32_t)T.rules[1].y;
    const int mode = bin ? kUtsBin : geo_fixed ? kUtsGeoFixed : (P.lds_tables ? kUtsRulesLds : kUtsRulesGlobal);
    P.mode = mode;
    const double est = uts_expected_nodes(p);

    // the depth trace and the chain stamps exist for one kernel family only
    const bool trace_refused = trace && (mode != kUtsBin || nshards > 1);

    // -------------------------------------------------------- chunk deques
    // 128 chunk deques (8 per XCD slice of 16): T3L 28.64 -> 28.57 ms and
    // 28.73 -> 28.58, T1XL 31.19 -> 31.00, T1 0.206 -> 0.202 (means of
    // interleaved rounds, profiles/r05/sweep_dq_*.log, sweep_t3l_j.log); 32
    // is a millisecond slower on T3L
    P.nq = (uint32_t)kn.deques;
    P.deque_cap = (uint32_t)kn.deque_cap;
    P.chunk = (uint32_t)kn.chunk;

    // ------------------------------------------- waves per CU, ring, seeding
    // waves per CU: span-bound BIN trees run fastest with 2 (fewer idle
    // pollers, fewer hand-offs); GEO trees are throughput-bound and fill 8
    // (the 512-item rings leave room for them) once they are large — a
    // small tree (T1, ~4 M nodes in 1 ms) loses more to spreading its few
    // first levels over 2048 waves than it gains (profiles/r02/
    // sweep_t1xl_waves_geo.log: T1XL 90 -> 52 ms from 4 to 8, T1 1.0 ->
    // 1.45 ms). Size: uts_expected_nodes.
    // Rule-table trees (other shapes, HYBRID) of a few million nodes run
    // fastest with 4 (T2 1.80 -> 1.36 ms, T4 1.05 -> 0.86, T5 1.07 -> 0.96;
    // T2L still wants 8: profiles/r02/geo_spill.log)
    // sharded launches of a rank attached to a global region share work
    const bool global = nshards > 1 && global_attached && max_levels == 0;
    P.global = global;
    // fixed-shape trees start seeded (breadth-first, hx_sched.h seed_levels)
    const bool seed_on = geo_fixed && !global && kn.uts_seed;
    // BIN shards: the grid expands the replicated top levels breadth-first to
    // the split depth (hx_sched.h seed_levels, the shard filter inside the
    // seeding) and then runs the plain kernel of a whole-tree search. With
    // the filter in the worker loop instead (FEAT = 1) the shard holding
    // T3L's deep chain ran 2.3-2.7 ms slower than the whole tree, although
    // below the split the filter executes nothing: the FEAT = 1 body
    // compiles the span-bound narrow loop worse (the FEAT = 0 kernel on the
    // same shard: +0.05-0.14 ms; profiles/r06/shard_big_a.log)
    // (... where the levels fit the seeding's buffers: the fit test below,
    // once the grid is known)
    bool bin_seed = bin && nshards > 1 && !global && max_levels == 0 && split_depth >= 1 &&
                    split_depth + 1 < kUtsSeedMaxLevels && kn.uts_seed;
    // BIN trees: four worker waves per CU in one workgroup (one per SIMD;
    // three siblings to hand work to through LDS before the HBM deques):
    // T3L 29.08 -> 28.76 ms mean of 6 interleaved rounds against two per CU
    // in pairs, T3 2.78 -> 2.76 (profiles/r05/sweep_wpg_t3l.log,
    // sweep_wpg_t3.log; the critical chain's HBM hand-offs 560 -> 295,
    // t3l_chain_wpg.jsonl). Launches that share work across ranks keep 2
    int wpc_default = bin && !global ? 4 : 2, ring_default = 512;
    if (!bin) {
        if (seed_on) {
            // seeded: every wave starts busy, so even a small tree fills 8
            // waves per CU on 512-item rings once its seeding is cheap (round
            // 5: T1 0.234 -> 0.220 ms at 8 waves per CU and 16 slots per wave,
            // profiles/r05/sweep_t1_d.log; round 4 had 4 per CU, 0.28 vs 0.61
            // ms unseeded on 2 / 256, profiles/r04/seed*_t1.log)
            wpc_default = 8;
            ring_default = 512;
        } else {
            wpc_default = est >= 3e7 ? 8 : (geo_fixed ? 2 : 4);
            // an unseeded small tree runs faster on 256-item rings (one piece
            // per task: the frontier fans out by range splitting), a fixed-shape
            // one at 2 waves per CU: T1 0.98 -> 0.70 ms; a large one slower
            // (T1XL 52 -> 70 ms), profiles/r02/sweep_t1_ring_waves.log,
            // sweep_t1xl_ring_waves.log, geo_lds_tail.log
            ring_default = est >= 3e7 ? 512 : 256;
        }
    }
    const int grid = kn.grid > 0 ? kn.grid : num_cus * (kn.waves_per_cu != U ? kn.waves_per_cu : wpc_default);
    P.grid = grid;
    P.waves_per_cu = grid / (num_cus > 0 ? num_cus : 1);
    // (a knob value that cannot fit the ring is refused below, before the
    // launch, as check_resident refuses a grid that cannot be resident,
    // instead of ending in a device error after it)
    if (bin_seed) {
        // the seeding's fit test, as the fixed-shape one below: level d holds
        // the slots of depth d + 1, expected n(1) = the root's children and
        // n(d) = n(1) (q m)^(d - 1) below. The unfiltered levels (depths 1 ..
        // split) and this shard's part of depth split + 1 stay within half
        // the level buffer (8 x target + 65,536 slots at target = 1: wave 0
        // also truncates a root wider than the buffer), and a wave's share of
        // that last level within a quarter of its 1,024-item ring on this
        // grid (seed_levels refuses more than half). Otherwise the worker
        // loop filters (FEAT = 1), which needs no level buffers.
        const double cap = 8.0 * 1 + 65536.0;
        const double qm = p.non_leaf_prob * bin_rule_m(p) > 0 ? p.non_leaf_prob * bin_rule_m(p) : 0.0;
        double n = T.root_nc > 0 ? (double)T.root_nc : 0.0, widest = n;
        for (int d = 2; d <= split_depth; ++d) {
            n *= qm;
            if (n > widest) widest = n;
        }
        const double n_mine = n * qm / nshards;
        if (!(widest <= 0.5 * cap && n_mine <= 0.5 * cap && n_mine <= (double)grid * (1024 / 4))) bin_seed = false;
    }
    P.spill_hi = (uint32_t)kn.spill_hi;
    // BIN trees with the narrow-frontier loop give work away from 72 items
    // (just over one batch: a wave keeps at most ~one batch of a narrow
    // frontier, T3L 36.3 -> 35.0 ms, profiles/r02/t3l_knobs.log). GEO trees
    // keep far more before feeding hungry waves (fewer, fuller hand-offs;
    // profiles/r02/geo_spill.log): 224 with rule tables (T2 2.82 -> 1.71 ms,
    // T5 1.40 -> 1.00, T2L 6.33 -> 5.20) and on the fixed-shape 512-item rings
    // at one piece per task (T1XL 37.2 ms, T1L 3.77; profiles/r02/
    // pieces_tune.log; 336 at five pieces), 128 on 256-item rings (T1)
    // (the ring knob: whole-tree launches only — sharded and histogram
    // launches size spill_lo and the seeding's fit check for 512-item rings)
    const int ring_used = geo_fixed && !(nshards > 1 || max_levels > 0) ? (kn.uts_ring != U ? kn.uts_ring : ring_default)
                                                                       : 512;
    if (ring_used != 256 && ring_used != 512 && ring_used != 1024) {
        P.status = refuse(err,
                          "hclib_hip_uts_search: HCLIB_HIP_UTS_RING=%d is not a ring the search is built for (256, 512 "
                          "or 1024 items per wave)", ring_used);
        return P;
    }
    // BIN trees: 66 since the register carry went through LDS (T3L 30.64 ->
    // 30.20 ms same-box against 72, profiles/r04/sc_ab_t3l*.log, t3l3_spill.log);
    // it must stay above one batch (64) or the narrow loop never runs
    int spill_lo_default = bin ? 66 : (geo_fixed && ring_used < 512) ? 128 : 224;
    // seeded fixed-shape trees (below) start with every wave busy, so a wave
    // keeps more before it feeds others: T1 0.285 -> 0.248 ms at 336, T1L
    // 2.70 -> 2.38, T1XL's 8-way shards 4.94 -> 4.75 at 448
    // (profiles/r04/seed5_*.log, seed6_*.log)
    // slots per wave: a few for a small tree (one level fewer to expand),
    // more for a large one (finer shares, less stealing later;
    // profiles/r04/seed3_*.log, seed4_*.log)
    // (16 for small trees since round 5: one level deeper, T1 0.234 ->
    // 0.220 ms, profiles/r05/sweep_t1_d.log; a level holds at most ~b x
    // the target, so 32 keeps a wave's share of a b = 4 level within
    // half its ring)
    const int per_wave = kn.seed_per_wave != U ? kn.seed_per_wave : (est >= 3e7 ? 32 : 16);
    bool seed_fits = seed_on && ring_used >= 512;
    if (seed_fits) {
        // the seeding stops at the first level of at least the target, which
        // the level before it (below the target) reaches b-fold: a wave's
        // share comes to b x per_wave items, and seed_levels takes at most
        // half a ring. A knob value past that is refused (the defaults are
        // measured shapes and stay as they are)
        if (kn.seed_per_wave_set) {
            const double b = geo_bi(p, 1) > kUtsMaxChildren ? (double)kUtsMaxChildren : geo_bi(p, 1);
            if (per_wave < 1) {
                P.status = refuse(err,
                                  "hclib_hip_uts_search: HCLIB_HIP_SEED_PER_WAVE=%d is not a slot count (1 or more; "
                                  "HCLIB_HIP_UTS_SEED=0 turns the seeding off)", per_wave);
                return P;
            }
            if (b * per_wave > ring_used / 2) {
                P.status = refuse(err,
                                  "hclib_hip_uts_search: HCLIB_HIP_SEED_PER_WAVE=%d cannot fit the ring: a wave's share "
                                  "of the seeded level reaches %.0f x %d items, the seeding hands over at most %d of a "
                                  "%d-item ring", per_wave, b, per_wave, ring_used / 2, ring_used);
                return P;
            }
        }
        // ... and the launch is seeded only where that level fits, by the
        // expected level sizes n(1) = the root's children, n(d + 1) = n(d) b_d:
        // the first level of at least the target within half the level
        // buffer (8 x target + 65,536 slots) and a wave's share of it within
        // a quarter of its ring, on this grid. (Always so at b = 4 with the
        // default slots per wave; not for a wide tree on a small grid: b = 40
        // on 4 waves passes a 63-slot level, one short of the target, and
        // shares out the 2,177 slots of the next.) A tree that ends below the
        // target is expanded by the seeding alone. Otherwise the search
        // starts unseeded, from the root.
        const double target = (double)grid * per_wave, cap = 8.0 * target + 65536.0;
        double n = T.root_nc > 0 ? (double)T.root_nc : 0.0;
        for (int d = 1; d < 64 && n > 0.0 && n < target; ++d) {
            const double b = geo_bi(p, d) > kUtsMaxChildren ? (double)kUtsMaxChildren : geo_bi(p, d);
            n *= b > 0.0 ? b : 0.0;
        }
        seed_fits = n <= 0.5 * cap && n <= (double)grid * (ring_used / 4);
    }
    const bool seeded = seed_fits;
    if (seeded) spill_lo_default = est >= 3e7 ? 448 : 336;
    {
        // a wave never holds more than its ring: a threshold past it would
        // keep every wave from ever feeding a hungry one
        const int ring_launch = bin ? 1024 : ring_used, lo = kn.spill_lo != U ? kn.spill_lo : spill_lo_default;
        if (lo < 1 || lo > ring_launch) {
            P.status = refuse(err,
                              "hclib_hip_uts_search: HCLIB_HIP_SPILL_LO=%d does not fit the %d-item ring of this launch "
                              "(1..%d)", lo, ring_launch, ring_launch);
            return P;
        }
        P.spill_lo = (uint32_t)lo;
    }
    P.spin_limit = (uint32_t)kn.spin_limit_ms;
    P.nwaves = (uint32_t)grid;
    P.stamps = (uint32_t)kn.stamps;
    // hunger read every 32 batches, every 8 while many waves are hungry
    // (scripts/sweep_uts.py: T1 1.37 -> 1.07 ms, T1XL 101 -> 97 ms, T3L even)
    // (fixed-shape GEO trees on 512-item rings every 64: T1XL 51.5 -> 49.9 ms,
    // T1L even, T2L slower; profiles/r02/geo_knobs.log)
    // hunger read interval: 64 batches on BIN trees (T3L 29.34 -> 29.23 ms mean of 7 interleaved rounds, and
    // -0.14 ms in two shorter sweeps: profiles/r05/sweep_h64sp1_t3l.log,
    // sweep_wpg4_t3l.log, sweep_spills_t3l.log), 32 otherwise
    // ... except small fixed-shape trees (expected < 3e7 nodes), which run
    // a few dozen batches per wave: 32 (T1 0.210 -> 0.200-0.201 ms mean of 6
    // and 8 interleaved rounds; T1L wants 64: 2.44 vs 2.48 ms;
    // profiles/r05/sweep_t1_g.log, sweep_t1_h.log, sweep_t1l_h.log)
    // ... and large fixed-shape trees every 128 (T1XL 31.15 -> 30.77 ms, T1L
    // 2.417 -> 2.383, means of 4-5 interleaved rounds, sweep_t1xl_l.log,
    // sweep_t1l_l.log)
    const bool small_fixed = geo_fixed && est < 3e7;
    const bool large_fixed = geo_fixed && ring_used >= 512 && !small_fixed;
    P.hunger = (uint32_t)(kn.hunger != U ? kn.hunger : large_fixed ? 128 : bin ? 64 : 32);
    P.carry = (uint32_t)kn.carry;
    P.backoff = (uint32_t)kn.backoff;
    P.defer = (uint32_t)kn.defer;
    // dual batches (two nodes per lane while a wave holds > 64 items; kinds
    // whose ring fits two batches' pushes: the fixed-shape GEO trees on
    // 512-item rings)
    P.dual = (uint32_t)kn.uts_dual;
    P.spills = (uint32_t)kn.spills_per_batch;
    // the narrow loop's overflow exit (hx_sched.h narrow_shed; BIN trees in
    // workgroups of 2 or 4 waves): HCLIB_HIP_NARROW_SHED = 0 every child onto
    // the ring and back to the main loop, 1 keep half the level's spawners and
    // hand the others' children to idle siblings, 2 keep as many as fit one
    // batch, 3 keep a quarter; HCLIB_HIP_NARROW_SHED_SIBS = the sibling
    // inboxes one exit may fill (0: none, every exit falls back to the ring)
    {
        const int rule = kn.narrow_shed, sibs = kn.narrow_shed_sibs;
        if (rule < 0 || rule > 3 || sibs < 0 || sibs > 3) {
            P.status = refuse(err,
                              "hclib_hip_uts_search: HCLIB_HIP_NARROW_SHED=%d / HCLIB_HIP_NARROW_SHED_SIBS=%d: the keep "
                              "rule is 0 (off), 1, 2 or 3, the sibling inboxes per exit 0..3", rule, sibs);
            return P;
        }
        P.narrow_shed = (uint32_t)rule | (uint32_t)sibs << 8;
    }
    if (trace_refused) {
        P.status = refuse(err, "hclib_hip_uts_search: the depth trace is for unsharded BIN trees");
        return P;
    }
    // breadth-first seeding (hx_sched.h seed_levels) for fixed-shape GEO
    // trees: the grid expands the top levels together and shares the level
    // that reaches HCLIB_HIP_SEED_PER_WAVE slots per wave out evenly, instead
    // of growing the busy set from one root by hand-offs
    if (seeded) {
        P.seed_target = (uint32_t)(grid * per_wave);
        P.seed_max_levels = (uint32_t)kn.seed_levels;
        // wave 0 alone runs the levels of at most 128 slots (its ring's room
        // is 224): a level of 189 (T1's depth 3) is cheaper on the grid
        // (T1 median 0.2051-0.2067 -> 0.1976-0.2011 ms over 18 + 40 launches,
        // T1L 2.490 -> 2.465; profiles/r06/sweep_t1_solo*.log)
        P.seed_solo_cap = (uint32_t)kn.seed_solo;
        // a shard's share is only known past its split (level d holds the
        // slots of depth d + 1, filtered when they run), so the seeding goes
        // on to the split — where the levels up to it fit the seeding's
        // buffers (expected sizes n(d) = prod b_k): the unfiltered level
        // (n(split) slots) within half the level buffer, and this shard's
        // share of the level past it within a quarter of each wave's ring
        // (hx_sched.h seed_levels: the buffer holds 8 x target + 65,536
        // slots, a wave takes at most CAP / 2 items). Deeper splits seed
        // only to the target and filter in the worker loop (FEAT = 1).
        if (nshards > 1) {
            double n_split = 1.0, n_next = 1.0;
            for (int d = 0; d <= split_depth && d < 64; ++d) {
                if (d < split_depth) n_split *= geo_bi(p, d) > 0 ? geo_bi(p, d) : 0.0;
                n_next *= geo_bi(p, d) > 0 ? geo_bi(p, d) : 0.0;
            }
            const double cap = 8.0 * P.seed_target + 65536.0;
            const bool fits = split_depth + 1 < kUtsSeedMaxLevels && split_depth < (int)P.seed_max_levels &&
                              n_split <= 0.5 * cap && n_next / nshards <= (double)grid * (512 / 8);
            P.seed_min_levels = fits ? (uint32_t)split_depth : 0u;
        }
    } else if (bin_seed) {
        // exactly the split's levels: a BIN level holds ~b0 slots (critical
        // branching, sd ~ sqrt(b0 d m^2 q (1 - q))), far inside the buffer
        P.seed_target = 1;
        P.seed_max_levels = (uint32_t)split_depth;
        P.seed_min_levels = (uint32_t)split_depth;
    }

    // -------------------------------------------------------------- kernel
    // a sharded search whose seeding reaches past its split (every seeded
    // fixed-shape shard with split < the seeding's level bound) filters its
    // shard inside the seeding (UtsKind::seed_process) and then runs the
    // plain kernel; otherwise the worker loop itself filters (FEAT = 1)
    const bool seed_past_split = P.seed_target && nshards > 1 && P.seed_min_levels == (uint32_t)split_depth;
    const bool filter = max_levels > 0 || (nshards > 1 && (global || !seed_past_split));
    P.feat = trace ? (trace_kind == 2 ? 3 : 2) : (filter ? 1 : 0);
    // ring items per wave: 1024 on BIN trees, 512 otherwise; the ring-size
    // variants of the fixed-shape GEO search are whole-tree launches
    P.ring = mode == kUtsBin ? 1024 : 512;
    if (mode == kUtsGeoFixed && !filter && !global) P.ring = ring_used;
    // BIN trees: the worker waves of a CU share a workgroup and hand work
    // to each other through LDS before the HBM deques (two: T3L 34.0 ->
    // 33.5-33.7 ms, profiles/r02/inbox_ab.log; four since round 5, see
    // wpc_default; HCLIB_HIP_WPG = 1, 2 or 4). The depth trace runs one wave
    // per workgroup; launches that share work across ranks do too
    if (mode == kUtsBin && !global && (!trace || trace_kind == 2)) {
        P.wpg = kn.wpg;
        if (P.wpg != 2 && P.wpg != 4) P.wpg = 1;
        if (grid % P.wpg) P.wpg = 1;
    }
    // the hand-off wave: where the workgroup has siblings to hand off for and
    // the kernel can run one (uts_block_waves: never a launch that shares
    // across ranks; the depth trace runs lone waves, the chain stamps keep it)
    if (P.wpg > 1 && uts_block_waves(P.wpg, global) > P.wpg) P.comm = (uint32_t)kn.uts_comm;
    // (narrow_shed fills a block with up to one batch of items, and the wave
    // enqueues a block as one chunk: with smaller chunks that user stays off)
    if (kn.chunk < 64) P.comm &= ~2u;
    P.block = 64 * (P.wpg + (P.comm ? 1 : 0));
    P.launch = hclib_hip_uts_launch_t{mode, trace ? 1 + trace_kind : P.feat, P.wpg, grid, P.ring, P.seed_target ? 1 : 0, (int)P.seed_target,
                                      (int)P.spill_lo, P.waves_per_cu};
    return P;
}

}  // namespace hx
