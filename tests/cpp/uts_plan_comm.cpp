// The hand-off wave in the UTS launch plan (hclib_amd/csrc/hx_uts_plan.h):
// when HCLIB_HIP_UTS_COMM turns the wave on, by tree class, workers per
// workgroup, a launch that shares across ranks and the traces; the workgroup
// size that follows (64 more threads with the wave, grid and wpg counting
// worker waves either way); that the rest of the plan does not move with the
// knob; and that a value outside 0..7 is refused by the plan's first check,
// with its own text, whatever else the launch asks for. The expected rows
// restate the rule of the issue (a BIN tree's workgroup of 2 or 4 workers,
// not GLOBAL, not the depth trace), not the header's expressions.
// Built with -fsanitize=address,undefined by tests/test_uts_plan_comm.py.
#include "hx_uts_plan.h"

#include <stdlib.h>
#include <string.h>

using namespace hx;

namespace {

const char *kT3 = "-t 0 -b 2000 -q 0.124875 -m 8 -r 42";     // BIN
const char *kT1 = "-t 1 -a 3 -d 10 -b 4 -r 19";              // fixed-shape GEO
const char *kT2 = "-t 1 -a 2 -d 16 -b 6 -r 502";             // rule tables
const char *kT4 = "-t 2 -a 0 -d 16 -b 6 -r 1 -q 0.234375 -m 4 -r 1";  // HYBRID

struct Case {
    const char *name, *args;
    int nshards, split, max_levels, attached;
    int wpg_knob, grid_knob, trace, comm;
    int want_status, want_wpg, want_global;
    uint32_t want_comm;
    int want_block;
};

const Case kCases[] = {
    // BIN, whole tree, four workers per workgroup: every knob value is carried, the block grows by one wave
    {"T3 comm 0", kT3, 1, 0, 0, 0, 4, 0, 0, 0, 0, 4, 0, 0u, 256},
    {"T3 comm 1", kT3, 1, 0, 0, 0, 4, 0, 0, 1, 0, 4, 0, 1u, 320},
    {"T3 comm 2", kT3, 1, 0, 0, 0, 4, 0, 0, 2, 0, 4, 0, 2u, 320},
    {"T3 comm 3", kT3, 1, 0, 0, 0, 4, 0, 0, 3, 0, 4, 0, 3u, 320},
    {"T3 comm 4", kT3, 1, 0, 0, 0, 4, 0, 0, 4, 0, 4, 0, 4u, 320},
    {"T3 comm 7", kT3, 1, 0, 0, 0, 4, 0, 0, 7, 0, 4, 0, 7u, 320},
    // pairs
    {"T3 wpg 2 comm 0", kT3, 1, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 0u, 128},
    {"T3 wpg 2 comm 3", kT3, 1, 0, 0, 0, 2, 0, 0, 3, 0, 2, 0, 3u, 192},
    // lone waves: by the knob, by a value the kernel table does not hold, by a grid the workgroups do not divide
    {"T3 wpg 1 comm 7", kT3, 1, 0, 0, 0, 1, 0, 0, 7, 0, 1, 0, 0u, 64},
    {"T3 wpg 3 comm 7", kT3, 1, 0, 0, 0, 3, 0, 0, 7, 0, 1, 0, 0u, 64},
    {"T3 grid 6 comm 7", kT3, 1, 0, 0, 0, 4, 6, 0, 7, 0, 1, 0, 0u, 64},
    {"T3 grid 8 comm 7", kT3, 1, 0, 0, 0, 4, 8, 0, 7, 0, 4, 0, 7u, 320},
    // sharded and histogram launches of a BIN tree keep their workgroups, and so the wave
    {"T3 2 shards comm 3", kT3, 2, 1, 0, 0, 4, 0, 0, 3, 0, 4, 0, 3u, 320},
    {"T3 histogram comm 3", kT3, 1, 0, 40, 0, 4, 0, 0, 3, 0, 4, 0, 3u, 320},
    // a launch that shares work across ranks runs lone waves: never a hand-off wave
    {"T3 2 shards attached comm 7", kT3, 2, 1, 0, 1, 4, 0, 0, 7, 0, 1, 1, 0u, 64},
    // traces: the depth trace runs lone waves, the chain stamps keep the workgroup and the wave
    {"T3 depth trace comm 7", kT3, 1, 0, 40, 0, 4, 0, 1, 7, 0, 1, 0, 0u, 64},
    {"T3 chain stamps comm 7", kT3, 1, 0, 40, 0, 4, 0, 2, 7, 0, 4, 0, 7u, 320},
    {"T3 chain stamps comm 0", kT3, 1, 0, 40, 0, 4, 0, 2, 0, 0, 4, 0, 0u, 256},
    // the other tree classes run lone waves whatever the knobs say
    {"T1 comm 7", kT1, 1, 0, 0, 0, 4, 0, 0, 7, 0, 1, 0, 0u, 64},
    {"T2 comm 7", kT2, 1, 0, 0, 0, 4, 0, 0, 7, 0, 1, 0, 0u, 64},
    {"T4 comm 7", kT4, 1, 0, 0, 0, 4, 0, 0, 7, 0, 1, 0, 0u, 64},
    // refused: not a set of the three bits; on every tree class, before any other knob is looked at
    {"T3 comm 8", kT3, 1, 0, 0, 0, 4, 0, 0, 8, HCLIB_HIP_EINVAL, 0, 0, 0u, 0},
    {"T3 comm -1", kT3, 1, 0, 0, 0, 4, 0, 0, -1, HCLIB_HIP_EINVAL, 0, 0, 0u, 0},
    {"T3 comm 1000", kT3, 1, 0, 0, 0, 4, 0, 0, 1000, HCLIB_HIP_EINVAL, 0, 0, 0u, 0},
    {"T1 comm 8", kT1, 1, 0, 0, 0, 4, 0, 0, 8, HCLIB_HIP_EINVAL, 0, 0, 0u, 0},
    {"T3 wpg 1 comm 9", kT3, 1, 0, 0, 0, 1, 0, 0, 9, HCLIB_HIP_EINVAL, 0, 0, 0u, 0},
};

// the UTS command line over the T1 defaults (as tests/cpp/uts_plan.cpp)
hclib_hip_uts_params_t parse_args(const char *args) {
    hclib_hip_uts_params_t p;
    p.type = 1;
    p.shape_fn = 3;
    p.gen_mx = 10;
    p.b_0 = 4.0;
    p.root_id = 19;
    p.non_leaf_bf = 4;
    p.non_leaf_prob = 15.0 / 64.0;
    p.shift_depth = 0.5;
    p.compute_gran = 1;
    char buf[256];
    snprintf(buf, sizeof(buf), "%s", args);
    for (char *f = strtok(buf, " "); f; f = strtok(nullptr, " ")) {
        const char *v = strtok(nullptr, " ");
        switch (f[1]) {
        case 'q': p.non_leaf_prob = atof(v); break;
        case 'm': p.non_leaf_bf = atoi(v); break;
        case 'r': p.root_id = atoi(v); break;
        case 't': p.type = atoi(v); break;
        case 'a': p.shape_fn = atoi(v); break;
        case 'b': p.b_0 = atof(v); break;
        case 'd': p.gen_mx = atoi(v); break;
        case 'f': p.shift_depth = atof(v); break;
        default: printf("unknown flag %s\n", f); exit(2);
        }
    }
    return p;
}

#define CHECK(what, got, want)                                                 \
    do {                                                                       \
        const long long g_ = (long long)(got), w_ = (long long)(want);         \
        if (g_ != w_) {                                                        \
            printf("  MISMATCH %s: plan %lld, expected %lld\n", what, g_, w_); \
            ++bad;                                                             \
        }                                                                      \
    } while (0)

}  // namespace

int main() {
    int ncases = 0, all_bad = 0;
    static_assert(uts_block_waves(1, false) == 1 && uts_block_waves(2, false) == 3 && uts_block_waves(4, false) == 5,
                  "a workgroup with siblings has room for the hand-off wave");
    static_assert(uts_block_waves(1, true) == 1 && uts_block_waves(2, true) == 2 && uts_block_waves(4, true) == 4,
                  "a sharing launch's kernels have none");
    for (const Case &c : kCases) {
        const hclib_hip_uts_params_t p = parse_args(c.args);
        UtsTables T;
        std::string err;
        if (build_tables(p, T, err) != HCLIB_HIP_OK) {
            printf("%s: build_tables: %s\n", c.name, err.c_str());
            return 2;
        }
        UtsKnobs kn;
        kn.wpg = c.wpg_knob;
        kn.grid = c.grid_knob;
        kn.uts_trace = c.trace;
        kn.uts_comm = c.comm;
        err.clear();
        const UtsPlan P = uts_plan(p, T, 256, 0, c.nshards, c.split, c.max_levels, c.attached != 0, kn, err);
        int bad = 0;
        CHECK("status", P.status, c.want_status);
        if (c.want_status) {
            // the refusal names the knob and its value, and nothing was planned
            char want[64];
            snprintf(want, sizeof(want), "HCLIB_HIP_UTS_COMM=%d ", c.comm);
            if (err.find(want) == std::string::npos) {
                printf("  MISMATCH error text: \"%s\" does not name %s\n", err.c_str(), want);
                ++bad;
            }
            CHECK("grid of a refused plan", P.grid, 0);
            CHECK("nq of a refused plan", P.nq, 0);
            // ... also beside a knob that is refused itself: the hand-off knob's check comes first
            UtsKnobs k2 = kn;
            k2.narrow_shed = 9;
            std::string e2;
            const UtsPlan P2 = uts_plan(p, T, 256, 0, c.nshards, c.split, c.max_levels, c.attached != 0, k2, e2);
            CHECK("status beside a second bad knob", P2.status, HCLIB_HIP_EINVAL);
            if (e2 != err) {
                printf("  MISMATCH the first refusal is not the hand-off knob's: \"%s\"\n", e2.c_str());
                ++bad;
            }
            std::string e3;
            CHECK("uts_comm_valid", uts_comm_valid(c.comm, e3), false);
        } else {
            if (!err.empty()) {
                printf("  MISMATCH error text of an accepted plan: \"%s\"\n", err.c_str());
                ++bad;
            }
            CHECK("wpg", P.wpg, c.want_wpg);
            CHECK("global", P.global, c.want_global);
            CHECK("comm", P.comm, c.want_comm);
            CHECK("block", P.block, c.want_block);
            CHECK("block = 64 (wpg + wave)", P.block, 64 * (P.wpg + (P.comm ? 1 : 0)));
            CHECK("block within the kernel's launch bounds", P.block <= 64 * uts_block_waves(P.wpg, P.global), 1);
            CHECK("grid counts worker waves", P.grid % P.wpg, 0);
            CHECK("launch.workers_per_group", P.launch.workers_per_group, P.wpg);
            CHECK("launch.grid", P.launch.grid, P.grid);
            CHECK("nwaves", P.nwaves, (uint32_t)P.grid);
            // the knob moves nothing else: the same launch with the wave off
            UtsKnobs k0 = kn;
            k0.uts_comm = 0;
            std::string e0;
            const UtsPlan Q = uts_plan(p, T, 256, 0, c.nshards, c.split, c.max_levels, c.attached != 0, k0, e0);
            CHECK("comm of the launch with the knob 0", Q.comm, 0);
            CHECK("block of the launch with the knob 0", Q.block, 64 * P.wpg);
            CHECK("same kernel", Q.mode == P.mode && Q.feat == P.feat && Q.ring == P.ring && Q.global == P.global &&
                                     Q.wpg == P.wpg && Q.grid == P.grid, 1);
            CHECK("same narrow_shed word", Q.narrow_shed, P.narrow_shed);
            CHECK("narrow_shed leaves bits 16.. to the wave's users", P.narrow_shed >> 16, 0);
            CHECK("same pool", Q.nq == P.nq && Q.deque_cap == P.deque_cap && Q.chunk == P.chunk, 1);
            CHECK("same thresholds", Q.spill_lo == P.spill_lo && Q.spill_hi == P.spill_hi && Q.hunger == P.hunger, 1);
            CHECK("same launch record", memcmp(&Q.launch, &P.launch, sizeof(P.launch)), 0);
        }
        printf("%s: %s\n", c.name, bad ? "FAILED" : "ok");
        all_bad += bad;
        ++ncases;
    }
    printf("%d cases\n", ncases);
    printf("Check results: %s\n", all_bad ? "FAILED" : "OK");
    return all_bad ? 1 : 0;
}
