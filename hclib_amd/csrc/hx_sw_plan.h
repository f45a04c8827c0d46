// hx_sw_plan.h — which of sw.hip's six launch paths a Smith-Waterman run
// takes, and everything the paths differ in, in plain C++: no HIP and no
// getenv, so a host program can check the decision (tests/cpp/sw_plan.cpp).
// sw.hip reads the environment into SwKnobs, plans, and launches the plan.
#pragma once

#include <stddef.h>

#include "../../include/hclib_hip.h"

namespace hx {

// ---------------------------------------------------------------- LDS bytes
// The one-wave tile (k_sw, SwDagKind::run, k_sw_rows): top row | bottom row |
// 64 dummy words (+ 4) | with `rows` the left and right columns | s1 as bytes,
// twice, + 16. Those kernels' prologues spell the same offsets out (taking
// them from here changed the generated code): keep both in step.
constexpr size_t sw_tile_lds_bytes(int tw, int th, bool rows) {
    return 2 * (size_t)(((tw + 1 + 3) & ~3) * 4) + 68 * 4 + 2 * (size_t)((tw + 3) & ~3) + 16 +
           (rows ? 2 * (size_t)(((th + 3) & ~3) * 4) : 0);
}

// The multi-wave band kernels (sw.hip, "multi-wave tile rows").
constexpr int kSwRing = 512;  // columns per inter-wave ring (+1 wrap slot)
constexpr int kSwRingStride = kSwRing + 4;
// dummy ring slots per compute wave (its lanes 0..62 write there every step
// while lane 63 writes the out ring; lane stride 1: neighbours' two-dword
// writes overlap, which measured no slower than stride 2)
constexpr int kSwDummy = 128;
constexpr size_t sw_band_lds_bytes(int nw) {
    return (size_t)(nw + 1) * kSwRingStride * 4  // rings
           + (size_t)nw * kSwDummy * 4            // per-wave dummy slots (lanes 0..62's ring writes)
           + (size_t)nw * 2048                    // per-wave code rings: 4 byte-shifted copies, double-mapped
           + 2 * 64 * 4;                          // prod / cons words
}

// The packed-half body (sw.hip, k_sw_dag_pk).
constexpr int kSwPkTh = 256;     // tile rows the packed body covers
constexpr int kSwPkMaxTw = 512;  // f16 exactness bound (sw.hip, above the packed body)
// LDS words of the packed body's arrays for tiles ncols wide: the top row
// (x < ncols + 196, zeros past the tile) and four copies of the per-column
// permute selectors (x in [-64, ncols + 200)), copy o at word x + 64 + o
constexpr int sw_pk_topw(int ncols) { return (ncols + 196 + 3) & ~3; }
constexpr int sw_pk_selw(int ncols) { return (ncols + 268 + 3) & ~3; }
// Ring: kSwPkSlots chunks of 64 steps; a chunk is 32 step pairs x 64 lanes of
// uint4 {sc0(2p), sc1(2p), sc0(2p+1), sc1(2p+1)}. misc[5] = chunks written,
// misc[6] = chunks read (both reset between tiles).
constexpr int kSwPkSlots = 2;
constexpr int kSwPkRingU4 = kSwPkSlots * 32 * 64;  // uint4 entries
// LDS: ring | top | sel x 4 | right columns [2][256] | misc[16] | score rows [4][64] | next top row [512]
constexpr int kSwPkMisc = 16;
constexpr int sw_pk_lds_words(int tw) {
    return kSwPkRingU4 * 4 + sw_pk_topw(tw) + 4 * sw_pk_selw(tw) + 2 * kSwPkTh + kSwPkMisc + 256 + kSwPkMaxTw;
}
constexpr size_t sw_pk_lds_bytes(int tw) { return (size_t)sw_pk_lds_words(tw) * 4; }

// ------------------------------------------------------------------- knobs
// HCLIB_HIP_SW_SCHED: "rows" (the default, and any other word) = owner-computes
// tile rows with granule hand-offs; "rows1" = the same with the
// one-wave-per-tile-row kernel; "queue" = dependency counters + a ready list;
// "dag" = the reference's three promises per tile on the generic promise DAG.
enum class SwSched { Rows, Rows1, Queue, Dag };

// The environment knobs' values (sw.hip's sw_knobs() reads them); a member's
// default is the knob's.
struct SwKnobs {
    static constexpr int kUnset = -0x7fffffff;
    SwSched sched = SwSched::Rows;
    // HCLIB_HIP_SW_<NAME>. form 0 (not a form): the path's default, see
    // sw_plan; waves_per_cu unset: 1 under the row schedule, else 2
    int form = 0, pk = 1, dag_wave = 0, progressive = 1, rows_per_wg = 1, waves_per_cu = kUnset;
    int pk_wgs_per_cu = 1, dag_wgs_per_cu = 1;
};

// ------------------------------------------------ the band kernels' rules
// the multi-wave kernel's shape: bands of bh = 64, 128 or 256 rows, 1..14
// compute waves per tile row (+ the ingress and egress waves)
inline bool sw_band_ok(int th, int bh) { return th % bh == 0 && th / bh >= 1 && th / bh <= 14; }
// 100 R + 10 S + K / 16 (rows per lane, skew, hand-off steps) asked for
// (`def` when `form` is none of the 11), kept to a valid form for th: four
// rows per lane need th % 256 == 0, two th % 128 == 0, else fewer rows per
// lane with the same skew and hand-off
inline int sw_pick_form(int th, int def, int form) {
    if (form != 11 && form != 12 && form != 14 && form != 21 && form != 22 && form != 211 && form != 212 &&
        form != 214 && form != 411 && form != 412 && form != 414)
        form = def;
    if (form > 400 && th % 256 != 0) form -= 200;
    if (form > 200 && th % 128 != 0) form -= 200;
    return form;
}
inline int sw_form_bh(int form) { return 64 * (form > 100 ? form / 100 : 1); }
// tile rows per workgroup (HCLIB_HIP_SW_ROWS_PER_WG, default 1): more share
// the CU's SIMDs between more waves and measured slower (scripts/probe_sw.py)
inline int sw_band_rows_per_wg(int th, int bh, int k) {
    const int most = 14 / (th / bh);
    return k < 1 ? 1 : (k > most ? most : k);
}

// -------------------------------------------------------------------- plan
enum class SwKernel { Queue, DagWave, DagWg, DagPk, Rows1Progressive, Rows1Whole, BandRows };

// One allocation: every array on a 256-byte boundary, then 1024 bytes of
// counters (ready tail / head, error word, stats). 0 bytes: no such array.
struct SwBytes {
    size_t s1, s2, bottom, right, corner, deps, ready, gbot, gright, gcorner;
    static constexpr size_t kMisc = 1024;
    static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
    size_t total() const {
        return al(s1) + al(s2) + al(bottom) + al(right) + al(corner) + al(deps) + al(ready) + al(gbot) + al(gright) +
               al(gcorner) + kMisc;
    }
};

struct SwPlan {
    bool too_large;  // the one-wave tile passes the CU's 160 KiB of LDS: nothing else is set
    // HCLIB_HIP_SW_PATH_*; the band kernels' form and band height
    int path, form, bh;
    SwKernel kernel;
    size_t lds;  // dynamic LDS bytes per workgroup
    // threads per workgroup. grid: workgroups of the queue, and of the row
    // schedule over all nth tile rows; on the DAG (grid 0) wgs_per_cu
    // workgroups per CU for hclib_hip_dag_begin. Row schedule: tile rows per
    // workgroup and the most workgroups of one launch (all resident, so every
    // granule wait ends)
    int threads, grid, wgs_per_cu, rows_per_wg, grid_cap;
    SwBytes bytes;

    void use(int path_, SwKernel k, int threads_, size_t lds_) { path = path_, kernel = k, threads = threads_, lds = lds_; }
    bool rows() const { return path == HCLIB_HIP_SW_PATH_ROWS1 || path == HCLIB_HIP_SW_PATH_BAND_ROWS; }
    bool dag() const { return path >= HCLIB_HIP_SW_PATH_DAG_WAVE; }
    bool pk() const { return path == HCLIB_HIP_SW_PATH_DAG_PK; }
    // workgroups of a row-schedule launch over `nrows` tile rows
    int rows_grid(int nrows) const {
        const int nblk = (nrows + rows_per_wg - 1) / rows_per_wg;
        return nblk < grid_cap ? nblk : grid_cap;
    }
};

// hclib_hip_sw / hclib_hip_sw_edges over ntw x nth tiles of tw x th, or with
// `session` a column-band session (hclib_hip_sw_band_begin, which has checked
// that the row layout fits 64 KiB): always the row schedule, form 412 by
// default, only "rows1" selects the one-wave kernel, HCLIB_HIP_SW_WAVES_PER_CU
// is not consulted, and the band keeps s1, s2 and its bottom rows' granules.
inline SwPlan sw_plan(int tw, int th, size_t ntw, size_t nth, int num_cus, const SwKnobs &kn, bool session = false) {
    SwPlan p{};
    const bool dag = !session && kn.sched == SwSched::Dag;
    // the row schedule keeps two tile columns in LDS: wide tiles fall back to
    // the queue (even where the band kernel, which keeps none, would run)
    const bool rows = session || (!dag && kn.sched != SwSched::Queue && sw_tile_lds_bytes(tw, th, true) <= 64 * 1024);
    // multi-wave band form (sw_pick_form): the DAG's tile tasks default to two
    // rows per lane (two waves per 256-row tile: one hand-off lag instead of
    // three), the row schedule to four (one band per 256-row tile row: the
    // per-row wavefront lag is paid once per 256 rows). SW-64K measured
    // (profiles/r02/sw_forms.log): rows 12: 4.4 ms, 212: 3.55, 412: 3.50;
    // dag 12: 11.2, 212: 9.4, 412: 9.6. Round 3, same box
    // (profiles/r03/sw_forms_k64.log): hand-offs every 64 steps for the DAG's
    // tiles, 212: 8.35 -> 214: 8.12-8.14 ms; rows 414 3.56 vs 412 3.49-3.51
    p.form = sw_pick_form(th, dag ? 214 : 412, kn.form);
    p.bh = sw_form_bh(p.form);
    const int nw = th / p.bh;
    const bool band_shape = sw_band_ok(th, p.bh) && tw <= 65536;
    // the promise DAG's 256-row tiles at most 512 wide: the packed-half body,
    // tagged outputs (HCLIB_HIP_SW_PK=0: the band forms)
    // (a two-sweep-wave body was exact but slower, 7.95 vs 6.56 ms, and was
    // removed in round 5: DESIGN.md Appendix A)
    const bool pk = dag && th == kSwPkTh && tw <= kSwPkMaxTw && kn.pk != 0;

    // the one-wave tile's LDS bounds every path, and the waves per CU of the
    // paths that run it
    const size_t one = sw_tile_lds_bytes(tw, th, rows);
    if ((p.too_large = one > 160 * 1024)) return p;
    // rows: one wave per CU owns tile rows (all resident, so every wait ends)
    int per_cu = kn.waves_per_cu;  // workgroups per CU: of one wave here, of a path's own below
    if (session || per_cu == SwKnobs::kUnset) per_cu = rows ? 1 : 2;
    if (per_cu > (int)((160 * 1024) / one)) per_cu = (int)((160 * 1024) / one);
    // the generic promise DAG launches at most 8 waves per CU
    // (hclib_hip_dag_begin); clamp here rather than fail its argument check
    if (dag && per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;

    p.rows_per_wg = 1;
    if (rows && band_shape && kn.sched != SwSched::Rows1) {
        // multi-wave tile rows (+ the ingress and egress waves) unless "rows1"
        // asks for the one-wave-per-tile-row kernel
        p.rows_per_wg = sw_band_rows_per_wg(th, p.bh, kn.rows_per_wg);
        p.use(HCLIB_HIP_SW_PATH_BAND_ROWS, SwKernel::BandRows, 64 * p.rows_per_wg * nw + 128,
              sw_band_lds_bytes(p.rows_per_wg * nw));
        per_cu = 1;
    } else if (rows)
        p.use(HCLIB_HIP_SW_PATH_ROWS1, kn.progressive ? SwKernel::Rows1Progressive : SwKernel::Rows1Whole, 64, one);
    else if (pk) {
        p.use(HCLIB_HIP_SW_PATH_DAG_PK, SwKernel::DagPk, 192, sw_pk_lds_bytes(tw));
        per_cu = kn.pk_wgs_per_cu;
    } else if (dag && band_shape && kn.dag_wave == 0) {
        // tile tasks on workgroups of th / bh + 2 waves where the band kernel
        // applies (HCLIB_HIP_SW_DAG_WAVE=1: one wave per tile); LDS + kept right columns
        p.use(HCLIB_HIP_SW_PATH_DAG_WG, SwKernel::DagWg, 64 * nw + 128, sw_band_lds_bytes(nw) + (4 + 2 * (size_t)th) * 4);
        per_cu = kn.dag_wgs_per_cu;
    } else if (dag)
        p.use(HCLIB_HIP_SW_PATH_DAG_WAVE, SwKernel::DagWave, 64, one);
    else
        p.use(HCLIB_HIP_SW_PATH_QUEUE, SwKernel::Queue, 64, one);
    if (dag) p.wgs_per_cu = per_cu;
    else p.grid_cap = num_cus * per_cu;
    if (!dag) p.grid = rows ? p.rows_grid((int)nth) : p.grid_cap;
    // what each path leaves on the device (include/hclib_hip.h): tagged
    // granules (rows: bottom rows; packed: all three) or the reference's
    // plain arrays; corner, deps and ready are carved on every path but a session's
    const size_t nt = ntw * nth, plain = !rows && !pk, aux = session ? 0 : nt * 4;
    p.bytes = {ntw * tw, nth * th, plain * nt * tw * 4,  plain * nt * th * 4, aux,
               aux,      aux,      !plain * nt * tw * 8, pk * nt * th * 8,    pk * nt * 8};
    return p;
}

}  // namespace hx
