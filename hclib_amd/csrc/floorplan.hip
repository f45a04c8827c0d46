// floorplan.hip — BOTS floorplan as a device task kind of the work-stealing
// scheduler: a branch-and-bound search whose tasks prune against a bound that
// other tasks lower while they run.
//
// The reference (test/performance-regression/full-apps/bots/floorplan/
// floorplan.c:230-328, the algorithm in floorplan.ref.c): add_cell(id) spawns
// one async per (shape i, north-west corner j) candidate of cell id; the async
// lays the cell down on a copy of the 64 x 64 board, computes the footprint's
// area, and calls add_cell(next) only `if (area < MIN_AREA)`; a complete
// placement lowers MIN_AREA and saves its board in a critical section.
//
// Here an item is one candidate: child k of the call add_cell(id) on a partial
// placement, k counting the (i, j) pairs in the reference's order. With its
// predecessors placed a cell's rectangle is fixed by its shape index and one
// coordinate (starts(), :73-127: a left dependence forces the column, an above
// dependence the row, both leave at most one corner), so a partial placement
// is 9 bits per placed cell, in placement order, plus a count: 185 of the 6-word
// template's 192 bits, no board and no allocation. process() replays the chain
// from the packed choices into a per-lane rectangle array in LDS; lay_down
// (:135-150) is a rectangle-intersection test against those rectangles (the
// board holds nothing else). A rectangle that leaves the board does not fit
// (the reference indexes past its board there).
//
// The bound is one word in HBM, read by every item with an agent-scope relaxed
// load (issued first, used last) and lowered with an agent-scope atomic min. A
// stale read only costs tasks. Every lane keeps the best complete placement it
// met; a wave writes the best of its lanes to its own record whenever its ring
// runs empty, and the host takes the minimum over the records.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "hx_client.h"

namespace hx {

constexpr int kFpMaxCells = HCLIB_HIP_FLOORPLAN_MAX_CELLS;
constexpr int kFpMaxShapes = HCLIB_HIP_FLOORPLAN_MAX_SHAPES;
constexpr int kFpSide = 64;                    // ROWS = COLS
constexpr uint32_t kFpArea0 = kFpSide * kFpSide;  // MIN_AREA before any placement
constexpr uint32_t kFpNone = 0xffu;            // table: no left / above dependence
constexpr uint32_t kFpDummy = 0xffff0000u;     // cell 0: top = bot = 0, lhs = rhs = -1
// the cell table, by position p = 1..n in the chain 1 -> next -> ...: word
// 9 p = shapes | left's position << 8 | above's position << 16 (0 the dummy
// cell, kFpNone none), words 9 p + 1 + i = rows | cols << 8 of shape i
constexpr int kFpTabStride = 1 + kFpMaxShapes;
constexpr int kFpTabWords = (kFpMaxCells + 1) * kFpTabStride;
// packed placement: the choice of the cell at position p is 9 bits (shape |
// coordinate << 3: the row under a left dependence alone, the column under an
// above dependence alone, 0 under both), seven choices per 64-bit pair of
// template words; the count of placed cells is bits 24..28 of word 5
constexpr uint32_t kFpFieldBits = 9, kFpPairBits = 63;
constexpr uint32_t kFpCountShift = 24;
constexpr int kFpLoweredShift = 48;  // FpAcc::totals

struct FpRect {
    int top, bot, lhs, rhs;
};
__host__ __device__ __forceinline__ FpRect fp_unpack(uint32_t w) {
    FpRect r;
    r.top = (int)(w & 0xffu);
    r.bot = (int)((w >> 8) & 0xffu);
    r.lhs = (int)(w << 8) >> 24;
    r.rhs = (int)w >> 24;
    return r;
}
__host__ __device__ __forceinline__ uint32_t fp_pack(int top, int bot, int lhs, int rhs) {
    return (uint32_t)top | ((uint32_t)bot << 8) | (((uint32_t)lhs & 0xffu) << 16) | ((uint32_t)rhs << 24);
}
__host__ __device__ __forceinline__ int fp_max(int a, int b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ int fp_min(int a, int b) { return a < b ? a : b; }

// starts() for one shape: the number of north-west corners and the first one;
// corner j is (t0 + j, l0) under a left dependence alone and (t0, l0 + j)
// under an above dependence alone. The touch test under both is the
// reference's loose one (bot = top + rows, :90-95)
__host__ __device__ __forceinline__ int fp_starts(bool has_l, bool has_a, const FpRect &L, const FpRect &A, int rows,
                                                  int cols, int &t0, int &l0) {
    if (has_l && has_a) {
        t0 = A.bot + 1;
        l0 = L.rhs + 1;
        return (t0 <= L.bot && t0 + rows >= L.top && l0 <= A.rhs && l0 + cols >= A.lhs) ? 1 : 0;
    }
    if (has_l) {
        t0 = fp_max(L.top - rows + 1, 0);
        l0 = L.rhs + 1;
        return fp_max(fp_min(L.bot, kFpSide) - t0 + 1, 0);
    }
    l0 = fp_max(A.lhs - cols + 1, 0);
    t0 = A.bot + 1;
    return fp_max(fp_min(A.rhs, kFpSide) - l0 + 1, 0);
}

struct FpCtx {
    uint32_t n;              // cells
    uint32_t root_children;  // candidates of the first cell
    uint32_t prune;          // 0: pruning compares against 4096 (the search is exhaustive)
    const uint32_t *tab;     // kFpTabWords
    uint32_t *bound;         // MIN_AREA
    unsigned long long *hist;  // n + 1 words (the histogram instantiation), or null
    uint32_t *best;          // per worker: {area, packed placement (6), 0}
};

__shared__ uint32_t s_fp_tab[kFpTabWords];
// the replayed rectangles, by chain position; one column of the array per lane
__shared__ uint32_t s_fp_rect[kFpMaxCells + 1][64];
// the wave's share of the per-depth histogram, handed over when it goes idle
__shared__ unsigned long long s_fp_hist[kFpMaxCells + 1];

struct FpAcc {
    unsigned long long items = 0, tasks = 0, laid = 0, complete = 0, improvements = 0;
    uint32_t best = kFpArea0;  // this lane's best complete placement: its area and packed state
    uint32_t bs[6] = {0, 0, 0, 0, 0, 0};
    uint32_t flushed = kFpArea0;  // the area in the wave's record (wave-uniform)
    // (a worker's exit record carries four sums of the kind's: the lowerings
    // ride above the complete placements. Each lowering takes the bound at
    // least one below its last value, so a launch has fewer than 4096)
    __device__ void totals(unsigned long long (&c)[8], unsigned long long (&)[4]) {
        c[0] = wave_sum(items);
        c[1] = wave_sum(tasks);
        c[2] = wave_sum(laid);
        c[3] = wave_sum(complete) + (wave_sum(improvements) << kFpLoweredShift);
    }
};

// the dependences of the cell at position p, from the lane's replayed column
struct FpDeps {
    bool has_l, has_a;
    FpRect L, A;
    uint32_t shapes;
};
__device__ __forceinline__ FpDeps fp_deps(uint32_t p, int lane) {
    const uint32_t hdr = s_fp_tab[p * kFpTabStride];
    const uint32_t lp = (hdr >> 8) & 0xffu, ap = (hdr >> 16) & 0xffu;
    FpDeps d;
    d.shapes = hdr & 0xffu;
    d.has_l = lp != kFpNone;
    d.has_a = ap != kFpNone;
    d.L = fp_unpack(s_fp_rect[d.has_l ? lp : 0u][lane]);
    d.A = fp_unpack(s_fp_rect[d.has_a ? ap : 0u][lane]);
    return d;
}

template <bool HIST>
struct FpKind {
    // template = the packed partial placement (see kFpFieldBits): its children
    // are the candidates of the next cell of the chain
    static constexpr int kTmplWords = 6;
    static constexpr int kWords = 8;
    static constexpr bool kPure = false;            // the bound is read and lowered
    static constexpr bool kBoundedChildren = true;  // at most 8 shapes x 64 corners
    using Ctx = FpCtx;
    using Acc = FpAcc;

    __device__ static int roots(const Ctx &c, Acc &, uint32_t *tmpl) {
        tmpl[0] = tmpl[1] = tmpl[2] = tmpl[3] = tmpl[4] = tmpl[5] = 0;
        return (int)c.root_children;
    }

    __device__ static int process(const Ctx &c, Acc &acc, const uint32_t *t, uint32_t k, uint32_t *child,
                                  uint32_t *err, bool) {
        const int lane = lane_id();
        // MIN_AREA as of now: the load is in flight while the chain is replayed
        const uint32_t bound = ld_agent(c.bound);
        unsigned long long w0 = t[0] | ((unsigned long long)t[1] << 32);
        unsigned long long w1 = t[2] | ((unsigned long long)t[3] << 32);
        unsigned long long w2 = t[4] | ((unsigned long long)t[5] << 32);
        const uint32_t cnt = (t[5] >> kFpCountShift) & 31u;
        // replay 1 -> next -> ... from the packed choices
        s_fp_rect[0][lane] = kFpDummy;
        int fr = 0, fc = 0;
        uint32_t which = 0, sh = 0;
        for (uint32_t p = 1; p <= cnt; ++p) {
            const unsigned long long w = which == 0 ? w0 : (which == 1 ? w1 : w2);
            const uint32_t f = (uint32_t)(w >> sh) & 511u;
            const FpDeps d = fp_deps(p, lane);
            const uint32_t dims = s_fp_tab[p * kFpTabStride + 1u + (f & 7u)];
            const int rows = (int)(dims & 0xffu), cols = (int)(dims >> 8);
            const int top = d.has_a ? d.A.bot + 1 : (int)(f >> 3);
            const int lhs = d.has_l ? d.L.rhs + 1 : (int)(f >> 3);
            const int bot = top + rows - 1, rhs = lhs + cols - 1;
            s_fp_rect[p][lane] = fp_pack(top, bot, lhs, rhs);
            fr = fp_max(fr, bot + 1);
            fc = fp_max(fc, rhs + 1);
            sh += kFpFieldBits;
            if (sh == kFpPairBits) {
                sh = 0;
                ++which;
            }
        }
        // candidate k of the next cell: shapes outermost, then starts()'s corners
        const uint32_t p = cnt + 1u;
        const FpDeps d = fp_deps(p, lane);
        bool found = false;
        uint32_t kk = k, si = 0;
        int t0 = 0, l0 = 0, rows = 1, cols = 1;
        for (uint32_t i = 0; i < d.shapes; ++i) {
            const uint32_t dims = s_fp_tab[p * kFpTabStride + 1u + i];
            const int r = (int)(dims & 0xffu), cl = (int)(dims >> 8);
            int ti, li;
            const uint32_t ni = (uint32_t)fp_starts(d.has_l, d.has_a, d.L, d.A, r, cl, ti, li);
            if (kk < ni) {
                found = true;
                si = i;
                t0 = ti;
                l0 = li;
                rows = r;
                cols = cl;
                break;
            }
            kk -= ni;
        }
        if (!found) dev_error(err, kErrBadTask);  // the parent counted with the same function
        const int top = t0 + (d.has_l && !d.has_a ? (int)kk : 0);
        const int lhs = l0 + (!d.has_l ? (int)kk : 0);
        const int bot = top + rows - 1, rhs = lhs + cols - 1;
        // lay_down: inside the board and clear of every placed rectangle
        bool fits = found && bot < kFpSide && rhs < kFpSide;
        for (uint32_t q = 1; q <= cnt; ++q) {
            const FpRect o = fp_unpack(s_fp_rect[q][lane]);
            fits = fits && (o.bot < top || o.top > bot || o.rhs < lhs || o.lhs > rhs);
        }
        acc.items += 1;
        // the child's state: this choice behind the parent's, one more cell
        const uint32_t coord = d.has_a ? (d.has_l ? 0u : (uint32_t)lhs) : (uint32_t)top;
        const unsigned long long fld = (unsigned long long)((si | (coord << 3)) & 511u) << sh;
        w0 |= which == 0 ? fld : 0ull;
        w1 |= which == 1 ? fld : 0ull;
        w2 |= which == 2 ? fld : 0ull;
        child[0] = (uint32_t)w0;
        child[1] = (uint32_t)(w0 >> 32);
        child[2] = (uint32_t)w1;
        child[3] = (uint32_t)(w1 >> 32);
        child[4] = (uint32_t)w2;
        child[5] = ((uint32_t)(w2 >> 32) & ~(31u << kFpCountShift)) | (p << kFpCountShift);
        // (the counts are added once, behind the branches: an increment in each
        // arm becomes one store through a selected address, and Acc then lives
        // in scratch memory)
        uint32_t nchild = 0, done = 0, lowered = 0;
        if (fits) {
            if constexpr (HIST)
                __hip_atomic_fetch_add(&s_fp_hist[p], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint32_t area = (uint32_t)(fp_max(fr, bot + 1) * fp_max(fc, rhs + 1));
            if (p == c.n) {
                // the last cell: a complete placement
                done = 1;
                if (area < bound) {
                    const uint32_t old =
                        __hip_atomic_fetch_min(c.bound, area, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    lowered = area < old ? 1u : 0u;
                }
                const bool better = area < acc.best;
                acc.best = better ? area : acc.best;
#pragma unroll
                for (int i = 0; i < 6; ++i) acc.bs[i] = better ? child[i] : acc.bs[i];
            } else if (area < (c.prune ? bound : kFpArea0)) {
                // add_cell(next): its candidates, counted against this placement
                s_fp_rect[p][lane] = fp_pack(top, bot, lhs, rhs);
                const FpDeps e = fp_deps(p + 1u, lane);
                for (uint32_t i = 0; i < e.shapes; ++i) {
                    const uint32_t dims = s_fp_tab[(p + 1u) * kFpTabStride + 1u + i];
                    int ti, li;
                    nchild += (uint32_t)fp_starts(e.has_l, e.has_a, e.L, e.A, (int)(dims & 0xffu), (int)(dims >> 8),
                                                  ti, li);
                }
            }
        }
        acc.laid += fits ? 1u : 0u;
        acc.complete += done;
        acc.improvements += lowered;
        acc.tasks += nchild;
        return (int)nchild;
    }

    // (whole wave, uniform control flow) the ring ran empty: the wave's best
    // complete placement goes to its record if it beats what is there, and the
    // histogram's share to HBM
    __device__ static void drain(const Ctx &c, Acc &acc, uint32_t *) {
        const int lane = lane_id();
        const uint32_t m = kFpArea0 - wave_max(kFpArea0 - acc.best);
        if (m < acc.flushed) {
            const unsigned long long has = __ballot(acc.best == m);
            if (lane == __builtin_ctzll(has)) {
                uint32_t *rec = c.best + 8u * blockIdx.x;
                rec[0] = m;
#pragma unroll
                for (int i = 0; i < 6; ++i) rec[1 + i] = acc.bs[i];
                rec[7] = 0;
            }
            acc.flushed = m;
        }
        if constexpr (HIST) {
            if (lane <= (int)c.n) {
                const unsigned long long v = s_fp_hist[lane];
                if (v) {
                    add_agent(&c.hist[lane], v);
                    s_fp_hist[lane] = 0;
                }
            }
            asm volatile("" ::: "memory");
        }
    }
};

constexpr int kFpCap = 1024;  // ring items per wave

template <class K>
__global__ __launch_bounds__(64) void k_floorplan(FpCtx ctx, PoolView pool, SchedGlobals *g, SchedConfig cfg) {
    __shared__ WaveStack<K, kFpCap> st;
    for (int i = threadIdx.x; i < kFpTabWords; i += 64) s_fp_tab[i] = ctx.tab[i];
    if (threadIdx.x <= kFpMaxCells) s_fp_hist[threadIdx.x] = 0;
    __syncthreads();
    run_worker<K, kFpCap>(ctx, pool, g, cfg, st, blockIdx.x == 0);
}

}  // namespace hx

using namespace hx;

namespace {

// The checked input: the chain's cell ids by position, and the device table.
struct FpPlan {
    int order[kFpMaxCells + 1];  // order[p] = the cell at position p (order[0] = 0, the dummy cell)
    int pos[kFpMaxCells + 1];    // pos[cell]
    uint32_t tab[kFpTabWords];
    uint32_t root_children;
};

int fp_plan(const char *who, const hclib_hip_floorplan_input_t *in, FpPlan *pl) {
    if (!in) {
        set_error("%s: in is NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    const int n = in->n;
    if (n < 1 || n > kFpMaxCells) {
        set_error("%s: n = %d must be in [1, %d]", who, n, kFpMaxCells);
        return HCLIB_HIP_EINVAL;
    }
    for (int c = 1; c <= n; ++c) {
        if (in->shapes[c] < 1 || in->shapes[c] > kFpMaxShapes) {
            set_error("%s: cell %d has %d shapes, must be in [1, %d]", who, c, in->shapes[c], kFpMaxShapes);
            return HCLIB_HIP_EINVAL;
        }
        for (int i = 0; i < in->shapes[c]; ++i)
            for (int x = 0; x < 2; ++x)
                if (in->shape[c][i][x] < 1 || in->shape[c][i][x] > kFpSide) {
                    set_error("%s: cell %d, shape %d: dimension %d must be in [1, %d]", who, c, i, in->shape[c][i][x],
                              kFpSide);
                    return HCLIB_HIP_EINVAL;
                }
        if (in->left[c] < -1 || in->left[c] > n || in->above[c] < -1 || in->above[c] > n || in->next[c] < 0 ||
            in->next[c] > n) {
            set_error("%s: cell %d: left %d, above %d or next %d is outside the table", who, c, in->left[c],
                      in->above[c], in->next[c]);
            return HCLIB_HIP_EINVAL;
        }
        if (in->left[c] < 0 && in->above[c] < 0) {
            set_error("%s: cell %d has neither a left nor an above cell", who, c);
            return HCLIB_HIP_EINVAL;
        }
    }
    // the chain from cell 1 visits every cell exactly once before 0
    memset(pl->pos, 0, sizeof(pl->pos));
    pl->order[0] = 0;
    int c = 1;
    for (int p = 1; p <= n; ++p) {
        if (c == 0 || pl->pos[c] != 0) {
            set_error("%s: the next chain from cell 1 %s after %d of %d cells", who,
                      c == 0 ? "ends" : "returns to a cell", p - 1, n);
            return HCLIB_HIP_EINVAL;
        }
        pl->pos[c] = p;
        pl->order[p] = c;
        c = in->next[c];
    }
    if (c != 0) {
        set_error("%s: the next chain from cell 1 does not end after %d cells", who, n);
        return HCLIB_HIP_EINVAL;
    }
    memset(pl->tab, 0, sizeof(pl->tab));
    for (int p = 1; p <= n; ++p) {
        c = pl->order[p];
        const int dep[2] = {in->left[c], in->above[c]};
        uint32_t dp[2];
        for (int x = 0; x < 2; ++x) {
            // a cell is placed against rectangles that exist: the dummy cell
            // or a cell earlier in the chain
            if (dep[x] > 0 && pl->pos[dep[x]] >= p) {
                set_error("%s: cell %d depends on cell %d, which the chain places later", who, c, dep[x]);
                return HCLIB_HIP_EINVAL;
            }
            dp[x] = dep[x] < 0 ? kFpNone : (uint32_t)pl->pos[dep[x]];
        }
        pl->tab[p * kFpTabStride] = (uint32_t)in->shapes[c] | (dp[0] << 8) | (dp[1] << 16);
        for (int i = 0; i < in->shapes[c]; ++i)
            pl->tab[p * kFpTabStride + 1 + i] = (uint32_t)in->shape[c][i][0] | ((uint32_t)in->shape[c][i][1] << 8);
    }
    // add_cell(1): its candidates against the dummy cell alone
    const uint32_t hdr = pl->tab[kFpTabStride];
    const bool has_l = ((hdr >> 8) & 0xffu) != kFpNone, has_a = ((hdr >> 16) & 0xffu) != kFpNone;
    const FpRect dummy = fp_unpack(kFpDummy);
    pl->root_children = 0;
    for (uint32_t i = 0; i < (hdr & 0xffu); ++i) {
        const uint32_t dims = pl->tab[kFpTabStride + 1 + i];
        int t0, l0;
        pl->root_children += (uint32_t)fp_starts(has_l, has_a, dummy, dummy, (int)(dims & 0xffu), (int)(dims >> 8), t0, l0);
    }
    return HCLIB_HIP_OK;
}

// A complete packed placement back into rectangles: the device's replay.
void fp_decode(const FpPlan &pl, int n, const uint32_t *t, hclib_hip_floorplan_result_t *res, uint8_t *board) {
    const unsigned long long w[3] = {t[0] | ((unsigned long long)t[1] << 32), t[2] | ((unsigned long long)t[3] << 32),
                                     t[4] | ((unsigned long long)t[5] << 32)};
    uint32_t rect[kFpMaxCells + 1];
    rect[0] = kFpDummy;
    int fr = 0, fc = 0;
    for (int p = 1; p <= n; ++p) {
        const uint32_t f = (uint32_t)(w[(p - 1) / 7] >> (kFpFieldBits * ((p - 1) % 7))) & 511u;
        const uint32_t hdr = pl.tab[p * kFpTabStride];
        const uint32_t lp = (hdr >> 8) & 0xffu, ap = (hdr >> 16) & 0xffu;
        const uint32_t dims = pl.tab[p * kFpTabStride + 1 + (f & 7u)];
        const int rows = (int)(dims & 0xffu), cols = (int)(dims >> 8);
        const int top = ap != kFpNone ? fp_unpack(rect[ap]).bot + 1 : (int)(f >> 3);
        const int lhs = lp != kFpNone ? fp_unpack(rect[lp]).rhs + 1 : (int)(f >> 3);
        rect[p] = fp_pack(top, top + rows - 1, lhs, lhs + cols - 1);
        fr = fp_max(fr, top + rows);
        fc = fp_max(fc, lhs + cols);
        const int c = pl.order[p];
        res->placements[c - 1].shape = (int32_t)(f & 7u);
        res->placements[c - 1].top = top;
        res->placements[c - 1].lhs = lhs;
        if (board)
            for (int r = top; r < top + rows && r < kFpSide; ++r)
                for (int x = lhs; x < lhs + cols && x < kFpSide; ++x) board[r * kFpSide + x] = (uint8_t)c;
    }
    res->footprint[0] = fr;
    res->footprint[1] = fc;
}

}  // namespace

extern "C" int hclib_hip_floorplan_read_input(const char *path, hclib_hip_floorplan_input_t *out) {
    const char *who = "hclib_hip_floorplan_read_input";
    if (!path || !out) {
        set_error("%s: %s is NULL", who, path ? "out" : "path");
        return HCLIB_HIP_EINVAL;
    }
    FILE *f = fopen(path, "r");
    if (!f) {
        set_error("%s: cannot open %s", who, path);
        return HCLIB_HIP_EINVAL;
    }
    memset(out, 0, sizeof(*out));
    out->solution = -1;
    int rc = HCLIB_HIP_OK, n = 0;
    // read_inputs (:159-195): n, then per cell its shape count, the shapes'
    // rows and columns, left, above and next; then, optionally, the solution
    auto bogus = [&](int cell) {
        set_error("%s: %s: bogus input file (cell %d)", who, path, cell);
        rc = HCLIB_HIP_EINVAL;
    };
    if (fscanf(f, "%d", &n) != 1) bogus(0);
    if (rc == HCLIB_HIP_OK && (n < 1 || n > kFpMaxCells)) {
        set_error("%s: %s: n = %d must be in [1, %d]", who, path, n, kFpMaxCells);
        rc = HCLIB_HIP_EINVAL;
    }
    out->n = n;
    for (int c = 1; rc == HCLIB_HIP_OK && c <= n; ++c) {
        int k = 0;
        if (fscanf(f, "%d", &k) != 1) {
            bogus(c);
            break;
        }
        if (k < 1 || k > kFpMaxShapes) {
            set_error("%s: %s: cell %d has %d shapes, must be in [1, %d]", who, path, c, k, kFpMaxShapes);
            rc = HCLIB_HIP_EINVAL;
            break;
        }
        out->shapes[c] = k;
        for (int i = 0; i < k && rc == HCLIB_HIP_OK; ++i)
            if (fscanf(f, "%d %d", &out->shape[c][i][0], &out->shape[c][i][1]) != 2) bogus(c);
        if (rc == HCLIB_HIP_OK && fscanf(f, "%d %d %d", &out->left[c], &out->above[c], &out->next[c]) != 3) bogus(c);
    }
    if (rc == HCLIB_HIP_OK) {
        int s = -1;
        const int got = fscanf(f, "%d", &s);
        if (got == 1) out->solution = s;
        else if (got != EOF) bogus(n + 1);
    }
    fclose(f);
    if (rc != HCLIB_HIP_OK) return rc;
    FpPlan pl;
    return fp_plan(who, out, &pl);
}

extern "C" int hclib_hip_floorplan(const hclib_hip_floorplan_input_t *in, int flags,
                                   hclib_hip_floorplan_result_t *result, uint8_t *board, uint64_t *hist) {
    const char *who = "hclib_hip_floorplan";
    if (!result) {
        set_error("%s: result is NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    if (flags & ~HCLIB_HIP_FLOORPLAN_NOPRUNE) {
        set_error("%s: unknown flags 0x%x", who, (unsigned)flags);
        return HCLIB_HIP_EINVAL;
    }
    FpPlan pl;
    HX_TRY(fp_plan(who, in, &pl));
    const int n = in->n;
    HX_TRY(ensure_device());
    Module &m = mod();
    const int grid = sched_grid(3);
    // one upload: the bound's line, the table, the histogram, the workers' records
    constexpr size_t kTabOff = 256, kTabBytes = (sizeof(uint32_t) * kFpTabWords + 255) & ~(size_t)255;
    constexpr size_t kHistOff = kTabOff + kTabBytes, kBestOff = kHistOff + 256;
    const size_t bytes = kBestOff + 32 * (size_t)grid;
    std::vector<uint32_t> init(bytes / 4, 0u);
    init[0] = kFpArea0;
    memcpy(&init[kTabOff / 4], pl.tab, sizeof(pl.tab));
    for (size_t i = kBestOff / 4; i < bytes / 4; ++i) init[i] = ~0u;
    DevBuf buf;
    HX_TRY(buf.alloc(bytes, who));
    HX_TRY(upload_async(buf.p, init.data(), bytes, m.stream));
    FpCtx ctx;
    ctx.n = (uint32_t)n;
    ctx.root_children = pl.root_children;
    ctx.prune = (flags & HCLIB_HIP_FLOORPLAN_NOPRUNE) ? 0u : 1u;
    ctx.bound = (uint32_t *)buf.p;
    ctx.tab = (const uint32_t *)(buf.p + kTabOff);
    ctx.hist = hist ? (unsigned long long *)(buf.p + kHistOff) : nullptr;
    ctx.best = (uint32_t *)(buf.p + kBestOff);
    PoolView pool;
    HX_TRY(sched_pool(64, (uint32_t)env_int("HCLIB_HIP_FLOORPLAN_CHUNK", 32), 8, &pool));
    const SchedConfig cfg = sched_config_unseeded("FLOORPLAN", grid);
    HX_TRY(reset_sched(pool, 1u, false, (uint32_t)grid));
    void (*const kern)(FpCtx, PoolView, SchedGlobals *, SchedConfig) =
        hist ? k_floorplan<FpKind<true>> : k_floorplan<FpKind<false>>;
    SchedGlobals gl;
    float ms = 0;
    HX_TRY(launch_sched((const void *)kern, grid, 64, who, [&] {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, m.stream, ctx, pool, m.globals, cfg);
    }, &gl, &ms, "hipLaunchKernelGGL(k_floorplan)"));
    std::vector<uint32_t> back(bytes / 4);
    HX_HIP(hipMemcpy(back.data(), buf.p, bytes, hipMemcpyDeviceToHost));
    // the minimum over the workers' records; on equal area any of them is right
    // (the reference's winner under its critical section depends on the schedule too)
    const uint32_t *best = nullptr;
    for (int wv = 0; wv < grid; ++wv) {
        const uint32_t *rec = &back[kBestOff / 4 + 8 * (size_t)wv];
        if (rec[0] < kFpArea0 && (!best || rec[0] < best[0])) best = rec;
    }
    const uint32_t bound = back[0];
    if ((best ? best[0] : kFpArea0) != bound) {
        set_error("%s: the bound ended at %u, the best recorded placement has area %u", who, bound,
                  best ? best[0] : kFpArea0);
        return HCLIB_HIP_EDEVICE;
    }
    memset(result, 0, sizeof(*result));
    result->min_area = (int32_t)bound;
    for (int c = 0; c < kFpMaxCells; ++c) result->placements[c].shape = result->placements[c].top = result->placements[c].lhs = -1;
    if (board) memset(board, 0, kFpArea0);
    if (best) fp_decode(pl, n, best + 1, result, board);
    // the reference's bots_number_of_tasks (nnc + nnl): the candidates spawned,
    // the first cell's included. Every candidate is one item
    result->tasks = gl.counters[1] + pl.root_children;
    result->items = gl.counters[0];
    result->laid = gl.counters[2];
    result->complete = gl.counters[3] & ((1ull << kFpLoweredShift) - 1);
    result->improvements = gl.counters[3] >> kFpLoweredShift;
    result->chunks_pushed = gl.counters[kCtrPushed];
    result->chunks_stolen = gl.counters[kCtrStolen];
    result->kernel_ms = ms;
    result->busy_frac = busy_frac(gl);
    if (hist)
        for (int i = 0; i <= n; ++i) hist[i] = ((const unsigned long long *)&back[kHistOff / 4])[i];
    return HCLIB_HIP_OK;
}
