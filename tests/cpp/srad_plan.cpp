// srad_plan.cpp — hclib_amd/csrc/hx_srad_plan.h as a host program (run by
// tests/test_srad_plan.py under AddressSanitizer and UBSan). Over every block
// grid up to 4 x 4 (block 16), regions of interest whole, 1 x 1 in each corner,
// a single row, a single column and the last block only, and niter 0 .. 3, it
// checks that
//   1. the await CSR is well formed and no task awaits a task twice,
//   2. any two tasks that touch the same (grid, block) or the same iteration's
//      scalar, at least one of them writing it, are ordered: one is an ancestor
//      of the other along the awaits (a task's footprint is taken from the cells
//      its body touches, not from the plan's neighbourhoods),
//   3. the counts equal the plan's closed forms (what hclib_hip_srad_bounds
//      reports), each from an enumeration over the graph or over the cells.
// Two controls run the same checker and must each find unordered pairs: the
// graph without the north-west await, and the graph whose T tasks do not await R.
#include <stdio.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "hx_srad_plan.h"

using namespace hx;

static int g_bad = 0;
#define CHECK(cond, ...)          \
    do {                          \
        if (!(cond)) {            \
            ++g_bad;              \
            printf("MISMATCH: "); \
            printf(__VA_ARGS__);  \
            printf("\n");         \
        }                         \
    } while (0)

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// unordered conflicting pairs of the graph (property 2); -1: not a DAG in id order
static long unordered_pairs(const SradPlan &p, const VersionGraph &g) {
    const int B = p.block, nb = (int)p.nb, n = (int)g.ntasks();
    const int words = (n + 63) / 64;
    std::vector<uint64_t> anc((size_t)n * (words ? words : 1), 0);
    for (int t = 0; t < n; ++t)
        for (uint32_t k = g.off[t]; k < g.off[t + 1]; ++k) {
            const int a = (int)g.ids[k];
            if (a >= t) return -1;
            anc[(size_t)t * words + a / 64] |= 1ull << (a % 64);
            for (int w = 0; w < words; ++w) anc[(size_t)t * words + w] |= anc[(size_t)a * words + w];
        }
    auto ordered = [&](int a, int b) { return (anc[(size_t)b * words + a / 64] >> (a % 64)) & 1; };  // a < b
    // resources: (grid, block) 0 .. 2 nb, then q0sqr(it), the datum of R(it)'s promise
    const int nres = 2 * nb + p.niter;
    std::vector<std::vector<int>> wr(nres), rd(nres);
    for (int t = 0; t < n; ++t) {
        const int kind = (int)g.payload[4 * t], it = (int)g.payload[4 * t + 1];
        const int bi = (int)g.payload[4 * t + 2], bj = (int)g.payload[4 * t + 3];
        std::set<int> reads;
        if (kind == 0) {
            for (int i = p.r1; i <= p.r2; ++i)
                for (int j = p.c1; j <= p.c2; ++j) reads.insert((i / B) * p.nby + j / B);
            wr[2 * nb + it].push_back(t);
        } else {
            // srad.hip stages the square one cell north and west, two south and east, indices clamped to the grid
            for (int r = -1; r <= B + 1; ++r)
                for (int c = -1; c <= B + 1; ++c) {
                    const int gi = clampi(bi * B + r, 0, p.rows - 1), gj = clampi(bj * B + c, 0, p.cols - 1);
                    reads.insert((gi / B) * p.nby + gj / B);
                }
            wr[((it + 1) & 1) * nb + bi * p.nby + bj].push_back(t);
            rd[2 * nb + it].push_back(t);
        }
        for (int r : reads) rd[(it & 1) * nb + r].push_back(t);
    }
    long bad = 0;
    for (int v = 0; v < nres; ++v)
        for (size_t i = 0; i < wr[v].size(); ++i) {
            for (size_t j = i + 1; j < wr[v].size(); ++j)
                if (!ordered(std::min(wr[v][i], wr[v][j]), std::max(wr[v][i], wr[v][j]))) ++bad;
            for (int r : rd[v])
                if (r != wr[v][i] && !ordered(std::min(r, wr[v][i]), std::max(r, wr[v][i]))) ++bad;
        }
    return bad;
}

static long g_control_nw = 0, g_control_r = 0;

static void check_case(int nbx, int nby, const int (&roi)[4], int niter) {
    const int B = 16, rows = nbx * B, cols = nby * B;
    char name[96];
    snprintf(name, sizeof name, "%dx%d roi %d..%d x %d..%d niter %d", rows, cols, roi[0], roi[1], roi[2], roi[3], niter);
    int block = B;
    SradPlan p;
    std::string err;
    const int rc = srad_plan(rows, cols, roi[0], roi[1], roi[2], roi[3], niter, block, 0, p, err);
    CHECK(rc == 0, "%s refused: %s", name, err.c_str());
    if (rc) return;
    VersionGraph g;
    srad_graph(p, g);
    const int nb = nbx * nby, n = (int)g.ntasks();
    // 3. the counts
    CHECK(p.nbx == nbx && p.nby == nby && p.nb == (uint64_t)nb, "%s: the block grid", name);
    CHECK((uint64_t)n == p.tasks && n == niter * (nb + 1), "%s: tasks %d plan %llu", name, n, (unsigned long long)p.tasks);
    CHECK(g.ids.size() == p.awaits, "%s: awaits %zu plan %llu", name, g.ids.size(), (unsigned long long)p.awaits);
    std::vector<uint32_t> waiters(n ? n : 1, 0);
    for (uint32_t a : g.ids) ++waiters[a];
    const uint64_t longest = n ? *std::max_element(waiters.begin(), waiters.end()) : 0;
    CHECK(longest == p.max_waiters, "%s: longest waiter list %llu plan %llu", name, (unsigned long long)longest,
          (unsigned long long)p.max_waiters);
    uint64_t moved = 0;
    for (int t = 0; t < n; ++t) {
        if (g.payload[4 * t] == 0) {
            moved += 4ull * (roi[1] - roi[0] + 1) * (roi[3] - roi[2] + 1);
            continue;
        }
        const int i0 = (int)g.payload[4 * t + 2] * B, j0 = (int)g.payload[4 * t + 3] * B;
        std::set<std::pair<int, int>> cells;  // the read region, clipped to the grid
        for (int r = -1; r <= B + 1; ++r)
            for (int c = -1; c <= B + 1; ++c)
                if (i0 + r >= 0 && i0 + r < rows && j0 + c >= 0 && j0 + c < cols) cells.insert({i0 + r, j0 + c});
        moved += 4ull * cells.size() + 4ull * B * B;
    }
    CHECK(moved == p.bytes_moved, "%s: bytes %llu plan %llu", name, (unsigned long long)moved,
          (unsigned long long)p.bytes_moved);
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    CHECK(p.arena_bytes == 2 * up((size_t)rows * cols * 4) + up((size_t)niter * 8), "%s: arena bytes", name);
    // 1. the CSR
    CHECK(g.off.size() == (size_t)n + 1 && g.off[0] == 0 && g.off[n] == g.ids.size(), "%s: off ends", name);
    CHECK(g.payload.size() == (size_t)4 * n, "%s: payload size", name);
    for (int t = 0; t < n; ++t) {
        CHECK(g.off[t + 1] >= g.off[t], "%s: off not monotone at %d", name, t);
        const int it = t / (nb + 1), k = t % (nb + 1);
        const bool is_r = k == 0;
        CHECK((int)g.payload[4 * t] == (is_r ? 0 : 1) && (int)g.payload[4 * t + 1] == it, "%s: payload of task %d", name, t);
        if (!is_r)
            CHECK((int)g.payload[4 * t + 2] == (k - 1) / nby && (int)g.payload[4 * t + 3] == (k - 1) % nby,
                  "%s: block of task %d", name, t);
        std::set<uint32_t> once(g.ids.begin() + g.off[t], g.ids.begin() + g.off[t + 1]);
        CHECK(once.size() == g.off[t + 1] - g.off[t], "%s: task %d awaits a task twice", name, t);
        for (uint32_t a : once) {
            CHECK((int)a < t, "%s: task %d awaits %u", name, t, a);
            const int ait = (int)a / (nb + 1), ak = (int)a % (nb + 1);
            if (is_r) CHECK(ait == it - 1 && ak != 0, "%s: R task %d awaits %u", name, t, a);
            else CHECK((ak == 0 && ait == it) || (ak != 0 && ait == it - 1), "%s: T task %d awaits %u", name, t, a);
        }
        if (!is_r) CHECK(once.count((uint32_t)(it * (nb + 1))) == 1, "%s: task %d does not await its R", name, t);
    }
    // 2. the order
    const long bad = unordered_pairs(p, g);
    CHECK(bad == 0, "%s: %ld conflicting pairs are not ordered", name, bad);
    // the controls
    if (nbx >= 2 && nby >= 2 && niter >= 2) {
        VersionGraph h;
        srad_graph(p, h, false, true);
        // (where the north-west neighbour lies in the ROI's blocks the chain through R orders the pair as well,
        // so the control is the total, and this case with the ROI elsewhere)
        const long c = unordered_pairs(p, h);
        CHECK(c >= 0, "%s: the graph without the north-west await is no DAG", name);
        if (p.rb1 == nbx - 1 && p.cb1 == nby - 1) CHECK(c > 0, "%s: the graph without the north-west await is ordered", name);
        g_control_nw += c > 0 ? c : 0;
    }
    if (niter >= 1) {
        VersionGraph h;
        srad_graph(p, h, true, false);
        const long c = unordered_pairs(p, h);
        CHECK(c > 0, "%s: the graph whose T tasks do not await R is ordered", name);
        g_control_r += c > 0 ? c : 0;
    }
}

int main() {
    int cases = 0;
    for (int nbx = 1; nbx <= 4; ++nbx)
        for (int nby = 1; nby <= 4; ++nby) {
            const int rows = nbx * 16, cols = nby * 16;
            const int rois[8][4] = {
                {0, rows - 1, 0, cols - 1},                    // whole
                {0, 0, 0, 0},                                  // 1 x 1 in each corner
                {0, 0, cols - 1, cols - 1},
                {rows - 1, rows - 1, 0, 0},
                {rows - 1, rows - 1, cols - 1, cols - 1},
                {rows / 2 + 1, rows / 2 + 1, 0, cols - 1},     // a single row
                {0, rows - 1, cols / 2 + 1, cols / 2 + 1},     // a single column
                {rows - 16, rows - 1, cols - 16, cols - 1},    // the last block only
            };
            for (const auto &roi : rois)
                for (int niter = 0; niter <= 3; ++niter) {
                    check_case(nbx, nby, roi, niter);
                    ++cases;
                }
        }
    // the default block and the refusals
    CHECK(srad_default_block(128, 192) == 64 && srad_default_block(96, 64) == 32 && srad_default_block(48, 16) == 16 &&
              srad_default_block(24, 16) == 0,
          "the default block");
    {
        SradPlan p;
        std::string err;
        int b = 0;
        CHECK(srad_plan(512, 512, 0, 127, 0, 127, 2, b, 0, p, err) == 0 && b == 64 && p.tasks == 130, "the default plan");
        b = 16;
        CHECK(srad_plan(16, 16, 0, 0, 0, 0, (1 << 25), b, 0, p, err) != 0 && err.find("tasks") != std::string::npos,
              "2^26 tasks are refused");
        b = 16;
        CHECK(srad_plan(16, 16, 0, 0, 0, 0, (1 << 25) - 1, b, 0, p, err) == 0, "2^26 - 2 tasks are accepted: %s", err.c_str());
    }
    printf("%d cases\n", cases);
    printf("control: %ld unordered pairs without the north-west await\n", g_control_nw);
    printf("control: %ld unordered pairs without T awaiting R\n", g_control_r);
    printf(g_bad ? "Check results: %d MISMATCH\n" : "Check results: OK\n", g_bad);
    return g_bad ? 1 : 0;
}
