// jacobi_plan.cpp — hclib_amd/csrc/hx_jacobi_plan.h as a host program (run by
// tests/test_jacobi_plan.py under AddressSanitizer and UBSan): for a sweep of
// small block grids, iteration counts and fuse depths it checks that
//   1. the await CSR is well formed,
//   2. every task awaits exactly its neighbour set of the superstep before,
//   3. any two tasks that touch the same (buffer, block), at least one of them
//      writing it, are ordered: one is an ancestor of the other along the awaits
//      (a task's footprint is taken from what its body does — the block it
//      writes, and the blocks its halo of t_s cells reaches — not from the
//      plan's neighbour rule),
//   4. the counts equal the closed forms, and an enumeration of the regions.
// As a control the same checker is run on the graph with the mistake the plan's
// header warns of (a last superstep of t = 1 awaiting only 4 neighbours under
// fuse >= 2) and must find it unordered.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <vector>

#include "hx_jacobi_plan.h"

using namespace hx;

static int g_bad = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            ++g_bad;                     \
            printf("MISMATCH: ");        \
            printf(__VA_ARGS__);         \
            printf("\n");                \
        }                                \
    } while (0)

struct Shape {
    int nbx, nby, block, niter, fuse;
};

// the blocks a halo of t cells around (bx, by) reaches: the block, its edge
// neighbours, and from t = 2 on its diagonal ones (t <= block)
static std::vector<int> footprint(const Shape &s, int bx, int by, int t) {
    std::vector<int> r;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy) {
            if (dx && dy && t < 2) continue;
            const int x = bx + dx, y = by + dy;
            if (x >= 0 && y >= 0 && x < s.nbx && y < s.nby) r.push_back(x * s.nby + y);
        }
    return r;
}

// unordered conflicting pairs of the graph (property 3)
static long unordered_pairs(const Shape &s, const VersionGraph &g) {
    const int nb = s.nbx * s.nby, n = (int)g.ntasks();
    // ancestors by bitset: awaits point at earlier tasks, so one pass in id order closes them
    const int words = (n + 63) / 64;
    std::vector<uint64_t> anc((size_t)n * (words ? words : 1), 0);
    for (int t = 0; t < n; ++t)
        for (uint32_t k = g.off[t]; k < g.off[t + 1]; ++k) {
            const int a = (int)g.ids[k];
            if (a >= t) return -1;  // not a DAG in id order
            anc[(size_t)t * words + a / 64] |= 1ull << (a % 64);
            for (int w = 0; w < words; ++w) anc[(size_t)t * words + w] |= anc[(size_t)a * words + w];
        }
    auto ordered = [&](int a, int b) {  // a < b
        return (anc[(size_t)b * words + a / 64] >> (a % 64)) & 1;
    };
    // per (buffer, block): the tasks that write it and the tasks that read it
    std::vector<std::vector<int>> wr(2 * nb), rd(2 * nb);
    for (int t = 0; t < n; ++t) {
        const int st = (int)g.payload[4 * t], bx = (int)g.payload[4 * t + 1], by = (int)g.payload[4 * t + 2];
        const int ts = (int)g.payload[4 * t + 3];
        wr[((st + 1) & 1) * nb + bx * s.nby + by].push_back(t);
        for (int b : footprint(s, bx, by, ts)) rd[(st & 1) * nb + b].push_back(t);
    }
    long bad = 0;
    for (int v = 0; v < 2 * nb; ++v) {
        for (size_t i = 0; i < wr[v].size(); ++i) {
            for (size_t j = i + 1; j < wr[v].size(); ++j)
                if (!ordered(std::min(wr[v][i], wr[v][j]), std::max(wr[v][i], wr[v][j]))) ++bad;
            for (int r : rd[v])
                if (r != wr[v][i] && !ordered(std::min(r, wr[v][i]), std::max(r, wr[v][i]))) ++bad;
        }
    }
    return bad;
}

static void check_shape(const Shape &s) {
    const int nx = s.nbx * s.block, ny = s.nby * s.block;
    int block = s.block, fuse = s.fuse;
    JacobiPlan p;
    std::string err;
    const int rc = jacobi_plan(nx, ny, block, s.niter, fuse, p, err);
    if (nx < 3 || ny < 3) {
        CHECK(rc != 0, "%d x %d accepted", nx, ny);
        return;
    }
    CHECK(rc == 0, "%d x %d block %d niter %d fuse %d refused: %s", nx, ny, s.block, s.niter, s.fuse, err.c_str());
    if (rc) return;
    VersionGraph g;
    jacobi_graph(p, g);
    const int nb = s.nbx * s.nby, n = (int)g.ntasks();
    const int S = (s.niter + s.fuse - 1) / s.fuse;
    // 4. counts
    CHECK((uint64_t)n == p.tasks && n == S * nb, "tasks %d plan %llu want %d", n, (unsigned long long)p.tasks, S * nb);
    CHECK(p.supersteps == (uint64_t)S, "supersteps");
    CHECK(g.ids.size() == p.awaits, "awaits %zu plan %llu", g.ids.size(), (unsigned long long)p.awaits);
    // 1. the CSR
    CHECK(g.off.size() == (size_t)n + 1 && g.off[0] == 0 && g.off[n] == g.ids.size(), "off ends");
    CHECK(g.payload.size() == (size_t)4 * n, "payload size");
    uint64_t moved = 0;
    int done = 0;
    for (int t = 0; t < n; ++t) {
        CHECK(g.off[t + 1] >= g.off[t], "off not monotone at %d", t);
        const int st = t / nb, b = t % nb, bx = b / s.nby, by = b % s.nby;
        const int ts = std::min(s.fuse, s.niter - st * s.fuse);
        CHECK((int)g.payload[4 * t] == st && (int)g.payload[4 * t + 1] == bx && (int)g.payload[4 * t + 2] == by &&
                  (int)g.payload[4 * t + 3] == ts && ts >= 1,
              "payload of task %d", t);
        done += b == 0 ? ts : 0;
        // 2. the awaits: the neighbour set (by fuse, not by t_s) of the superstep before, each once
        std::multiset<uint32_t> got(g.ids.begin() + g.off[t], g.ids.begin() + g.off[t + 1]), want;
        if (st)
            for (int nbk : footprint(s, bx, by, s.fuse)) want.insert((uint32_t)((st - 1) * nb + nbk));
        CHECK(got == want, "awaits of task %d (%zu, want %zu)", t, got.size(), want.size());
        for (uint32_t a : got) CHECK((int)a < t, "task %d awaits %u", t, a);
        // bytes: the clipped regions, enumerated
        auto region = [&](int h) {
            const int i0 = bx * s.block, j0 = by * s.block;
            return (uint64_t)(std::min(i0 + s.block + h, nx) - std::max(i0 - h, 0)) *
                   (uint64_t)(std::min(j0 + s.block + h, ny) - std::max(j0 - h, 0));
        };
        moved += 8 * (region(ts) + region(ts - 1) + (uint64_t)s.block * s.block);
    }
    CHECK(done == s.niter, "the supersteps advance %d of %d iterations", done, s.niter);
    CHECK(moved == p.bytes_moved, "bytes %llu plan %llu", (unsigned long long)moved, (unsigned long long)p.bytes_moved);
    // 3. ordering
    const long bad = unordered_pairs(s, g);
    CHECK(bad == 0, "%d x %d blocks niter %d fuse %d: %ld unordered conflicting pairs", s.nbx, s.nby, s.niter, s.fuse, bad);
}

// the graph with the neighbour rule keyed on t_s instead of fuse
static VersionGraph mistaken_graph(const Shape &s) {
    const size_t nb = (size_t)s.nbx * s.nby;
    VersionGraph g(2 * nb);
    const int S = (s.niter + s.fuse - 1) / s.fuse;
    for (int st = 0; st < S; ++st) {
        const int ts = std::min(s.fuse, s.niter - st * s.fuse);
        for (int bx = 0; bx < s.nbx; ++bx)
            for (int by = 0; by < s.nby; ++by) {
                std::vector<size_t> reads;
                for (int b : footprint(s, bx, by, ts)) reads.push_back((st & 1) * nb + b);
                g.task((uint32_t)st, (uint32_t)bx, (uint32_t)by, (uint32_t)ts, ((st + 1) & 1) * nb + (size_t)bx * s.nby + by,
                       reads.data(), reads.size());
            }
    }
    return g;
}

int main() {
    int cases = 0;
    // every block grid up to 4 x 4 (1 x 1, 1 x k and k x 1 among them), niter 0 .. 9 (0, 1, below
    // fuse, a last superstep of t = 1 under fuse >= 2, ...), every fuse the block allows
    for (int nbx = 1; nbx <= 4; ++nbx)
        for (int nby = 1; nby <= 4; ++nby)
            for (int block : {3, 4})
                for (int niter = 0; niter <= 9; ++niter)
                    for (int fuse = 1; fuse <= block; ++fuse) {
                        check_shape(Shape{nbx, nby, block, niter, fuse});
                        ++cases;
                    }
    // a longer chain on a wider grid
    check_shape(Shape{6, 5, 4, 23, 3});
    check_shape(Shape{5, 7, 2, 17, 2});
    cases += 2;

    // the control: with fuse >= 2, a last superstep of t = 1 and a diagonal neighbour, awaiting by t_s is unordered
    {
        const Shape s{3, 3, 4, 7, 3};  // steps 3, 3, 1
        const long bad = unordered_pairs(s, mistaken_graph(s));
        CHECK(bad > 0, "the 4-neighbour mistake went unnoticed");
        printf("control: %ld unordered pairs in the mistaken graph\n", bad);
        const Shape ok{3, 3, 4, 6, 3};  // steps 3, 3: the same rule is then the plan's
        CHECK(unordered_pairs(ok, mistaken_graph(ok)) == 0, "control of the control");
    }

    // defaults and limits
    {
        JacobiPlan p;
        std::string err;
        for (int w = 3; w <= kJacobiMaxRegion + 8; ++w) {
            int lanes = 0, pitch = 0;
            jacobi_layout(w, lanes, pitch);
            CHECK((lanes == 16 || lanes == 32 || lanes == 64) && pitch >= w, "layout of %d", w);
            CHECK(lanes != 16 || pitch % 32 == 16, "pitch %d of %d with 16 lanes", pitch, w);
            if (w <= kJacobiMaxRegion) CHECK(3 * w * pitch <= kJacobiLdsDoubles, "region %d: %d doubles", w, 3 * w * pitch);
        }
        struct {
            int nx, ny, block, niter, fuse, ok;
        } lim[] = {{160, 80, 80, 4, 1, 1},  {162, 81, 81, 4, 1, 0}, {128, 64, 64, 4, 9, 1}, {128, 64, 64, 4, 10, 0},
                   {64, 64, 32, 4, 25, 1},  {64, 64, 32, 4, 26, 0}, {512, 512, 0, 4, 0, 0}, {2, 9, 1, 4, 1, 0},
                   {9, 9, 3, -1, 1, 0},     {9, 9, 3, 4, 4, 0},     {9, 9, 2, 4, 1, 0},     {9, 9, -3, 4, 1, 0},
                   {9, 9, 3, 4, -1, 0},     {8192, 8192, 1, 1, 1, 0}, {8190, 8190, 1, 1, 1, 1}, {9, 9, 3, 0, 0, 1}};
        for (auto &l : lim) {
            int block = l.block, fuse = l.fuse;
            const int rc = jacobi_plan(l.nx, l.ny, block, l.niter, fuse, p, err);
            CHECK((rc == 0) == (l.ok != 0), "limit %d x %d block %d niter %d fuse %d: rc %d (%s)", l.nx, l.ny, l.block, l.niter,
                  l.fuse, rc, err.c_str());
            CHECK(rc != 0 || (block >= 1 && fuse >= 1 && fuse <= block), "defaults of %d / %d", l.block, l.fuse);
            ++cases;
        }
        int block = 64, fuse = 0;
        CHECK(jacobi_plan(128, 128, block, 9, fuse, p, err) == 0 && fuse == kJacobiDefaultFuse && p.supersteps == 3,
              "default fuse");
    }

    // rhs(): the corners of the unit square and the initial estimate
    {
        std::vector<double> f(5 * 7), u(5 * 7);
        jacobi_rhs_fill(5, 7, f.data(), u.data());
        CHECK(f[0] == 0.0 && u[0] == 0.0 && u[1 * 7 + 1] == 0.0 && f[1 * 7 + 1] != 0.0, "rhs interior");
        CHECK(u[4 * 7 + 6] == f[4 * 7 + 6] && f[4 * 7 + 6] < 1e-15 && f[4 * 7 + 6] > 0, "rhs corner sin(pi)");
    }

    printf("%d cases\n", cases);
    if (g_bad) printf("Check results: %d MISMATCHES\n", g_bad);
    else printf("Check results: OK\n");
    return g_bad ? 1 : 0;
}
