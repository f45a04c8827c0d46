// cfd_plan.cpp — hclib_amd/csrc/hx_cfd_plan.h and hx_cfd_host.h as a host
// program (run by tests/test_cfd_plan.py under AddressSanitizer and UBSan).
// Over every fixture of tests/golden/cfd (as plain text in the folder argv[1]) and a few hundred seeded
// meshes, at blocks 8, 16, 64 and 24 and iterations 0 .. 3, it checks that
//   1. the await CSR is well formed and no task awaits a task twice,
//   2. any two tasks that touch the same (buffer, block), the same block of old
//      or the same block of step_factors, at least one of them writing it, are
//      ordered: one is an ancestor of the other along the awaits (a task's
//      footprint is taken from what its body does, element by element and face
//      by face, not from the plan's neighbourhoods),
//   3. the counts equal the plan's (what hclib_hip_cfd_bounds reports), each
//      from an enumeration over the graph or over the elements.
// As a control the same checker is run on the graph built without the reverse
// edges (N(b) without the blocks that name b) and must find the hub fixture
// unordered.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "hx_cfd_host.h"
#include "hx_cfd_plan.h"

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

struct Mesh {
    int nel = 0, nelr = 0;
    std::vector<double> areas, normals;
    std::vector<int> nbs;
};

// the graph of cfd_graph over neighbourhoods given as CSR
static VersionGraph graph_of(int nblocks, int stages, const std::vector<uint32_t> &noff, const std::vector<uint32_t> &nids) {
    CfdPlan p;
    p.nblocks = nblocks;
    p.stages = (uint64_t)stages;
    p.tasks = (uint64_t)stages * nblocks;
    p.noff = noff;
    p.nids = nids;
    VersionGraph g;
    cfd_graph(p, g);
    return g;
}

// unordered conflicting pairs of the graph (property 2); -1: not a DAG in id order
static long unordered_pairs(const Mesh &m, int block, const VersionGraph &g) {
    const int nb = (m.nelr + block - 1) / block, n = (int)g.ntasks();
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
    // resources: (buffer, block) 0 .. 2 nb, old of a block 2 nb .. 3 nb, step_factors of a block 3 nb .. 4 nb
    std::vector<std::vector<int>> wr(4 * nb), rd(4 * nb);
    for (int t = 0; t < n; ++t) {
        const int st = (int)g.payload[4 * t], b = (int)g.payload[4 * t + 1], j = st % kCfdRk;
        wr[((st + 1) & 1) * nb + b].push_back(t);
        std::set<int> reads;
        for (int i = b * block; i < std::min((b + 1) * block, m.nelr); ++i) {
            reads.insert(i / block);
            for (int f = 0; f < kCfdNnb; ++f)
                if (m.nbs[(size_t)i * kCfdNnb + f] >= 0) reads.insert(m.nbs[(size_t)i * kCfdNnb + f] / block);
        }
        for (int r : reads) rd[(st & 1) * nb + r].push_back(t);
        (j == 0 ? wr : rd)[2 * nb + b].push_back(t);
        (j == 0 ? wr : rd)[3 * nb + b].push_back(t);
    }
    long bad = 0;
    for (int v = 0; v < 4 * nb; ++v)
        for (size_t i = 0; i < wr[v].size(); ++i) {
            for (size_t j = i + 1; j < wr[v].size(); ++j)
                if (!ordered(std::min(wr[v][i], wr[v][j]), std::max(wr[v][i], wr[v][j]))) ++bad;
            for (int r : rd[v])
                if (r != wr[v][i] && !ordered(std::min(r, wr[v][i]), std::max(r, wr[v][i]))) ++bad;
        }
    return bad;
}

static void check_case(const char *name, const Mesh &m, int block_in, int iterations) {
    int block = block_in;
    CfdPlan p;
    std::string err;
    const int rc = cfd_plan(m.nel, m.nbs.data(), iterations, block, 0, p, err);
    CHECK(rc == 0, "%s block %d iterations %d refused: %s", name, block_in, iterations, err.c_str());
    if (rc) return;
    VersionGraph g;
    cfd_graph(p, g);
    const int nb = (m.nelr + block - 1) / block, S = kCfdRk * iterations, n = (int)g.ntasks();
    // 3. the counts
    CHECK(p.nelr == m.nelr && p.nblocks == nb && p.stages == (uint64_t)S, "%s: nelr, nblocks or stages", name);
    CHECK((uint64_t)n == p.tasks && n == S * nb, "%s: tasks %d plan %llu want %d", name, n, (unsigned long long)p.tasks, S * nb);
    CHECK(g.ids.size() == p.awaits, "%s: awaits %zu plan %llu", name, g.ids.size(), (unsigned long long)p.awaits);
    std::vector<uint32_t> waiters(n ? n : 1, 0);
    for (uint32_t a : g.ids) ++waiters[a];
    const uint64_t longest = n ? *std::max_element(waiters.begin(), waiters.end()) : 0;
    CHECK(longest == p.max_waiters, "%s block %d iterations %d: longest waiter list %llu plan %llu", name, block, iterations,
          (unsigned long long)longest, (unsigned long long)p.max_waiters);
    uint64_t moved = 0;
    for (int t = 0; t < n; ++t) {
        const int b = (int)g.payload[4 * t + 1], j = (int)g.payload[4 * t + 2];
        for (int i = b * block; i < std::min((b + 1) * block, m.nelr); ++i) {
            moved += 40 + 40 + 16 + 96 + (j == 0 ? 8 + 48 : 48);
            for (int f = 0; f < kCfdNnb; ++f) moved += m.nbs[(size_t)i * kCfdNnb + f] >= 0 ? 40 : 0;
        }
    }
    CHECK(moved == p.bytes_moved, "%s: bytes %llu plan %llu", name, (unsigned long long)moved, (unsigned long long)p.bytes_moved);
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t e = (size_t)m.nelr;
    CHECK(p.arena_bytes == up(8 * e) + up(16 * e) + up(96 * e) + 3 * 5 * up(8 * e) + up(8 * e), "%s: arena bytes", name);
    // 1. the CSR
    CHECK(g.off.size() == (size_t)n + 1 && g.off[0] == 0 && g.off[n] == g.ids.size(), "%s: off ends", name);
    CHECK(g.payload.size() == (size_t)4 * n, "%s: payload size", name);
    for (int t = 0; t < n; ++t) {
        CHECK(g.off[t + 1] >= g.off[t], "%s: off not monotone at %d", name, t);
        const int st = t / nb, b = t % nb;
        CHECK((int)g.payload[4 * t] == st && (int)g.payload[4 * t + 1] == b && (int)g.payload[4 * t + 2] == st % kCfdRk,
              "%s: payload of task %d", name, t);
        std::set<uint32_t> once(g.ids.begin() + g.off[t], g.ids.begin() + g.off[t + 1]);
        CHECK(once.size() == g.off[t + 1] - g.off[t], "%s: task %d awaits a task twice", name, t);
        CHECK(st == 0 ? once.empty() : once.count((uint32_t)(t - nb)) == 1, "%s: task %d and its own block", name, t);
        for (uint32_t a : once) CHECK((int)a / nb == st - 1, "%s: task %d awaits %u, not of the stage before", name, t, a);
    }
    // the neighbourhoods are symmetric
    for (int b = 0; b < nb; ++b)
        for (uint32_t k = p.noff[b]; k < p.noff[b + 1]; ++k) {
            const uint32_t o = p.nids[k];
            CHECK(std::binary_search(p.nids.begin() + p.noff[o], p.nids.begin() + p.noff[o + 1], (uint32_t)b),
                  "%s: block %d has %u but not the reverse", name, b, o);
        }
    // 2. ordering
    const long bad = unordered_pairs(m, block, g);
    CHECK(bad == 0, "%s block %d iterations %d: %ld unordered conflicting pairs", name, block, iterations, bad);
}

static bool read_fixture(const std::string &path, Mesh &m) {
    std::string err;
    if (cfd_read_input(path.c_str(), 0, nullptr, nullptr, nullptr, m.nel, m.nelr, err)) {
        CHECK(false, "%s", err.c_str());
        return false;
    }
    m.areas.resize(m.nelr);
    m.nbs.resize((size_t)m.nelr * kCfdNnb);
    m.normals.resize((size_t)m.nelr * kCfdNnb * kCfdNdim);
    int nel = 0, nelr = 0;
    const int rc = cfd_read_input(path.c_str(), m.nel, m.areas.data(), m.nbs.data(), m.normals.data(), nel, nelr, err);
    CHECK(rc == 0 && nel == m.nel && nelr == m.nelr, "%s: %s", path.c_str(), err.c_str());
    return rc == 0;
}

static uint32_t g_rng = 1;
static uint32_t rnd(uint32_t n) {  // 0 .. n - 1
    g_rng = g_rng * 1664525u + 1013904223u;
    return (uint32_t)(((uint64_t)(g_rng >> 8) * n) >> 24);
}

// a ring with chords; a face is the wing, the far field or a one-directional jump (also into the padding) with
// probability 1/10, 1/10 and 2/10
static Mesh seeded(uint32_t seed) {
    g_rng = seed * 2654435761u + 12345u;
    Mesh m;
    m.nel = 1 + (int)rnd(seed % 5 == 0 ? 700 : 150);
    m.nelr = (int)cfd_nelr(m.nel);
    m.nbs.resize((size_t)m.nelr * kCfdNnb);
    const int step[4] = {1, m.nel - 1, 7 % m.nel, m.nel - 7 % m.nel};
    for (int i = 0; i < m.nel; ++i)
        for (int f = 0; f < kCfdNnb; ++f) {
            const uint32_t u = rnd(10);
            m.nbs[(size_t)i * kCfdNnb + f] = u == 0 ? -1 : u == 1 ? -2 : u <= 3 ? (int)rnd((uint32_t)m.nelr) : (i + step[f]) % m.nel;
        }
    for (int i = m.nel; i < m.nelr; ++i)
        for (int f = 0; f < kCfdNnb; ++f) m.nbs[(size_t)i * kCfdNnb + f] = m.nbs[(size_t)(m.nel - 1) * kCfdNnb + f];
    return m;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        printf("usage: cfd_plan <folder of the fixtures' inputs>\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int blocks[4] = {8, 16, 64, 24};
    int cases = 0;
    Mesh hub;
    for (const char *name : {"tiny", "pad1", "grid", "hub", "odd"}) {
        Mesh m;
        if (!read_fixture(dir + "/" + name + ".txt", m)) continue;
        if (std::string(name) == "hub") hub = m;
        for (int block : blocks)
            for (int it = 0; it <= 3; ++it) {
                check_case(name, m, block, it);
                ++cases;
            }
    }
    for (uint32_t seed = 1; seed <= 300; ++seed) {
        const Mesh m = seeded(seed);
        const std::string name = "seed " + std::to_string(seed);
        for (int it = 0; it <= 3; ++it) {
            check_case(name.c_str(), m, blocks[seed % 4], it);
            ++cases;
        }
    }

    // the fixtures are what their names say
    if (hub.nel) {
        CfdPlan p;
        std::string err;
        int block = 8;
        CHECK(cfd_plan(hub.nel, hub.nbs.data(), 5, block, 0, p, err) == 0, "hub: %s", err.c_str());
        CHECK(p.nblocks >= 67 && p.max_waiters > 64 && p.noff[1] - p.noff[0] == (uint32_t)p.nblocks, "hub: block 0's list");
        std::vector<uint32_t> noff, nids;
        cfd_neighbourhoods(hub.nelr, hub.nbs.data(), 8, false, noff, nids);
        CHECK(noff[1] - noff[0] == 1, "hub: block 0 names another block");
        // the control: without the reverse edges the overwrite of block 0 is not ordered behind its readers
        const long bad = unordered_pairs(hub, 8, graph_of(p.nblocks, 6, noff, nids));
        CHECK(bad > 0, "the graph without the reverse edges went unnoticed");
        printf("control: %ld unordered pairs in the graph without the reverse edges\n", bad);
        CHECK(unordered_pairs(hub, 8, graph_of(p.nblocks, 6, p.noff, p.nids)) == 0, "control of the control");
    }

    // limits
    {
        Mesh m = seeded(7);
        struct {
            int nel, iterations, block, form, ok;
        } lim[] = {{m.nel, 5, 0, 0, 1},  {m.nel, 5, 0, 1, 1},    {m.nel, 5, 0, 2, 0},  {m.nel, 5, 0, -1, 0}, {m.nel, -1, 8, 0, 0},
                   {0, 5, 8, 0, 0},      {-3, 5, 8, 0, 0},       {m.nel, 5, 4, 0, 0},  {m.nel, 5, 12, 0, 0}, {m.nel, 5, 1032, 0, 0},
                   {m.nel, 5, 1024, 0, 1}, {m.nel, 5, -8, 0, 0}, {m.nel, 0, 8, 0, 1},  {INT32_MAX, 1, 8, 0, 0}};
        for (auto &l : lim) {
            CfdPlan p;
            std::string err;
            int block = l.block;
            const int rc = cfd_plan(l.nel, m.nbs.data(), l.iterations, block, l.form, p, err);
            CHECK((rc == 0) == (l.ok != 0), "limit nel %d iterations %d block %d form %d: rc %d (%s)", l.nel, l.iterations,
                  l.block, l.form, rc, err.c_str());
            CHECK(rc != 0 || l.block != 0 || block == kCfdDefaultBlock, "the default block");
            ++cases;
        }
        // a neighbour index: nelr - 1 (a padded copy) is accepted, nelr refused
        CfdPlan p;
        std::string err;
        int block = 8;
        m.nbs[1] = m.nelr - 1;
        CHECK(cfd_plan(m.nel, m.nbs.data(), 1, block, 0, p, err) == 0, "index nelr - 1 refused: %s", err.c_str());
        m.nbs[1] = m.nelr;
        CHECK(cfd_plan(m.nel, m.nbs.data(), 1, block, 0, p, err) != 0, "index nelr accepted");
        CHECK(cfd_plan(m.nel, nullptr, 1, block, 0, p, err) != 0, "NULL accepted");
        // 2^26 tasks: 8 elements a block, 3 stages an iteration
        Mesh big;
        big.nel = 8 * 1024;
        big.nbs.assign((size_t)big.nel * kCfdNnb, -2);
        CHECK(cfd_plan(big.nel, big.nbs.data(), 21845, block, 0, p, err) == 0 && p.tasks == 3ull * 21845 * 1024, "below 2^26");
        CHECK(cfd_plan(big.nel, big.nbs.data(), 21846, block, 0, p, err) != 0, "2^26 tasks accepted");
        cases += 5;
    }

    // the far field (:383-408): mach 1.2 at angle 0 over a sound speed of 1
    {
        CfdFarField ff;
        cfd_far_field(ff);
        CHECK(ff.variable[0] == 1.4 && ff.variable[1] == 1.4 * 1.2 && ff.variable[2] == 0.0 && ff.variable[3] == 0.0, "far field");
        CHECK(ff.momentum_x[0] == 1.2 * (1.4 * 1.2) + 1.0 && ff.momentum_y[1] == 1.0 && ff.momentum_z[2] == 1.0, "far field flux");
    }

    printf("%d cases\n", cases);
    if (g_bad) printf("Check results: %d MISMATCHES\n", g_bad);
    else printf("Check results: OK\n");
    return g_bad ? 1 : 0;
}
