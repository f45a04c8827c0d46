// bfs_plan.cpp — hclib_amd/csrc/hx_bfs_plan.h as a host program (run by
// tests/test_bfs_plan.py under AddressSanitizer and UBSan). It checks that
//   1. a graph the plan accepts is one the kernel can walk without an index
//      check: the walk below (the level form's, serially) touches order,
//      lvl_off, cost and edges only inside arrays of exactly the sizes the
//      arena gives them, which ASan watches;
//   2. the arena's parts are 256-aligned, in order and disjoint, and the
//      bounds are the closed forms;
//   3. every mutation of a good graph that the header lists is refused, with
//      arrays allocated at their exact sizes (a check that read first and
//      refused afterwards would trip ASan);
//   4. the walk's close count is the protocol's: level L closes at done ==
//      (vertices in levels <= L) + (their degrees summed), and the targets
//      grow strictly;
//   5. bfs_read_input sizes, fills and refuses as the header says, on files
//      written here.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "hx_bfs_plan.h"

using namespace hx;

static int g_bad = 0, g_cases = 0, g_refused = 0;
#define CHECK(cond, ...)          \
    do {                          \
        if (!(cond)) {            \
            ++g_bad;              \
            printf("MISMATCH: "); \
            printf(__VA_ARGS__);  \
            printf("\n");         \
        }                         \
    } while (0)

struct Graph {
    std::vector<int32_t> starting, degree, edges;
    int source = 0;
};

static uint32_t g_rng = 12345;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (g_rng >> 8) % n;
}

static Graph random_graph(int n, int maxdeg) {
    Graph g;
    for (int v = 0; v < n; ++v) {
        const int d = (int)rnd((uint32_t)maxdeg + 1);
        g.starting.push_back((int32_t)g.edges.size());
        g.degree.push_back(d);
        for (int i = 0; i < d; ++i) g.edges.push_back((int32_t)rnd((uint32_t)n));
    }
    g.source = (int)rnd((uint32_t)n);
    return g;
}

static int plan(const Graph &g, int form, BfsPlan &p, std::string &err, int n_nodes = INT_MIN, int n_edges = INT_MIN) {
    // exact-size copies on the heap: one read past an end is an ASan report
    std::vector<int32_t> s(g.starting), d(g.degree), e(g.edges);
    s.shrink_to_fit(), d.shrink_to_fit(), e.shrink_to_fit();
    return bfs_plan(s.data(), d.data(), n_nodes == INT_MIN ? (int)s.size() : n_nodes, e.empty() ? nullptr : e.data(),
                    n_edges == INT_MIN ? (int)e.size() : n_edges, g.source, form, p, err);
}

// the level form, serially, inside arrays of the arena's sizes
static void walk(const Graph &g, const BfsPlan &p) {
    const size_t n = (size_t)p.n_nodes;
    CHECK(p.off_order - p.off_edges >= 4 * (size_t)p.n_edges && p.off_lvl - p.off_order >= 4 * n &&
              p.bytes - p.off_lvl >= 4 * (n + 2),
          "arena parts too small");
    std::vector<int32_t> cost(n, -1);
    std::vector<uint32_t> order(n, 0xffffffffu), lvl(n + 2, 0);
    order.shrink_to_fit(), lvl.shrink_to_fit(), cost.shrink_to_fit();
    uint64_t packed = (1ull << kBfsCountShift) + (uint64_t)g.degree[(size_t)g.source], done = 0;
    uint64_t target = 1 + (uint64_t)g.degree[(size_t)g.source], last_target = 0;
    cost[(size_t)g.source] = 0;
    order[0] = (uint32_t)g.source;
    lvl[1] = 1;
    uint32_t L = 0, off = 0, cnt = 1;
    while (cnt) {
        CHECK(target > last_target, "targets must grow");
        last_target = target;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t v = order[off + k];
            ++done;
            for (int32_t i = 0; i < g.degree[v]; ++i) {
                const int32_t id = g.edges[(size_t)(g.starting[v] + i)];
                ++done;
                if (cost[(size_t)id] == -1) {
                    cost[(size_t)id] = (int32_t)L + 1;
                    order[(size_t)(packed >> kBfsCountShift)] = (uint32_t)id;
                    packed += (1ull << kBfsCountShift) + (uint64_t)g.degree[(size_t)id];
                }
            }
            CHECK(k + 1 == cnt || done < target, "level %u would close early", L);
        }
        CHECK(done == target, "level %u: done %llu, target %llu", L, (unsigned long long)done, (unsigned long long)target);
        const uint32_t reached = (uint32_t)(packed >> kBfsCountShift);
        lvl[L + 2] = reached;
        off = lvl[L + 1];
        cnt = reached - off;
        target = reached + (packed & ((1ull << kBfsCountShift) - 1));
        ++L;
    }
    CHECK(done <= p.items, "more items than the bound");
}

static void layout(const BfsPlan &p) {
    const size_t parts[] = {p.off_cost, p.off_starting, p.off_degree, p.off_edges,
                            p.form == kBfsLevel ? p.off_order : p.bytes, p.form == kBfsLevel ? p.off_lvl : p.bytes, p.bytes};
    const size_t n4 = 4 * (size_t)p.n_nodes;
    const size_t need[] = {n4, n4, n4, 4 * (size_t)p.n_edges, n4, 4 * ((size_t)p.n_nodes + 2)};
    CHECK(parts[0] == 256, "ctl is one 256-byte line");
    for (int i = 0; i < 6; ++i) {
        CHECK(parts[i] % 256 == 0, "part %d not aligned", i);
        if (parts[i] == p.bytes) continue;
        CHECK(parts[i + 1] >= parts[i] + need[i] && parts[i + 1] - parts[i] < need[i] + 256, "part %d size", i);
    }
    CHECK(p.items == (uint64_t)p.n_nodes + (uint64_t)p.n_edges, "item bound");
    if (p.form == kBfsAsync) CHECK(p.off_order == 0 && p.off_lvl == 0, "the async form has no order");
}

static void refuse(const Graph &g, const char *word, int form = kBfsLevel, int n_nodes = INT_MIN, int n_edges = INT_MIN) {
    BfsPlan p;
    std::string err;
    const int rc = plan(g, form, p, err, n_nodes, n_edges);
    CHECK(rc == -1 && err.find(word) != std::string::npos, "not refused with '%s': rc %d '%s'", word, rc, err.c_str());
    ++g_refused;
}

static void refusals(const Graph &good) {
    Graph g = good;
    refuse(g, "form", 2);
    refuse(g, "form", -1);
    refuse(g, "n_nodes", kBfsLevel, 0);
    refuse(g, "n_nodes", kBfsLevel, -1);
    refuse(g, "n_nodes", kBfsLevel, 1 << 24);
    refuse(g, "n_edges", kBfsLevel, INT_MIN, -1);
    g.source = (int)good.starting.size();
    refuse(g, "source");
    g.source = -1;
    refuse(g, "source");
    for (size_t v = 0; v < good.starting.size(); ++v) {
        g = good;
        g.degree[v] = -1;
        refuse(g, "degree");
        g.degree[v] = 1 << 24;
        refuse(g, "degree");
        g = good;
        g.starting[v] = -1;
        refuse(g, "are outside");
        g.starting[v] = (int32_t)good.edges.size() + 1;
        refuse(g, "are outside");
        g = good;
        g.degree[v] = (int32_t)good.edges.size() - good.starting[v] + 1;
        refuse(g, "are outside");
    }
    for (size_t e = 0; e < good.edges.size(); ++e) {
        g = good;
        g.edges[e] = (int32_t)good.starting.size();
        refuse(g, "leads to vertex");
        g.edges[e] = -1;
        refuse(g, "leads to vertex");
    }
    BfsPlan p;
    std::string err;
    CHECK(bfs_plan(nullptr, good.degree.data(), 2, good.edges.data(), 1, 0, 0, p, err) == -1, "NULL starting");
    CHECK(bfs_plan(good.starting.data(), nullptr, 2, good.edges.data(), 1, 0, 0, p, err) == -1, "NULL degree");
    CHECK(bfs_plan(good.starting.data(), good.degree.data(), (int)good.starting.size(), nullptr, (int)good.edges.size(),
                   0, 0, p, err) == -1 || good.edges.empty(),
          "NULL edges");
    g_refused += 3;
}

static void files(const char *dir) {
    const std::string path = std::string(dir) + "/g.txt";
    Graph g = random_graph(9, 4);
    auto write = [&](size_t nodes, size_t edges) {
        FILE *f = fopen(path.c_str(), "w");
        fprintf(f, "%zu\n", g.starting.size());
        for (size_t v = 0; v < nodes; ++v) fprintf(f, "%d %d\n", g.starting[v], g.degree[v]);
        if (nodes == g.starting.size()) {
            fprintf(f, "\n%d\n\n%zu\n", g.source, g.edges.size());
            for (size_t e = 0; e < edges; ++e) fprintf(f, "%d %d\n", g.edges[e], 1 + (int)rnd(10));
        }
        fclose(f);
    };
    std::string err;
    int64_t counts[3] = {-1, -1, -1};
    write(g.starting.size(), g.edges.size());
    CHECK(bfs_read_input(path.c_str(), nullptr, nullptr, nullptr, counts, err) == 0, "sizing: %s", err.c_str());
    CHECK(counts[0] == (int64_t)g.starting.size() && counts[1] == (int64_t)g.edges.size() && counts[2] == g.source, "counts");
    std::vector<int32_t> s((size_t)counts[0]), d((size_t)counts[0]), e((size_t)counts[1]);
    s.shrink_to_fit(), d.shrink_to_fit(), e.shrink_to_fit();
    CHECK(bfs_read_input(path.c_str(), s.data(), d.data(), e.data(), counts, err) == 0, "filling: %s", err.c_str());
    CHECK(s == g.starting && d == g.degree && e == g.edges, "the arrays read back");
    int64_t wrong[3] = {counts[0] - 1, counts[1], 0};
    CHECK(bfs_read_input(path.c_str(), s.data(), d.data(), e.data(), wrong, err) == -1, "fewer nodes than the file");
    wrong[0] = counts[0], wrong[1] = counts[1] - 1;
    CHECK(bfs_read_input(path.c_str(), s.data(), d.data(), e.data(), wrong, err) == -1, "fewer edges than the file");
    write(g.starting.size() - 1, 0);
    CHECK(bfs_read_input(path.c_str(), nullptr, nullptr, nullptr, counts, err) == -1, "a node is missing");
    write(g.starting.size(), g.edges.size() - 1);
    CHECK(bfs_read_input(path.c_str(), nullptr, nullptr, nullptr, counts, err) == -1, "an edge is missing");
    CHECK(bfs_read_input((path + ".absent").c_str(), nullptr, nullptr, nullptr, counts, err) == -1, "no file");
    remove(path.c_str());
}

int main(int argc, char **argv) {
    for (int n = 1; n <= 40; ++n)
        for (int maxdeg = 0; maxdeg <= 6; maxdeg += 2)
            for (int form = 0; form < 2; ++form) {
                const Graph g = random_graph(n, maxdeg);
                BfsPlan p;
                std::string err;
                const int rc = plan(g, form, p, err);
                CHECK(rc == 0, "a good graph refused: %s", err.c_str());
                if (rc) continue;
                layout(p);
                if (form == kBfsLevel) walk(g, p);
                ++g_cases;
            }
    refusals(random_graph(6, 3));
    refusals(random_graph(1, 0));
    if (argc > 1) files(argv[1]);
    printf("%d cases, %d refusals\n", g_cases, g_refused);
    printf(g_bad ? "Check results: %d MISMATCHES\n" : "Check results: OK\n", g_bad);
    return g_bad ? 1 : 0;
}
