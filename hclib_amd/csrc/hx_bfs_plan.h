// hx_bfs_plan.h — the plan of one Rodinia BFS launch (bfs.hip) in plain C++:
// no HIP, so a host program can build and check it (tests/cpp/bfs_plan.cpp):
// the argument checks, the arena's layout and the item bound, and the reader
// of Rodinia's text format.
//
// The graph is Rodinia's (bfs.ref.cpp:32-36, 84-121): vertex v owns
// edges[starting[v] .. starting[v] + degree[v]). The reference indexes with
// whatever the file holds; every case in which that is undefined is refused
// here, so the kernel checks no index: a vertex id it reads is an edge head or
// the source, both in [0, n_nodes), and an edge index is below n_edges.
//
// Arena (bytes, every part 256-aligned, in this order):
//   ctl       256: [0] packed  (reached << 40 | degrees of the reached summed)
//                  [1] done    items run and flushed, monotonic
//                  [2] target  done's value that closes the open level
//                  [3] level   the open level
//   cost      4 n_nodes
//   starting  4 n_nodes
//   degree    4 n_nodes
//   edges     4 n_edges
//   level form only:
//   order     4 n_nodes        the reached vertices, level after level
//   lvl_off   4 (n_nodes + 2)  level L is order[lvl_off[L] .. lvl_off[L + 1])
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

namespace hx {

constexpr int kBfsLevel = 0, kBfsAsync = 1;  // HCLIB_HIP_BFS_LEVEL / _ASYNC
// a level's vertices are the children of one template, a vertex's edges of
// another: both counts share the scheduler's kMaxChildren (hx_sched.h)
constexpr int64_t kBfsMaxChildren = 1 << 24;
constexpr int kBfsCountShift = 40;  // ctl[0]: the reached count above the degree sum (< 2^31)

struct BfsPlan {
    int n_nodes = 0, n_edges = 0, source = 0, form = 0;
    size_t off_cost = 0, off_starting = 0, off_degree = 0, off_edges = 0, off_order = 0, off_lvl = 0;
    size_t bytes = 0;     // the whole arena
    uint64_t items = 0;   // n_nodes + n_edges: no level-form launch runs more
};

inline size_t bfs_align(size_t b) { return (b + 255) & ~(size_t)255; }

// Checks the arguments and lays the arena out. 0, or -1 with `err`.
inline int bfs_plan(const int32_t *starting, const int32_t *degree, int n_nodes, const int32_t *edges, int n_edges,
                    int source, int form, BfsPlan &p, std::string &err) {
    auto fail = [&](const std::string &m) {
        err = m;
        return -1;
    };
    if (form != kBfsLevel && form != kBfsAsync)
        return fail("form " + std::to_string(form) + " is neither HCLIB_HIP_BFS_LEVEL nor HCLIB_HIP_BFS_ASYNC");
    if (n_nodes < 1 || n_nodes >= kBfsMaxChildren)
        return fail("n_nodes = " + std::to_string(n_nodes) + " must be in [1, 2^24)");
    if (n_edges < 0) return fail("n_edges = " + std::to_string(n_edges) + " must not be negative");
    if (!starting || !degree) return fail("starting or degree is NULL");
    if (!edges && n_edges > 0) return fail("edges is NULL");
    if (source < 0 || source >= n_nodes)
        return fail("source = " + std::to_string(source) + " is outside [0, " + std::to_string(n_nodes) + ")");
    for (int v = 0; v < n_nodes; ++v) {
        const int64_t s = starting[v], d = degree[v];
        if (d < 0 || d >= kBfsMaxChildren)
            return fail("vertex " + std::to_string(v) + " has degree " + std::to_string(d) + " outside [0, 2^24)");
        if (s < 0 || s + d > n_edges)
            return fail("vertex " + std::to_string(v) + ": edges [" + std::to_string(s) + ", " + std::to_string(s + d) +
                        ") are outside [0, " + std::to_string(n_edges) + ")");
    }
    for (int e = 0; e < n_edges; ++e)
        if (edges[e] < 0 || edges[e] >= n_nodes)
            return fail("edge " + std::to_string(e) + " leads to vertex " + std::to_string(edges[e]) + " outside [0, " +
                        std::to_string(n_nodes) + ")");
    p = BfsPlan();
    p.n_nodes = n_nodes, p.n_edges = n_edges, p.source = source, p.form = form;
    const size_t nb = bfs_align(4 * (size_t)n_nodes);
    size_t at = 256;
    p.off_cost = at, at += nb;
    p.off_starting = at, at += nb;
    p.off_degree = at, at += nb;
    p.off_edges = at, at += bfs_align(4 * (size_t)n_edges);
    if (form == kBfsLevel) {
        p.off_order = at, at += nb;
        p.off_lvl = at, at += bfs_align(4 * ((size_t)n_nodes + 2));
    }
    p.bytes = at;
    p.items = (uint64_t)n_nodes + (uint64_t)n_edges;
    return 0;
}

// Rodinia's text format as the reference's fscanf sequence reads it
// (bfs.ref.cpp:84-121). With every array null it only sizes: counts = {nodes,
// edges, source}. Otherwise counts holds, on entry, the sizes of the arrays
// (as a sizing call reported them) and the file's must equal them. 0, or -1
// with `err`; a count that is negative or does not fit an int is refused.
inline int bfs_read_input(const char *path, int32_t *starting, int32_t *degree, int32_t *edges, int64_t counts[3],
                          std::string &err) {
    auto fail = [&](const std::string &m) {
        err = std::string(path ? path : "(null)") + ": " + m;
        return -1;
    };
    if (!path || !counts) return fail("path or counts is NULL");
    const bool sizing = !starting && !degree && !edges;
    if (!sizing && (!starting || !degree || (!edges && counts[1] > 0))) return fail("some arrays are NULL, not all");
    FILE *fp = fopen(path, "r");
    if (!fp) return fail("cannot be opened");
    auto close_fail = [&](const std::string &m) {
        fclose(fp);
        return fail(m);
    };
    int n = 0, m = 0, src = 0, a = 0, b = 0;
    if (fscanf(fp, "%d", &n) != 1 || n < 0) return close_fail("no node count");
    if (!sizing && n != counts[0]) return close_fail("the node count differs from the sizing call's");
    for (int i = 0; i < n; ++i) {
        if (fscanf(fp, "%d %d", &a, &b) != 2) return close_fail("node " + std::to_string(i) + " is missing");
        if (!sizing) starting[i] = a, degree[i] = b;
    }
    if (fscanf(fp, "%d", &src) != 1) return close_fail("no source");
    if (fscanf(fp, "%d", &m) != 1 || m < 0) return close_fail("no edge count");
    if (!sizing && m != counts[1]) return close_fail("the edge count differs from the sizing call's");
    for (int i = 0; i < m; ++i) {
        if (fscanf(fp, "%d", &a) != 1 || fscanf(fp, "%d", &b) != 1)
            return close_fail("edge " + std::to_string(i) + " is missing");
        if (!sizing) edges[i] = a;
    }
    fclose(fp);
    counts[0] = n, counts[1] = m, counts[2] = src;
    return 0;
}

}  // namespace hx
