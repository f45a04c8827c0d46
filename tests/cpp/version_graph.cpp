// The version-graph builder (hclib_amd/csrc/hx_vgraph.h) against a naive
// restatement: a task awaits, for each block it reads and in the order of the
// reads, the last earlier task that wrote the block, found by scanning back;
// a block nobody wrote yet (version 0) gives no await. Built with
// -fsanitize=address,undefined by tests/test_version_graph.py.
#include "hx_vgraph.h"

#include <stdio.h>

#include <vector>

namespace {

struct Task {
    uint32_t pl[4];
    size_t writes;
    std::vector<size_t> reads;
};

int failures = 0;

void check(const char *name, size_t nblocks, const std::vector<Task> &prog, const std::vector<uint32_t> *want_ids) {
    hx::VersionGraph g(nblocks);
    g.reserve(prog.size(), 3);
    for (const Task &t : prog) {
        // (the builder takes its reads as a braced list: the streams here have at most three)
        const std::vector<size_t> &r = t.reads;
        if (r.size() == 0) g.task(t.pl[0], t.pl[1], t.pl[2], t.pl[3], t.writes, {});
        else if (r.size() == 1) g.task(t.pl[0], t.pl[1], t.pl[2], t.pl[3], t.writes, {r[0]});
        else if (r.size() == 2) g.task(t.pl[0], t.pl[1], t.pl[2], t.pl[3], t.writes, {r[0], r[1]});
        else g.task(t.pl[0], t.pl[1], t.pl[2], t.pl[3], t.writes, {r[0], r[1], r[2]});
    }
    std::vector<uint32_t> payload, off(1, 0), ids;
    for (size_t t = 0; t < prog.size(); ++t) {
        payload.insert(payload.end(), prog[t].pl, prog[t].pl + 4);
        for (size_t r : prog[t].reads)
            for (size_t s = t; s-- > 0;)
                if (prog[s].writes == r) {
                    ids.push_back((uint32_t)s);
                    break;
                }
        off.push_back((uint32_t)ids.size());
    }
    bool ok = g.ntasks() == prog.size() && g.payload == payload && g.off == off && g.ids == ids;
    if (want_ids) ok = ok && g.ids == *want_ids;
    printf("%s: %zu tasks, %zu awaits: %s\n", name, prog.size(), ids.size(), ok ? "ok" : "MISMATCH");
    if (!ok) ++failures;
}

// cholesky.cpp:80-124 over the lower triangle's tiles, (j, i) at j (j + 1) / 2 + i
std::vector<Task> cholesky_program(uint32_t nt) {
    auto tidx = [](uint32_t j, uint32_t i) { return (size_t)j * (j + 1) / 2 + i; };
    std::vector<Task> p;
    for (uint32_t k = 0; k < nt; ++k) {
        p.push_back({{0, k, k, k}, tidx(k, k), {tidx(k, k)}});
        for (uint32_t j = k + 1; j < nt; ++j) p.push_back({{1, k, j, k}, tidx(j, k), {tidx(j, k), tidx(k, k)}});
        for (uint32_t j = k + 1; j < nt; ++j) {
            for (uint32_t i = k + 1; i < j; ++i)
                p.push_back({{3, k, j, i}, tidx(j, i), {tidx(j, i), tidx(i, k), tidx(j, k)}});
            p.push_back({{2, k, j, j}, tidx(j, j), {tidx(j, j), tidx(j, k)}});
        }
    }
    return p;
}

}  // namespace

int main() {
    const std::vector<uint32_t> none;
    // a block read before any write: no await
    check("read before write", 3, {{{7, 1, 2, 3}, 0, {1, 2}}}, &none);
    // read after write: the reader awaits the writer, and only the newest one
    const std::vector<uint32_t> raw = {0, 1};
    check("read after write", 2, {{{1, 0, 0, 0}, 0, {}}, {{2, 0, 0, 0}, 1, {0}}, {{3, 0, 0, 0}, 1, {1}}}, &raw);
    // write after write, neither reading the block: no await between them; the reader sees the second
    const std::vector<uint32_t> waw = {1};
    check("write after write", 2, {{{1, 0, 0, 0}, 0, {}}, {{2, 0, 0, 0}, 0, {}}, {{3, 0, 0, 0}, 1, {0}}}, &waw);
    // in-place updates chain: each awaits the one before
    const std::vector<uint32_t> chain = {0, 1};
    check("update in place", 1, {{{1, 0, 0, 0}, 0, {0}}, {{2, 0, 0, 0}, 0, {0}}, {{3, 0, 0, 0}, 0, {0}}}, &chain);
    // one block read twice: awaited twice, in the order of the reads
    const std::vector<uint32_t> twice = {0, 1, 0};
    check("read twice", 3, {{{1, 0, 0, 0}, 0, {}}, {{2, 0, 0, 0}, 1, {}}, {{3, 0, 0, 0}, 2, {0, 1, 0}}}, &twice);
    // Cholesky's program order for 1, 2 and 3 tile rows
    check("cholesky 1", 1, cholesky_program(1), &none);
    const std::vector<uint32_t> chol2 = {0, 1, 2};  // trsm <- potrf; syrk <- trsm; potrf(1) <- syrk
    check("cholesky 2", 3, cholesky_program(2), &chol2);
    check("cholesky 3", 6, cholesky_program(3), nullptr);
    if (cholesky_program(3).size() != 10) {
        printf("cholesky 3: %zu tasks, want 10\n", cholesky_program(3).size());
        ++failures;
    }
    printf(failures ? "FAILED\n" : "Check results: OK\n");
    return failures ? 1 : 0;
}
