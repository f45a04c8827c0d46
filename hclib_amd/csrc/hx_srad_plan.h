// hx_srad_plan.h — the plan of one Rodinia SRAD launch (srad.hip) in plain C++:
// no HIP, so a host program can build and check it (tests/cpp/srad_plan.cpp):
// the limits, the default block, the task graph, the exact counts and the
// traffic model.
//
// The program (test/performance-regression/full-apps/rodinia/srad,
// srad.ref.cpp). An image J of rows x cols floats and a rectangular region of
// interest (ROI) r1..r2 x c1..c2, both ends included. An iteration has three
// parts: a serial section on the main thread (:131-141), float sums of J and
// J^2 over the ROI that end in one scalar q0sqr; sweep 1 (:145-176), four
// directional derivatives and a diffusion coefficient c per cell, every cell
// using q0sqr; sweep 2 (:182-207), the image update from c of the cell, of its
// south and of its east neighbour. The HClib port runs each sweep as a
// hclib_forasync_future with a hclib_future_wait after it and the sums between
// them on the host thread.
//
// Grids and tasks. The image is cut into nbx x nby blocks of block x block
// cells (nbx block rows, nby block columns), nb = nbx nby. There are two image
// grids: iteration `it` reads grid it & 1 and writes grid (it + 1) & 1, so the
// reference's in-place update of sweep 2 becomes a ping-pong. Grid 0 starts as
// the upload and the answer is in grid niter & 1. Per iteration one reduce task
// R(it), then one task T(it, b) per block in row-major block order: task ids
// R(it) = it (nb + 1), T(it, b) = it (nb + 1) + 1 + b. Both sweeps of a block
// are one task: it recomputes c on the block's south row and east column from
// J, so dN..dE and c never exist outside a task.
//
// R(it) reads the ROI's blocks of grid it & 1 and makes q0sqr(it), which is the
// 64-bit datum of its one promise: a value of its own per iteration, put once.
// T(it, b) awaits R(it) and, for it >= 1, T(it - 1, b') for b' = b and its up to
// eight in-grid neighbours N(b). Its own reads reach north and west by one
// cell, south and east by two, and the north-east, south-east and south-west
// diagonals by one (c of the south and east neighbours is recomputed from J),
// so of the nine only the north-west block holds no cell the arithmetic uses
// (srad.hip stages the whole square, so that block's corner cell is loaded and
// dropped): it is awaited for the symmetry the argument below needs.
// As a VersionGraph: 2 nb image versions (grid, block) and one scalar. R(it)
// writes the scalar and reads (it & 1, b), b in the ROI's blocks; T(it, b)
// writes ((it + 1) & 1, b) and reads the scalar and (it & 1, b'), b' in N(b).
// Version 0 of a grid has no task, so iteration 0 awaits only R(0).
//
// Why these awaits order everything. N is symmetric: b' in N(b) exactly when
// b in N(b').
//  * Read after write: T(it, b) reads cells of grid it & 1 in blocks of N(b),
//    made by T(it - 1, b'), which it awaits; R(it) reads the ROI's blocks, made
//    by T(it - 1, ROI), which it awaits; T(it, b) reads q0sqr(it) from R(it).
//  * Write after read by a T: T(it, b) overwrites ((it + 1) & 1, b) =
//    ((it - 1) & 1, b), which the tasks T(it - 1, b') with b in N(b') read:
//    by symmetry b' in N(b), tasks T(it, b) awaits. Without the north-west
//    await, T(it, b) could overwrite what its north-west neighbour's south-east
//    read still loads (unless that neighbour lies in the ROI's blocks, where
//    the chain through R(it) orders the two as well).
//  * Write after read by an R: T(it + 1, b), b in the ROI, overwrites
//    (it & 1, b), which R(it) read. It awaits R(it + 1), which awaits
//    T(it, ROI), which await R(it): R(it + 1) <- T(it, ROI) <- R(it). Without
//    T awaiting R this chain is gone, and with it the order of T(it, b) after
//    the write of q0sqr(it).
//  * The version a task reads is not overwritten under it: the next writer of
//    (it & 1, b') is T(it + 1, b'), which awaits T(it, b) because b in N(b').
//  * The scalar: q0sqr(it) is written once, by R(it), and read by T(it, .),
//    which await it. R(it + 1) writes q0sqr(it + 1), another datum; it does NOT
//    wait for the T(it, b) outside the ROI's blocks, which is what lets the
//    serial sum of iteration it + 1 run under the tail of iteration it.
//
// Counts. tasks = niter (nb + 1). awaits = niter nb (every T awaits its R)
// + (niter - 1) (nroi + sum |N(b)|), nroi the ROI's blocks and sum |N(b)| =
// (3 nbx - 2)(3 nby - 2); 0 when niter = 0. The longest waiter list is R's, nb,
// or on a grid of fewer than ten blocks a T's where that is longer: T(it, b)'s
// waiters are the |N(b)| <= 9 tasks T(it + 1, .) and, in the ROI, R(it + 1).
//
// Traffic model (bytes_moved): the bytes the bodies ask of memory, without
// credit for a cache. Per iteration 4 bytes for every cell of the ROI (R), for
// every cell of a block's read region (the block, one cell north and west, two
// south and east, clipped to the grid; over all blocks (rows + 3 nbx - 3)
// (cols + 3 nby - 3) cells) and for every cell written (rows cols).
//
// Arena (arena_bytes): the two grids, each on a 256-byte line, and one line of
// 8 bytes per iteration for the phases form's scalars.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "hx_vgraph.h"

namespace hx {

constexpr int kSradForms = 2;  // HCLIB_HIP_SRAD_DAG, HCLIB_HIP_SRAD_PHASES
constexpr int kSradSide = 16;  // rows and cols are multiples of 16 (srad.ref.cpp:69-72)
constexpr int kSradMaxBlock = 64;
constexpr uint64_t kSradMaxTasks = 1ull << 26;  // as the other run_dag_group clients
// LDS floats of a task at block B: the J image (B + 3)^2 and the c image (B + 1)^2
constexpr int srad_lds_floats(int B) { return (B + 3) * (B + 3) + (B + 1) * (B + 1); }

// What block = 0 resolves to: the largest of 64, 32, 16 that divides both
// sides (0: none does). Kernel ms at block 16 / 32 / 64 (profiles/r27/srad.json,
// one MI355X, one process), ROI 0..127 squared: 2048 squared, 100
// iterations, dag 38.0 / 22.3 / 20.4, phases 23.0 / 21.2 / 21.3; 8192 squared,
// 2 iterations, dag 8.13 / 1.93 / 0.94, phases 1.84 / 1.15 / 1.10
inline int srad_default_block(int rows, int cols) {
    for (int b = 64; b >= 16; b >>= 1)
        if (rows > 0 && cols > 0 && rows % b == 0 && cols % b == 0) return b;
    return 0;
}

struct SradPlan {
    int rows = 0, cols = 0, r1 = 0, r2 = 0, c1 = 0, c2 = 0, niter = 0, block = 0, form = 0;
    int nbx = 0, nby = 0;                    // block rows, block columns
    int rb1 = 0, rb2 = 0, cb1 = 0, cb2 = 0;  // the ROI's blocks, both ends included
    uint64_t nb = 0, nroi = 0, size_r = 0;
    uint64_t tasks = 0, awaits = 0, max_waiters = 0, arena_bytes = 0, bytes_moved = 0;
};

inline size_t srad_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Checks the arguments (block = 0 is replaced by its default) and fills the
// plan with the exact counts. 0, or -1 with `err`.
inline int srad_plan(int rows, int cols, int r1, int r2, int c1, int c2, int niter, int &block, int form, SradPlan &p,
                     std::string &err) {
    auto fail = [&](const std::string &m) {
        err = m;
        return -1;
    };
    if (rows < kSradSide || cols < kSradSide || rows % kSradSide || cols % kSradSide)
        return fail("rows and cols must be positive multiples of 16 (" + std::to_string(rows) + " x " +
                    std::to_string(cols) + ")");
    if ((int64_t)rows * cols > INT32_MAX) return fail("rows * cols is above what the reference's int indices reach");
    if (block == 0) block = srad_default_block(rows, cols);
    if ((block != 16 && block != 32 && block != 64) || rows % block || cols % block)
        return fail("block " + std::to_string(block) + " is not 16, 32 or 64 dividing both sides (" +
                    std::to_string(rows) + " x " + std::to_string(cols) + ")");
    if (r1 < 0 || r2 < r1 || r2 >= rows || c1 < 0 || c2 < c1 || c2 >= cols)
        return fail("the region of interest rows " + std::to_string(r1) + ".." + std::to_string(r2) + ", columns " +
                    std::to_string(c1) + ".." + std::to_string(c2) + " is empty or outside the image");
    if (niter < 0) return fail("niter must not be negative (niter " + std::to_string(niter) + ")");
    if (form < 0 || form >= kSradForms) return fail("unknown form " + std::to_string(form));
    p = SradPlan();
    p.rows = rows, p.cols = cols, p.r1 = r1, p.r2 = r2, p.c1 = c1, p.c2 = c2, p.niter = niter, p.block = block;
    p.form = form;
    p.nbx = rows / block, p.nby = cols / block;
    p.nb = (uint64_t)p.nbx * p.nby;
    p.rb1 = r1 / block, p.rb2 = r2 / block, p.cb1 = c1 / block, p.cb2 = c2 / block;
    p.nroi = (uint64_t)(p.rb2 - p.rb1 + 1) * (p.cb2 - p.cb1 + 1);
    p.size_r = (uint64_t)(r2 - r1 + 1) * (c2 - c1 + 1);
    p.tasks = (uint64_t)niter * (p.nb + 1);
    if (p.tasks >= kSradMaxTasks) return fail(std::to_string(p.tasks) + " tasks (at most 2^26): use a larger block");
    const uint64_t nsum = (uint64_t)(3 * p.nbx - 2) * (3 * p.nby - 2);
    p.awaits = niter ? (uint64_t)niter * p.nb + (uint64_t)(niter - 1) * (p.nroi + nsum) : 0;
    if (p.awaits >= (1ull << 32)) return fail(std::to_string(p.awaits) + " awaits (at most 2^32): use a larger block");
    p.max_waiters = niter ? p.nb : 0;
    if (niter >= 2 && p.nb < 10)  // a small grid: a T's waiters can outnumber R's
        for (int bi = 0; bi < p.nbx; ++bi)
            for (int bj = 0; bj < p.nby; ++bj) {
                const uint64_t nr = 1 + (bi > 0) + (bi + 1 < p.nbx), nc = 1 + (bj > 0) + (bj + 1 < p.nby);
                const bool in_roi = bi >= p.rb1 && bi <= p.rb2 && bj >= p.cb1 && bj <= p.cb2;
                if (nr * nc + in_roi > p.max_waiters) p.max_waiters = nr * nc + in_roi;
            }
    const uint64_t cells = (uint64_t)rows * cols;
    p.arena_bytes = 2 * srad_up256(cells * 4) + srad_up256((uint64_t)niter * 8);
    p.bytes_moved = (uint64_t)niter * 4 *
                    (p.size_r + (uint64_t)(rows + 3 * p.nbx - 3) * (uint64_t)(cols + 3 * p.nby - 3) + cells);
    return 0;
}

// The task graph: payload {kind (0 R, 1 T), it, block row, block column},
// awaits as the header comment says. The controls of tests/cpp/srad_plan.cpp,
// never a launch's graph: `northwest` = false leaves the north-west block out
// of T's reads; `await_r` = false leaves the scalar out of them.
inline void srad_graph(const SradPlan &p, VersionGraph &g, bool northwest = true, bool await_r = true) {
    const size_t nb = (size_t)p.nb, scalar = 2 * nb;
    g = VersionGraph(2 * nb + 1);
    g.reserve(p.tasks, 10);
    std::vector<size_t> reads;
    for (int it = 0; it < p.niter; ++it) {
        const size_t rd = (size_t)(it & 1) * nb, wr = (size_t)((it + 1) & 1) * nb;
        reads.clear();
        for (int bi = p.rb1; bi <= p.rb2; ++bi)
            for (int bj = p.cb1; bj <= p.cb2; ++bj) reads.push_back(rd + (size_t)bi * p.nby + bj);
        g.task(0u, (uint32_t)it, 0u, 0u, scalar, reads.data(), reads.size());
        for (int bi = 0; bi < p.nbx; ++bi)
            for (int bj = 0; bj < p.nby; ++bj) {
                reads.clear();
                if (await_r) reads.push_back(scalar);
                for (int di = -1; di <= 1; ++di)
                    for (int dj = -1; dj <= 1; ++dj) {
                        const int ni = bi + di, nj = bj + dj;
                        if (ni < 0 || ni >= p.nbx || nj < 0 || nj >= p.nby) continue;
                        if (!northwest && di == -1 && dj == -1) continue;
                        reads.push_back(rd + (size_t)ni * p.nby + nj);
                    }
                g.task(1u, (uint32_t)it, (uint32_t)bi, (uint32_t)bj, wr + (size_t)bi * p.nby + bj, reads.data(),
                       reads.size());
            }
    }
}

}  // namespace hx
