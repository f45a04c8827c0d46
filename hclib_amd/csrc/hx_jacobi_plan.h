// hx_jacobi_plan.h — the plan of one Kastors Jacobi launch (jacobi.hip) in
// plain C++: no HIP, so a host program can build and check it
// (tests/cpp/jacobi_plan.cpp): the limits, the supersteps, the task graph and
// the closed-form counts.
//
// Supersteps. niter sweeps are run as S = ceil(niter / fuse) supersteps;
// superstep s advances every block by t_s = min(fuse, niter - s fuse) sweeps.
// There are two device buffers: superstep s reads buffer s & 1 and writes
// buffer (s + 1) & 1, buffer 0 starts as the uploaded unew0, and the answer is
// in buffer S & 1. The reference's copy phase (u = unew) has no counterpart:
// the ping-pong gives the same bits.
//
// Tasks. One task per block per superstep, superstep-major, then in the
// reference's block order (block_x outer, block_y inner: jacobi-block-task.c
// :87-88; block_x counts rows i, block_y columns j). The VersionGraph has
// 2 nbx nby blocks, (buffer, bx, by). Task (s, b) writes ((s + 1) & 1, b) and
// reads (s & 1, b') for b' = b and b's in-grid neighbours: the 4 edge
// neighbours when fuse == 1, all 8 when fuse >= 2 (a halo t >= 2 wide reaches
// the diagonal blocks; fuse <= block keeps it inside the adjacent ones).
// Version 0, the upload, has no task: superstep 0 awaits nothing.
//
// Why these reads also order the overwrites. Task (s, b) overwrites the old
// contents of ((s + 1) & 1, b) = ((s - 1) & 1, b). Those were read only by the
// tasks (s - 1, b') that have b in their neighbourhood; neighbourhoods are
// symmetric, so these are the tasks (s - 1, b') with b' in b's neighbourhood,
// which are exactly the tasks whose output (s, b) awaits. So a read-after-write
// await of every neighbour doubles as the write-after-read order, provided the
// neighbour set is the same in every superstep of a launch. With fuse >= 2 the
// last superstep may have t = 1 and would need only 4 neighbours for its own
// reads; it must still await all 8, or it could overwrite a corner halo that a
// diagonal task of the superstep before is still reading. That is why the rule
// keys on fuse and not on t_s. (Older writers are ordered transitively: task
// (s, b) awaits (s - 1, b), which awaits (s - 2, b), the block's writer before.)
//
// LDS. A task keeps three images of its region in LDS, two of u (the sweeps
// ping-pong between them) and one of f, each W rows of `pitch` doubles with
// W = block + 2 fuse. Lanes run along j, lanes_j = 16, 32 or 64 of them per
// row, whichever pads a W-wide row least (ties: the wider); with 16 the two
// rows that one 32-lane group of a ds_read_b64 touches must fall on different
// halves of the 32 8-byte banks, so the pitch is rounded up to 16 mod 32
// doubles; with 32 or 64 a group reads one row and any pitch is free of
// conflicts. Limit: 3 W pitch doubles within kJacobiLdsDoubles, which is
// W = block + 2 fuse <= 82: block 80 at fuse 1, block 64 up to fuse 9,
// block 32 up to fuse 25. The reference's default block of 128 does not fit
// (one image of 130 x 130 doubles is 132 KiB of the CU's 160 KiB).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "hx_vgraph.h"

namespace hx {

constexpr int kJacobiDefaultBlock = 128;  // run()'s default (poisson.c:99-103)
// What fuse = 0 resolves to (clipped to the block and to the LDS limit, see
// jacobi_default_fuse): the depth the record favours at the grid far beyond
// the Infinity Cache. 8192 x 8192, 64 sweeps, kernel ms at fuse 1 / 2 / 4 /
// the largest that fits (profiles/r20/jacobi.json, one MI355X, one process):
// block 64: 58.0 / 40.1 / 27.8 / 29.0 (fuse 9); block 32: 128.5 / 61.7 / 35.7
// / 68.1 (fuse 25). Past 4 the recomputed halo and the longer body of the one
// workgroup a CU holds cost what the saved traffic and tasks gain.
constexpr int kJacobiDefaultFuse = 4;
constexpr uint64_t kJacobiMaxTasks = 1ull << 26;  // as the other run_dag_group clients
// static LDS of the largest kernel form: 159 KiB of the CU's 160, the rest is
// run_dag_group's own
constexpr int kJacobiLdsDoubles = 159 * 1024 / 8;
constexpr int kJacobiMaxRegion = 82;  // the largest block + 2 fuse (derived above, checked in jacobi_plan)

struct JacobiPlan {
    int nx = 0, ny = 0, block = 0, fuse = 0, niter = 0;
    int nbx = 0, nby = 0;
    int lanes_j = 0, pitch = 0;  // the LDS layout of a task's region
    int lds_doubles = 0;         // 3 * (block + 2 fuse) * pitch
    uint64_t supersteps = 0, tasks = 0, awaits = 0, bytes_moved = 0;
};

// lanes along j and the row pitch (doubles) for regions up to w wide
inline void jacobi_layout(int w, int &lanes_j, int &pitch) {
    int best = 0, pad = 0;
    for (int l = 16; l <= 64; l *= 2) {
        const int p = (w + l - 1) / l * l;
        if (!best || p <= pad) best = l, pad = p;
    }
    lanes_j = best;
    pitch = w;
    if (best == 16)
        while (pitch % 32 != 16) ++pitch;
}

// fuse = 0: kJacobiDefaultFuse, or the largest below it that the block and the LDS allow
inline int jacobi_default_fuse(int block) {
    int f = kJacobiDefaultFuse;
    if (f > block) f = block;
    if (block + 2 * f > kJacobiMaxRegion) f = (kJacobiMaxRegion - block) / 2;
    return f < 1 ? 1 : f;
}

// sweeps of superstep s
inline int jacobi_step(const JacobiPlan &p, uint64_t s) {
    const int64_t left = (int64_t)p.niter - (int64_t)s * p.fuse;
    return (int)(left < p.fuse ? left : p.fuse);
}

// the in-grid neighbourhood of block (bx, by), itself first, as block indices bx nby + by
inline int jacobi_neighbours(const JacobiPlan &p, int bx, int by, size_t out[9]) {
    int n = 0;
    out[n++] = (size_t)bx * p.nby + by;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy) {
            if ((!dx && !dy) || (p.fuse == 1 && dx && dy)) continue;
            const int x = bx + dx, y = by + dy;
            if (x < 0 || y < 0 || x >= p.nbx || y >= p.nby) continue;
            out[n++] = (size_t)x * p.nby + y;
        }
    return n;
}

// Checks the arguments (block = 0 and fuse = 0 are replaced by their defaults)
// and fills the plan with the closed-form counts. 0, or -1 with `err`.
inline int jacobi_plan(int nx, int ny, int &block, int niter, int &fuse, JacobiPlan &p, std::string &err) {
    auto fail = [&](const std::string &m) {
        err = m;
        return -1;
    };
    if (nx < 3 || ny < 3) return fail("the grid must be at least 3 x 3");
    if (block < 0 || fuse < 0 || niter < 0) return fail("block, fuse and niter must not be negative");
    if (block == 0) block = kJacobiDefaultBlock;
    if (nx % block || ny % block)  // poisson.c:121-126
        return fail("blocsize must divide NX and NY (block " + std::to_string(block) + ")");
    if (fuse == 0) fuse = jacobi_default_fuse(block);
    if (fuse > block)
        return fail("fuse " + std::to_string(fuse) + " is above the block size " + std::to_string(block) +
                    " (a halo must not reach past the adjacent block)");
    p = JacobiPlan();
    p.nx = nx, p.ny = ny, p.block = block, p.fuse = fuse, p.niter = niter;
    p.nbx = nx / block, p.nby = ny / block;
    const int w = block + 2 * fuse;
    if (w > kJacobiMaxRegion)
        return fail("block " + std::to_string(block) + " + 2 * fuse " + std::to_string(fuse) + " is above " +
                    std::to_string(kJacobiMaxRegion) + ": three images of a task's region must fit the CU's LDS");
    jacobi_layout(w, p.lanes_j, p.pitch);
    p.lds_doubles = 3 * w * p.pitch;
    if (p.lds_doubles > kJacobiLdsDoubles) return fail("the LDS layout does not fit");  // (never: w <= 82 fits)
    const uint64_t nb = (uint64_t)p.nbx * p.nby;
    p.supersteps = ((uint64_t)niter + fuse - 1) / fuse;
    p.tasks = p.supersteps * nb;
    if (p.tasks >= kJacobiMaxTasks)
        return fail(std::to_string(p.tasks) + " tasks (at most 2^26): use a larger block or fuse");
    // per superstep after the first: every block itself, each adjacent pair
    // twice, and with fuse >= 2 each diagonal pair twice
    const uint64_t ax = (uint64_t)(p.nbx - 1), ay = (uint64_t)(p.nby - 1);
    uint64_t per = nb + 2 * (ax * p.nby + ay * p.nbx);
    if (fuse >= 2) per += 4 * ax * ay;
    p.awaits = p.supersteps ? (p.supersteps - 1) * per : 0;
    // a region of halo h, clipped: the end blocks lose all of h, so the rows of
    // all blocks sum to nx + 2 h (nbx - 1); likewise the columns
    auto cells = [&](int h) { return ((uint64_t)nx + 2ull * h * ax) * ((uint64_t)ny + 2ull * h * ay); };
    auto step_bytes = [&](int t) { return 8 * (cells(t) + cells(t - 1) + cells(0)); };
    const uint64_t full = (uint64_t)niter / fuse;
    p.bytes_moved = full * step_bytes(fuse);
    if (niter % fuse) p.bytes_moved += step_bytes(niter % fuse);
    return 0;
}

// The task graph: payload {s, bx, by, t_s}, awaits as the header comment says.
inline void jacobi_graph(const JacobiPlan &p, VersionGraph &g) {
    const size_t nb = (size_t)p.nbx * p.nby;
    g = VersionGraph(2 * nb);
    g.reserve(p.tasks, p.fuse == 1 ? 5 : 9);
    for (uint64_t s = 0; s < p.supersteps; ++s) {
        const size_t rd = (s & 1) * nb, wr = ((s + 1) & 1) * nb;
        const int t = jacobi_step(p, s);
        for (int bx = 0; bx < p.nbx; ++bx)
            for (int by = 0; by < p.nby; ++by) {
                size_t reads[9];
                const int n = jacobi_neighbours(p, bx, by, reads);
                for (int k = 0; k < n; ++k) reads[k] += rd;
                g.task((uint32_t)s, (uint32_t)bx, (uint32_t)by, (uint32_t)t, wr + (size_t)bx * p.nby + by, reads, (size_t)n);
            }
    }
}

// rhs() and run()'s initial estimate (poisson.c:129-164, 277-354) through the
// host's libm: f holds the boundary values of sin(pi x y) and, inside, the
// right-hand side; unew0 is f on the boundary and 0 inside
inline void jacobi_rhs_fill(int nx, int ny, double *f, double *unew0) {
    const double pi = 3.141592653589793;
    for (int i = 0; i < nx; ++i) {
        const double x = (double)i / (double)(nx - 1);
        for (int j = 0; j < ny; ++j) {
            const double y = (double)j / (double)(ny - 1);
            const bool edge = i == 0 || i == nx - 1 || j == 0 || j == ny - 1;
            const double sn = sin(pi * x * y);
            const double v = edge ? sn : -(-pi * pi * (x * x + y * y) * sn);
            const size_t at = (size_t)i * ny + j;
            if (f) f[at] = v;
            if (unew0) unew0[at] = edge ? v : 0.0;
        }
    }
}

}  // namespace hx
