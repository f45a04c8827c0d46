// hx_cfd_plan.h — the plan of one Rodinia CFD launch (cfd.hip) in plain C++:
// no HIP, so a host program can build and check it (tests/cpp/cfd_plan.cpp):
// the limits, the far field, the blocks' neighbourhoods, the task graph, the
// exact counts and the traffic model.
//
// The program (test/performance-regression/full-apps/rodinia/cfd,
// euler3d_cpu_double.ref.cpp). An unstructured mesh of nelr elements, each with
// an area and four faces; a face names a neighbour element (>= 0), the wing
// (-1) or the far field (-2) and has a normal. Five state variables per element
// (density, momentum x y z, density energy). An iteration keeps a copy `old` of
// the state, computes a step factor per element from the element alone and
// runs three Runge-Kutta stages j = 0..2, each `flux` (an element reads its own
// state and its neighbours') and `time_step` (state = old + step_factor /
// (4 - j) * flux, per element). The reference runs each of these as a sweep
// over all elements with a wait after it (:470-482): 1 + 5 (2 + 3 * 2) = 41.
//
// Blocks and tasks. Elements are cut into nblocks blocks of `block`
// consecutive elements (the last may be short). Stage s = 3 it + j, S = 3
// iterations stages. One task per (stage, block), stage-major, blocks
// ascending. There are two state buffers: task (s, b) reads buffer s & 1, its
// own elements and their neighbours, and writes its own elements of buffer
// (s + 1) & 1. Buffer 0 starts as the upload and the answer is in buffer S & 1.
// flux and time_step of an element are one expression in the task, so the
// reference's `fluxes` array does not exist; its copy sweep and step-factor
// sweep are the head of the j == 0 task, which stores `old` and `step_factors`
// for its block's elements; the block's j == 1 and j == 2 tasks load them.
//
// Awaits. The VersionGraph has 2 nblocks versions, (buffer, block). Task (s, b)
// writes ((s + 1) & 1, b) and reads (s & 1, b') for every b' in N(b), where
//   N(b) = {b}  +  the blocks of the neighbours >= 0 of b's elements
//               +  the blocks that have an element naming one of b's,
// every duplicate removed, ascending. Version 0 of either buffer has no task,
// so stage 0 awaits nothing and (s, b) for s >= 1 awaits (s - 1, b'), b' in N(b).
//
// Why these awaits order everything. N is symmetric by construction: b' in N(b)
// exactly when b in N(b'). A mesh file gives no such guarantee on its own (a
// face may name an element that does not name it back), which is why the third
// term is there.
//  * Read after write: (s, b) reads the elements of buffer s & 1 that its faces
//    name; they lie in blocks of N(b), whose stage s - 1 tasks it awaits.
//  * Write after read: (s, b) overwrites ((s + 1) & 1, b) = ((s - 1) & 1, b).
//    That version was read by the stage s - 1 tasks (s - 1, b') that name an
//    element of b, that is b in N(b'), that is b' in N(b): tasks (s, b) awaits.
//    Without the third term a block named by b' but not naming b' back would
//    overwrite what (s - 1, b') may still be reading. (Readers of still older
//    stages are ordered transitively through b in N(b).)
//  * The version (s, b) reads is not overwritten under it: the next writer of
//    (s & 1, b') is (s + 1, b'), which awaits (s, b) because b in N(b').
//  * old and step_factors of block b are written by (3 it, b), read by
//    (3 it + 1, b) and (3 it + 2, b) and overwritten by (3 it + 3, b): b in N(b)
//    makes (s - 1, b) an await of (s, b), so they run as a chain.
// The awaits are the same in every stage of a launch, as hx_jacobi_plan.h needs.
//
// Counts. tasks = S nblocks; awaits = (S - 1) sum |N(b)| (0 when S = 0); the
// waiters of task (s, b), s < S - 1, are the (s + 1, b') with b in N(b'), which
// by symmetry number |N(b)|: the longest waiter list is max |N(b)| when S >= 2,
// else 0.
//
// Traffic model (bytes_moved): the bytes the bodies ask of memory, without
// credit for a cache or for two lanes sharing a line. Per element and stage:
// its state read (40) and written (40), its four neighbour indices (16) and
// normals (96), 40 per face whose neighbour is >= 0; at j == 0 its area (8) and
// old and step factor stored (48); at j == 1, 2 old and step factor loaded (48):
//   per iteration  3 (192 nelr + 40 F) + 152 nelr,  F = faces with a neighbour.
// Device layouts pad (cfd.hip); the model does not count the padding.
//
// Arena (arena_bytes): areas, neighbours, normals, two state buffers, old and
// step_factors, each on a 256-byte line; state and old as five arrays of
// cfd_pitch(nelr) doubles (cfd.hip's default layout).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "hx_vgraph.h"

namespace hx {

constexpr int kCfdBlockLength = 8;  // block_length (:30; the Makefile passes the same)
constexpr int kCfdNnb = 4, kCfdNdim = 3, kCfdNvar = 5, kCfdRk = 3;
constexpr int kCfdForms = 2;  // HCLIB_HIP_CFD_DAG, HCLIB_HIP_CFD_PHASES
constexpr int kCfdMinBlock = 8, kCfdMaxBlock = 1024;
// What block = 0 resolves to. Kernel ms at block 64 / 256 / 1024, 5 iterations
// (profiles/r24/cfd.json, one MI355X, one process): 97,032
// elements, dag 0.376 / 0.236 / 0.460, phases 0.191 / 0.160 / 0.295; 194,040
// elements, dag 0.650 / 0.356 / 0.489, phases 0.311 / 0.250 / 0.317
constexpr int kCfdDefaultBlock = 256;
constexpr uint64_t kCfdMaxTasks = 1ull << 26;  // as the other run_dag_group clients
constexpr int kCfdStride = 8;  // doubles per element of the padded array-of-structures device layout

// nelr of the reference's reader (:420)
inline int64_t cfd_nelr(int64_t nel) {
    return kCfdBlockLength * (nel / kCfdBlockLength + std::min<int64_t>(1, nel % kCfdBlockLength));
}

// The far field, exactly as :383-408 (mach 1.2, angle of attack 0)
struct CfdFarField {
    double variable[kCfdNvar];
    double momentum_x[3], momentum_y[3], momentum_z[3], density_energy[3];  // ff_flux_contribution_*
};
inline void cfd_far_field(CfdFarField &ff) {
    const double gamma = 1.4;
    const double angle_of_attack = double(3.1415926535897931 / 180.0) * double(0.0);
    ff.variable[0] = double(1.4);
    double ff_pressure = double(1.0);
    double ff_speed_of_sound = sqrt(gamma * ff_pressure / ff.variable[0]);
    double ff_speed = double(1.2) * ff_speed_of_sound;
    double vel[3];
    vel[0] = ff_speed * double(cos((double)angle_of_attack));
    vel[1] = ff_speed * double(sin((double)angle_of_attack));
    vel[2] = 0.0;
    ff.variable[1] = ff.variable[0] * vel[0];
    ff.variable[2] = ff.variable[0] * vel[1];
    ff.variable[3] = ff.variable[0] * vel[2];
    ff.variable[4] = ff.variable[0] * (double(0.5) * (ff_speed * ff_speed)) + (ff_pressure / double(gamma - 1.0));
    const double *mom = ff.variable + 1;
    // compute_flux_contribution (:136-154)
    ff.momentum_x[0] = vel[0] * mom[0] + ff_pressure;
    ff.momentum_x[1] = vel[0] * mom[1];
    ff.momentum_x[2] = vel[0] * mom[2];
    ff.momentum_y[0] = ff.momentum_x[1];
    ff.momentum_y[1] = vel[1] * mom[1] + ff_pressure;
    ff.momentum_y[2] = vel[1] * mom[2];
    ff.momentum_z[0] = ff.momentum_x[2];
    ff.momentum_z[1] = ff.momentum_y[2];
    ff.momentum_z[2] = vel[2] * mom[2] + ff_pressure;
    const double de_p = ff.variable[4] + ff_pressure;
    ff.density_energy[0] = vel[0] * de_p;
    ff.density_energy[1] = vel[1] * de_p;
    ff.density_energy[2] = vel[2] * de_p;
}

struct CfdPlan {
    int nel = 0, nelr = 0, block = 0, iterations = 0, form = 0, nblocks = 0;
    uint64_t stages = 0, tasks = 0, awaits = 0, max_waiters = 0, arena_bytes = 0, bytes_moved = 0;
    uint64_t faces = 0;                // faces whose neighbour is >= 0, over all nelr elements
    std::vector<uint32_t> noff, nids;  // N(b) as CSR, ascending within a block
};

inline size_t cfd_up256(size_t b) { return (b + 255) & ~(size_t)255; }
// doubles per variable of the array-per-variable device layout: whole 256-byte lines
inline size_t cfd_pitch(size_t nelr) { return (nelr + 31) & ~(size_t)31; }

// The blocks' neighbourhoods N(b). `symmetric` = false leaves out the third
// term (the blocks naming b): the control of tests/cpp/cfd_plan.cpp, never a
// launch's graph.
inline void cfd_neighbourhoods(int nelr, const int *neighbours, int block, bool symmetric, std::vector<uint32_t> &noff,
                               std::vector<uint32_t> &nids) {
    const uint32_t nb = (uint32_t)((nelr + block - 1) / block);
    std::vector<uint64_t> pairs;
    pairs.reserve((size_t)nb + (size_t)nelr * kCfdNnb);
    for (uint32_t b = 0; b < nb; ++b) pairs.push_back((uint64_t)b << 32 | b);
    for (int i = 0; i < nelr; ++i) {
        const uint64_t b = (uint64_t)(i / block);
        for (int j = 0; j < kCfdNnb; ++j) {
            const int k = neighbours[(size_t)i * kCfdNnb + j];
            if (k < 0) continue;
            const uint64_t o = (uint64_t)(k / block);
            if (o == b) continue;
            pairs.push_back(b << 32 | o);
            if (symmetric) pairs.push_back(o << 32 | b);
        }
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    noff.assign(nb + 1, 0);
    nids.resize(pairs.size());
    for (size_t k = 0; k < pairs.size(); ++k) {
        ++noff[(size_t)(pairs[k] >> 32) + 1];
        nids[k] = (uint32_t)pairs[k];
    }
    for (uint32_t b = 0; b < nb; ++b) noff[b + 1] += noff[b];
}

// Checks the arguments (block = 0 is replaced by its default) and fills the
// plan with the neighbourhoods and the exact counts. 0, or -1 with `err`.
inline int cfd_plan(int nel, const int *neighbours, int iterations, int &block, int form, CfdPlan &p, std::string &err) {
    auto fail = [&](const std::string &m) {
        err = m;
        return -1;
    };
    if (nel < 1) return fail("nel must be at least 1 (nel " + std::to_string(nel) + ")");
    // (the reference indexes normals with the int (i * 4 + j) * 3)
    if (nel > (INT32_MAX - 7) / (kCfdNnb * kCfdNdim))
        return fail("nel " + std::to_string(nel) + " is above what the reference's int indices reach");
    if (!neighbours) return fail("the arrays must not be NULL");
    if (iterations < 0) return fail("iterations must not be negative (iterations " + std::to_string(iterations) + ")");
    if (form < 0 || form >= kCfdForms) return fail("unknown form " + std::to_string(form));
    if (block == 0) block = kCfdDefaultBlock;
    if (block < kCfdMinBlock || block > kCfdMaxBlock || block % kCfdBlockLength)
        return fail("block " + std::to_string(block) + " is not a multiple of 8 in [8, 1024]");
    const int nelr = (int)cfd_nelr(nel);
    uint64_t faces = 0;
    for (int i = 0; i < nelr; ++i)
        for (int j = 0; j < kCfdNnb; ++j) {
            const int k = neighbours[(size_t)i * kCfdNnb + j];
            if (k >= nelr)
                return fail("element " + std::to_string(i) + " face " + std::to_string(j) + " names element " +
                            std::to_string(k) + " of " + std::to_string(nelr));
            faces += k >= 0;
        }
    p = CfdPlan();
    p.nel = nel, p.nelr = nelr, p.block = block, p.iterations = iterations, p.form = form;
    p.nblocks = (nelr + block - 1) / block;
    p.faces = faces;
    p.stages = (uint64_t)kCfdRk * (uint64_t)iterations;
    p.tasks = p.stages * (uint64_t)p.nblocks;
    if (p.tasks >= kCfdMaxTasks) return fail(std::to_string(p.tasks) + " tasks (at most 2^26): use a larger block");
    cfd_neighbourhoods(nelr, neighbours, block, true, p.noff, p.nids);
    uint64_t longest = 0;
    for (int b = 0; b < p.nblocks; ++b) longest = std::max<uint64_t>(longest, p.noff[b + 1] - p.noff[b]);
    p.awaits = p.stages ? (p.stages - 1) * (uint64_t)p.nids.size() : 0;
    if (p.awaits >= (1ull << 32)) return fail(std::to_string(p.awaits) + " awaits (at most 2^32): use a larger block");
    p.max_waiters = p.stages >= 2 ? longest : 0;
    const size_t n = (size_t)nelr;
    p.arena_bytes = cfd_up256(n * 8) + cfd_up256(n * kCfdNnb * 4) + cfd_up256(n * kCfdNnb * kCfdNdim * 8) +
                    3 * (kCfdNvar * cfd_pitch(n) * 8) + cfd_up256(n * 8);
    p.bytes_moved = (uint64_t)iterations * (3 * (192 * (uint64_t)n + 40 * faces) + 152 * (uint64_t)n);
    return 0;
}

// The task graph: payload {s, b, j, 0}, awaits as the header comment says.
inline void cfd_graph(const CfdPlan &p, VersionGraph &g) {
    const size_t nb = (size_t)p.nblocks;
    g = VersionGraph(2 * nb);
    g.reserve(p.tasks, nb ? (p.nids.size() + nb - 1) / nb : 0);
    std::vector<size_t> reads;
    for (uint64_t s = 0; s < p.stages; ++s) {
        const size_t rd = (s & 1) * nb, wr = ((s + 1) & 1) * nb;
        for (size_t b = 0; b < nb; ++b) {
            reads.clear();
            for (uint32_t k = p.noff[b]; k < p.noff[b + 1]; ++k) reads.push_back(rd + p.nids[k]);
            g.task((uint32_t)s, (uint32_t)b, (uint32_t)(s % kCfdRk), 0u, wr + b, reads.data(), reads.size());
        }
    }
}

}  // namespace hx
