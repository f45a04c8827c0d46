// hx_vgraph.h — the version graph of a block program (cholesky.hip,
// sparselu.hip), in plain C++: no HIP, so a host program can build one.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <vector>

namespace hx {

// The tasks of a program in which every task rewrites one block and reads
// others, given in program order. Task t makes the next version of the block it
// writes and has one promise, id t, put when that version is there. It awaits,
// for each block it reads, the task that made the block's newest version, in
// the order the reads are given (a block read twice: awaited twice). Version 0
// of a block (the host's upload, a zeroed fill-in) has no task and is left out
// of the awaits: that is what lets a task's one promise carry the task's id.
// A task that updates a block in place lists it among its reads.
// The result is what hclib_hip_dag_begin takes: `payload`, 4 words per task,
// and the awaits as CSR `off` / `ids`.
struct VersionGraph {
    std::vector<uint32_t> payload, off, ids;

    explicit VersionGraph(size_t nblocks = 0) : off(1, 0), last_(nblocks, kNone) {}
    void reserve(size_t ntasks, size_t reads_per_task) {
        payload.reserve(ntasks * 4);
        off.reserve(ntasks + 1);
        ids.reserve(ntasks * reads_per_task);
    }
    uint32_t ntasks() const { return (uint32_t)(off.size() - 1); }
    void task(uint32_t kind, uint32_t a, uint32_t b, uint32_t c, size_t writes, std::initializer_list<size_t> reads) {
        task(kind, a, b, c, writes, reads.begin(), reads.size());
    }
    // the same for a read set whose size is known only at run time (hx_jacobi_plan.h)
    void task(uint32_t kind, uint32_t a, uint32_t b, uint32_t c, size_t writes, const size_t *reads, size_t nreads) {
        const uint32_t id = ntasks();
        const uint32_t pl[4] = {kind, a, b, c};
        payload.insert(payload.end(), pl, pl + 4);
        for (size_t k = 0; k < nreads; ++k) {
            const size_t r = reads[k];
            if (last_[r] != kNone) ids.push_back(last_[r]);
        }
        off.push_back((uint32_t)ids.size());
        last_[writes] = id;
    }

  private:
    static constexpr uint32_t kNone = 0xffffffffu;
    std::vector<uint32_t> last_;  // per block, the task that made its newest version (kNone: version 0)
};

}  // namespace hx
