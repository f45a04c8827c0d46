// hx_client.h — what the clients of the device dataflow runtimes share:
// run_dag_group clients (cholesky.hip, sparselu.hip) the version graph, the
// one-promise Kind and the launch; run_dyn_worker clients (sort.hip,
// strassen.hip, health.hip) the per-class counters, the timed Kind and the
// launch.
#pragma once

#include <string.h>

#include "hx_module.h"
#include "hx_vgraph.h"
#include "../../include/hclib_hip/hx_dag.h"
#include "../../include/hclib_hip/hx_dyn.h"

namespace hx {

// ------------------------------------------------------- run_dag_group clients
// A group Kind of a VersionGraph: one promise per task, the block version it
// makes, with the task's id and datum 0 (run_dag_group's split put).
template <class C>
struct OnePromiseKind {
    using Ctx = C;
    static constexpr int kPutN = 1;
    __device__ static void promises(const Ctx &, uint32_t t, uint32_t (&p)[1]) { p[0] = t; }
    __device__ static void datums(const Ctx &, uint32_t, unsigned long long (&d)[1]) { d[0] = 0ull; }
};

// Runs the graph on `kern` (workgroups of `threads`, no dynamic LDS):
// `launch(grid, view)` launches it on the module stream. The order carries
// three conditions:
//  1. The caller has queued uploads from host memory it owns, so no path
//     returns before the stream is synchronised: hclib_hip_dag_end does it,
//     and where begin fails, nothing was opened and it is done here.
//  2. The workgroups of a group launch wait for each other's puts, so the
//     kernel is launched only if check_resident finds them all resident.
//  3. hclib_hip_dag_end closes the launch begin opened, so it runs whether or
//     not the kernel was launched; the residency code is returned before its
//     code ("0 of n tasks ran" would hide why).
template <class Launch>
int launch_dag_group(const VersionGraph &g, int wgs_per_cu, const void *kern, int threads, const char *who,
                     hclib_hip_dag_stats_t *st, Launch launch) {
    hclib_hip_dag_launch_t L;
    int rc = hclib_hip_dag_begin(g.ntasks(), g.ntasks(), 4, g.payload.data(), g.off.data(), g.ids.data(), nullptr,
                                 nullptr, wgs_per_cu, 0, &L);
    if (rc) {
        (void)hipStreamSynchronize(mod().stream);
        return rc;
    }
    rc = check_resident(kern, L.grid, threads, 0, who);
    if (rc == HCLIB_HIP_OK) launch(L.grid, *(const DagView *)L.view);
    const int rc_end = hclib_hip_dag_end(who, nullptr, nullptr, st);
    return rc ? rc : rc_end;
}

// ------------------------------------------------------ run_dyn_worker clients
// Per-task-class counters: a 256-byte line per class at the head of the
// client's arena, [0] tasks, [1] ticks of the 100 MHz clock spent in them.
// one task of class `which` that took `ticks`, check-out included
template <class C>
__device__ __forceinline__ void class_count(const C &c, int which, unsigned long long ticks) {
    if (lane_id() == 0) {
        add_agent(&c.counts[which * 32], 1ull);
        add_agent(&c.counts[which * 32 + 1], ticks);
    }
}

// A dyn Kind K whose K::body(c, w, pay, which) names the class of the task it
// ran (or leaves -1: not counted); Ctx has the counter lines as `counts`.
template <class K, class C>
struct TimedKind {
    using Ctx = C;
    __device__ static void run(const Ctx &c, DynWave &w, uint32_t, const uint32_t *pay) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        int which = -1;
        K::body(c, w, pay, which);
        if (which >= 0) class_count(c, which, __builtin_amdgcn_s_memrealtime() - t0);
    }
};

// the host's copy: the last launch's counts and ticks, by class
template <int KINDS>
struct ClassCounters {
    static constexpr size_t kBytes = (size_t)KINDS * 256;
    unsigned long long tasks[KINDS] = {}, ticks[KINDS] = {};
};

// Runs one root task on a run_dyn_worker kernel: `launch(grid, view)` launches
// it on the module stream. The counter lines at `dev_counts` are zeroed before
// and read back after, also from a launch that failed (what ran before the
// error is the diagnosis). As for launch_dag_group the caller has queued
// uploads, so every path synchronises the stream; there is no residency check:
// a dyn worker waits only for ready-list slots below the tail, which waves
// that already run fill, and one that starts late joins in.
template <int KINDS, class Launch>
int launch_dyn(uint32_t words, const uint32_t *root, uint64_t tasks, uint64_t promises, uint64_t nodes, int waves_per_cu,
               const char *who, void *dev_counts, ClassCounters<KINDS> &cnt, hclib_hip_dyn_stats_t *st,
               uint64_t finish[2], Launch launch) {
    hclib_hip_dyn_launch_t L;
    int rc = hip_check(hipMemsetAsync(dev_counts, 0, cnt.kBytes, mod().stream), "hipMemsetAsync");
    if (rc == HCLIB_HIP_OK)
        rc = hclib_hip_dyn_begin(words, root, 1, (uint32_t)tasks, (uint32_t)promises, (uint32_t)nodes, waves_per_cu, 0, &L);
    if (rc) {
        (void)hipStreamSynchronize(mod().stream);
        return rc;
    }
    launch(L.grid, *(const DynView *)L.view);
    rc = hclib_hip_dyn_end(who, st);
    hclib_hip_dyn_finish_stats(finish);
    unsigned long long h[KINDS * 32] = {};
    if (hipMemcpy(h, dev_counts, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) memset(h, 0, sizeof(h));
    for (int k = 0; k < KINDS; ++k) cnt.tasks[k] = h[k * 32], cnt.ticks[k] = h[k * 32 + 1];
    return rc;
}

}  // namespace hx
