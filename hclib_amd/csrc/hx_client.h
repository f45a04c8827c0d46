// hx_client.h — what the clients of the device dataflow runtimes share:
// run_dag_group clients (cholesky.hip, sparselu.hip) the version graph, the
// one-promise Kind and the launch; run_dyn_worker clients (sort.hip,
// strassen.hip, health.hip) the per-class counters, the timed Kind and the
// launch; run_worker clients (fib.hip, nqueens.hip, floorplan.hip, uts.hip,
// bfs.hip) the grid and pool knobs, the unseeded SchedConfig, the launch and
// busy_frac.
#pragma once

#include <string.h>

#include <string>

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
// `datum_out`, where given, receives every promise's datum (srad.hip: a
// promise that carries a value).
template <class Launch>
int launch_dag_group(const VersionGraph &g, int wgs_per_cu, const void *kern, int threads, const char *who,
                     hclib_hip_dag_stats_t *st, Launch launch, uint64_t *datum_out = nullptr) {
    hclib_hip_dag_launch_t L;
    int rc = hclib_hip_dag_begin(g.ntasks(), g.ntasks(), 4, g.payload.data(), g.off.data(), g.ids.data(), nullptr,
                                 nullptr, wgs_per_cu, 0, &L);
    if (rc) {
        (void)hipStreamSynchronize(mod().stream);
        return rc;
    }
    rc = check_resident(kern, L.grid, threads, 0, who);
    if (rc == HCLIB_HIP_OK) launch(L.grid, *(const DagView *)L.view);
    const int rc_end = hclib_hip_dag_end(who, datum_out, nullptr, st);
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

// ---------------------------------------------------------- run_worker clients
// workers of a launch: HCLIB_HIP_GRID, else HCLIB_HIP_WAVES_PER_CU on every CU
inline int sched_grid(int default_waves_per_cu) {
    const int grid = env_int("HCLIB_HIP_GRID", 0);
    return grid > 0 ? grid : mod().num_cus * env_int("HCLIB_HIP_WAVES_PER_CU", default_waves_per_cu);
}

// the chunk deques: HCLIB_HIP_DEQUES (the client's default count) of
// HCLIB_HIP_DEQUE_CAP slots, `chunk` items of `words` u32 per slot
inline int sched_pool(int nq_default, uint32_t chunk, uint32_t words, PoolView *pool) {
    return make_pool((uint32_t)env_int("HCLIB_HIP_DEQUES", nq_default), (uint32_t)env_int("HCLIB_HIP_DEQUE_CAP", 4096),
                     chunk, words, pool);
}

// The settings of a launch that starts from one root, under the client's knob
// names HCLIB_HIP_<CLIENT>_SPILL_HI / _SPILL_LO / _HUNGER: a batch pushes at
// most 64 * 10 range items, so 256 leaves a 1,024-item ring its room; 32 / 8
// from scripts/sweep_uts.py fib30 (profiles/r01_s5/knob_sweeps.log: spill_lo
// 32 -> 1.50 ms, 2 -> 1.70 ms)
inline SchedConfig sched_config_unseeded(const char *client, int grid) {
    auto knob = [&](const char *name, int dflt) {
        return (uint32_t)env_int((std::string("HCLIB_HIP_") + client + name).c_str(), dflt);
    };
    SchedConfig cfg;
    cfg.spill_hi = knob("_SPILL_HI", 256);
    cfg.spill_lo = knob("_SPILL_LO", 32);
    cfg.spin_limit = (uint32_t)env_int("HCLIB_HIP_SPIN_LIMIT_MS", 20000);
    cfg.nwaves = (uint32_t)grid;
    cfg.stamps = 0;
    cfg.hunger = knob("_HUNGER", 8);
    cfg.carry = (uint32_t)env_int("HCLIB_HIP_CARRY", 1);
    return cfg;
}

// The end of a run_worker launch: the launch's own error (reported as
// `launch_what` failing), the closing event, the globals and exit records
// read back with the stream drained (finish_sched, which translates the
// device error word), the time between the module's two events.
inline int end_sched(const char *who, SchedGlobals *gl, float *kernel_ms, const char *launch_what = "hipGetLastError()") {
    Module &m = mod();
    HX_TRY(hip_check(hipGetLastError(), launch_what));
    HX_HIP(hipEventRecord(m.ev1, m.stream));
    const int rc = finish_sched(gl, who);
    *kernel_ms = 0;
    (void)hipEventElapsedTime(kernel_ms, m.ev0, m.ev1);
    return rc;
}

// Runs a run_worker kernel `kern` (`blocks` workgroups of `threads`, no
// dynamic LDS): `launch()` launches it on the module stream. The order
// carries three conditions:
//  1. reset_sched is the caller's (outstanding count and seeding differ) and
//     is queued before this: the opening event follows it, so kernel_ms
//     covers the pool reset as it always has.
//  2. The workers wait for each other's work until the launch's outstanding
//     count is zero, so the kernel is launched only if check_resident finds
//     every workgroup resident; a refusal returns with nothing launched.
//  3. A launched kernel is followed by finish_sched, which drains the
//     stream: *gl is complete (also after a device error, whose code is
//     returned) and the caller may read its results back with plain copies.
template <class Launch>
int launch_sched(const void *kern, int blocks, int threads, const char *who, Launch launch, SchedGlobals *gl,
                 float *kernel_ms, const char *launch_what = "hipGetLastError()") {
    Module &m = mod();
    HX_HIP(hipEventRecord(m.ev0, m.stream));
    HX_TRY(check_resident(kern, blocks, threads, 0, who));
    launch();
    return end_sched(who, gl, kernel_ms, launch_what);
}

// share of wave time spent inside batches
inline double busy_frac(const SchedGlobals &gl) {
    const double busy = (double)gl.counters[kCtrBusyCycles], idle = (double)gl.counters[kCtrIdleCycles];
    return (busy + idle) > 0 ? busy / (busy + idle) : 0.0;
}

}  // namespace hx
