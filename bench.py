#!/usr/bin/env python3
"""bench.py — BASELINE.json's metric on MI355X.

    python bench.py --gpus N --steps K --warmup W

Headline (`value`): UTS nodes/sec over the whole job for the BASELINE
multi-GPU config, test/uts T3L (-t 0 -b 2000 -q 0.200014 -m 5 -r 7,
111,345,631 nodes). One step = one complete search of the tree: every rank
expands the top `split` levels identically and then searches the T3L nodes
it owns at depth `split` (hash of the node state mod N) on its own GPU with
the persistent work-stealing megakernel; per-step totals are combined with an
RCCL all-reduce (sum nodes/leaves, max depth) and checked bit-exact against
the published tree statistics every step. Scaling is STRONG (the tree is
fixed as N grows); T3L is span-bound (17,844 dependent SHA-1 levels).

A plain run does that and no more: set up, warm up, time the K steps, print
the line (`value`, `ms_per_step`, the per-rank kernel times). `--dump-outputs
DIR` also writes the counts the last timed step returned as DIR/*.npy.

    python bench.py --full [--gpus N ...]

With `--full` the same JSON line also carries, at N=1, the other BASELINE
configs measured in the same process (T1 nodes/s, forasync triad HBM GB/s
with its roofline, fib(30) tasks/s, Smith-Waterman 64K cells/s) and the
host-CPU baseline: the repo's C restatement of HClib's work-stealing runtime
(oracle/, "port") on T3L with the box's CPU share; at N>1, T(1) with the
strong-scaling efficiency and the sharded legs (`--no-extras` skips those).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

T3L = "-t 0 -b 2000 -q 0.200014 -m 5 -r 7"
T3L_GOLD = (111345631, 89076904, 17844)  # test/uts/sample_trees.sh:42-43
T1 = "-t 1 -a 3 -d 10 -b 4 -r 19"
T1_GOLD = (4130071, 3305118, 10)          # test/uts/sample_trees.sh:17-18
T1XL = "-t 1 -a 3 -d 15 -b 4 -r 29"
T1XL_GOLD = (1635119272, 1308100063, 15)  # test/uts/sample_trees.sh:50-51
T1L = "-t 1 -a 3 -d 13 -b 4 -r 29"
T1L_GOLD = (102181082, 81746377, 13)      # test/uts/sample_trees.sh:36-37
HBM_PEAK_GBS = 8000.0                      # MI355X_MICROARCH.md chip table (spec)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def uts_step(H, rank, world, split):
    r = H.uts(T3L, rank, world, split) if world > 1 else H.uts(T3L)
    return r


def wide_tree(H, rank, world, be, steps=2, split=7):
    """The same sharded search on the wide GEO tree T1XL (1.6 G nodes,
    throughput-bound, not span-bound): what UTS sharding does when the tree
    has parallelism to spare. Whole-job nodes/s, max over ranks, bit-exact."""
    from hclib_amd import dist

    H.uts(T1XL, rank, world, split) if world > 1 else H.uts(T1XL)
    dist.barrier(world, be)
    t0 = time.perf_counter()
    kms = 0.0
    for _ in range(steps):
        r = H.uts(T1XL, rank, world, split) if world > 1 else H.uts(T1XL)
        kms += r["kernel_ms"] / steps
    dist.barrier(world, be)
    el = dist.max_over_ranks(time.perf_counter() - t0, world, be)
    tot = dist.combine_counts(r["nodes"], r["leaves"], r["max_depth"], world, be)
    if tot != T1XL_GOLD:
        raise SystemExit(f"T1XL mismatch: {tot} != {T1XL_GOLD}")
    per_rank = dist.gather_floats(kms, world, be)
    nodes = dist.gather_floats(float(r["nodes"]), world, be)
    out = {"workload": f"test/uts T1XL ({T1XL}) sharded over {world} GPU(s), split depth {split}",
           "nodes_per_s": T1XL_GOLD[0] * steps / el, "ms_per_step": el * 1e3 / steps,
           "scaling": "strong", "bit_exact": True, "kernel_ms_per_rank": per_rank,
           "nodes_per_rank": [int(n) for n in nodes]}
    if world > 1:
        # the same tree searched whole by each GPU alone (outside the timed
        # region): T(1) for the efficiency T(1) / (N * T(N))
        dist.barrier(world, be)
        t1 = time.perf_counter()
        r1 = H.uts(T1XL)
        one = dist.max_over_ranks(time.perf_counter() - t1, world, be)
        out["ms_one_gpu"] = one * 1e3
        out["efficiency"] = one / (world * el / steps)
        # the same from the GPUs' own clocks: the whole tree's kernel time
        # over N x the slowest rank's (what wall-clock skew and host overhead
        # cannot blur; the partition's own balance)
        k1 = dist.max_over_ranks(r1["kernel_ms"], world, be)
        out["kernel_ms_one_gpu"] = k1
        out["projected_efficiency_kernel"] = k1 / (world * max(per_rank))
    return out


def skewed_sharing(H, rank, world, be, split=1):
    """Cross-GPU work sharing (dist.GlobalPool) on a
    partition the static hash cannot balance: T1L split at depth 1 (a handful
    of depth-1 subtrees over `world` shards). Searched once with the static
    partition only and once sharing work through the region in rank 0's HBM;
    bit-exact both ways. Any failure is reported in the line, not raised."""
    from hclib_amd import dist

    out = {"workload": f"test/uts T1L ({T1L}) sharded over {world} GPU(s), split depth {split}: "
                       "static partition vs cross-GPU work sharing"}
    pool, err = None, ""
    try:
        pool = dist.GlobalPool(rank, world, be)
    except Exception as e:  # noqa: BLE001 (reported, every rank reaches the collective below)
        err = f"setup: {e}"
    if dist.max_over_ranks(1.0 if pool is None else 0.0, world, be) != 0.0:
        out["error"] = err or "setup failed on another rank"
        try:
            H.global_attach(None)  # (local: no collective on this path)
        except Exception:  # noqa: BLE001
            pass
        return out
    for shared in (False, True):
        if shared:
            H.global_attach(pool.ptr, pool.cap, rank)
            pool.reset()
        else:
            H.global_attach(None)
            dist.barrier(world, be)
        t0 = time.perf_counter()
        r = None
        try:
            r = H.uts(T1L, rank, world, split)
        except Exception as e:  # noqa: BLE001
            err = str(e)
        el = dist.max_over_ranks(time.perf_counter() - t0, world, be)
        if dist.max_over_ranks(1.0 if r is None else 0.0, world, be) != 0.0:
            out["error"] = err or "search failed on another rank"
            break
        tot = dist.combine_counts(r["nodes"], r["leaves"], r["max_depth"], world, be)
        key = "shared" if shared else "static"
        out[key] = {"ms": el * 1e3, "bit_exact": tot == T1L_GOLD,
                    "nodes_per_rank": [int(n) for n in dist.gather_floats(float(r["nodes"]), world, be)],
                    "kernel_ms_per_rank": dist.gather_floats(r["kernel_ms"], world, be)}
    if "error" not in out:
        g = pool.read()
        out["shared"].update({"chunks_exported": g["exported"][:world], "chunks_imported": g["imported"][:world],
                              "region_memory": pool.mem_kind})
        out["speedup"] = out["static"]["ms"] / out["shared"]["ms"]
    H.global_attach(None)
    pool.close()
    return out


def measure_triad(H, reps=20, n=1 << 28, sync=None):
    """forasync triad (BASELINE config 1): 2^28 fp32, a = b + 3*c; HIP events
    on the stream the kernel is launched on; checked bit-exact. `sync` (the
    ranks' barrier) runs just before the timed launches when sharded."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(1)
    # one allocation, the three arrays staggered by 2 MiB + 4 KiB (the
    # STREAM-style array offset: HBM channels are not all hit at the same
    # offsets by the three streams; scripts/probe_triad_layout.py measured
    # 0.50 ms here vs 0.50-0.54 ms for whatever separate allocations get)
    pad = (0x201000 // 4)
    buf = torch.empty(3 * n + 2 * pad, device="cuda")
    b = buf[:n]
    c = buf[n + pad:2 * n + pad]
    a = buf[2 * n + 2 * pad:3 * n + 2 * pad]
    b.copy_(torch.rand(n, device="cuda", generator=g))
    c.copy_(torch.rand(n, device="cuda", generator=g))
    st = torch.cuda.current_stream()
    for _ in range(3):
        H.triad_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), 3.0, n, st.cuda_stream)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if sync:
        sync()
    e0.record(st)
    for _ in range(reps):
        H.triad_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), 3.0, n, st.cuda_stream)
    e1.record(st)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    # per-launch spread (one event pair per launch, same stream): the box's
    # HBM rate varies run to run, min / median say how much
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s0, s1 in evs:
        s0.record(st)
        H.triad_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), 3.0, n, st.cuda_stream)
        s1.record(st)
    torch.cuda.synchronize()
    per = sorted(s0.elapsed_time(s1) for s0, s1 in evs)
    ok = bool(torch.equal(a, torch.add(b, torch.mul(c, 3.0))))
    del a, b, c, buf
    torch.cuda.empty_cache()
    algo = 12 * n  # read b, c; write a (write-allocate not counted)
    return {"ms": ms, "gbs": algo / ms / 1e6, "bytes": algo, "bit_exact": ok,
            "launch_ms_min": per[0], "launch_ms_median": per[len(per) // 2],
            "gbs_best": algo / per[0] / 1e6, "gbs_median": algo / per[len(per) // 2] / 1e6}


def measure_atomics(H, fib_stats):
    """L2 atomic throughput of the fib megakernel (BASELINE north_star: the
    fraction of peak L2 atomic throughput). Two figures, kept apart:
    * algorithmic: one check-out per task (tasks - 1; the root's result is a
      store), the reference's check_out_finish (src/hclib-runtime.c:431-446),
      as a rate over this run's kernel time;
    * counted: the L2 atomic requests rocprofv3 counted per fib(30) launch
      (TCC_ATOMIC_sum, profiles/atomics_pmc.json from
      scripts/pmc_atomics_r05.sh) over this run's kernel time, against the
      scattered-returning peak measured here (hclib_hip_atomic_calibrate:
      every lane its own random 16-B record). Most check-outs resolve in the
      wave's LDS finish scopes (hx_finish.h LocalScopes) and never reach L2:
      `lds_checkout_share` says how many."""
    scatter, _ = H.atomic_calibrate(H.ATOMIC_SCATTER_RET64, 256)
    hot, _ = H.atomic_calibrate(H.ATOMIC_HOT_WORD, 256)
    coal, _ = H.atomic_calibrate(H.ATOMIC_COALESCED32, 256)
    ops = fib_stats["tasks"] - 1
    sec = fib_stats["kernel_ms"] * 1e-3
    out = {"kernel": "k_fib (fib(30) join check-outs)", "unit": "Mops/s",
           "algorithmic_atomics_per_launch": ops, "algorithmic_checkouts_per_s": ops / sec / 1e6,
           "peak": scatter,
           "peak_shape": "returning 64-bit add, every lane its own random 16-B record (256 MiB)",
           "hot_word_peak": hot, "coalesced32_peak": coal}
    pmc = None
    p = os.path.join(ROOT, "profiles", "atomics_pmc.json")
    if os.path.exists(p):
        try:
            pmc = json.load(open(p))
        except Exception:  # noqa: BLE001
            pmc = None
    fib = (pmc or {}).get("fib30")
    if fib:
        # the counted figure comes from an earlier rocprofv3 run (PMC counters
        # cannot be read from inside this process): it is reported under
        # `offline_counted`, with the checks that tie it to this run — the
        # same workload (check-outs per launch) and a kernel time close to
        # this run's; `achieved` / `frac` use it only when both hold
        counted = fib["counted_l2_atomics_per_launch"]
        file_ms = ((pmc.get("kernels") or {}).get("k_fib") or {}).get("avg_ns", 0.0) * 1e-6
        same_work = fib.get("algorithmic_checkouts_per_launch") == ops
        ratio = fib_stats["kernel_ms"] / file_ms if file_ms else None
        valid = same_work and ratio is not None and 0.8 <= ratio <= 1.25
        out["offline_counted"] = {
            "l2_atomics_per_launch": counted, "rate_mops_at_this_run_kernel_time": counted / sec / 1e6,
            "frac_of_peak": counted / sec / 1e6 / scatter, "file_checkouts_per_launch":
                fib.get("algorithmic_checkouts_per_launch"), "same_workload": same_work,
            "file_kernel_ms": file_ms, "this_run_over_file_kernel_ms": ratio, "valid_for_this_run": valid,
            "lds_checkout_share": fib.get("lds_checkout_share"),
            "l2_atomics_per_checkout": fib.get("l2_atomics_per_checkout"),
            "source": "profiles/atomics_pmc.json (rocprofv3 --pmc TCC_ATOMIC_sum, scripts/pmc_atomics_r05.sh)"}
        out["achieved"] = counted / sec / 1e6 if valid else None
        out["frac"] = counted / sec / 1e6 / scatter if valid else None
        out["achieved_source"] = ("offline_counted (validated: same workload, kernel time within 25 %)" if valid
                                  else "none: the offline count does not match this run")
    else:
        out.update({"achieved": None, "frac": None, "achieved_source": "missing: profiles/atomics_pmc.json"})
    return out


def load_pmc_traffic():
    """HBM bytes per triad launch from the committed rocprofv3 PMC summary
    (profiles/), corrected per MI355X_MICROARCH.md (FETCH_SIZE x2 on gfx950)."""
    p = os.path.join(ROOT, "profiles", "triad_pmc.json")
    if os.path.exists(p):
        try:
            return json.load(open(p)).get("hbm_bytes_per_launch")
        except Exception:
            return None
    return None


def load_triad_ceiling():
    """The measured HBM ceiling of the triad's 2-read / 1-write mix
    (scripts/ubench/ub_triad_ceiling.hip -> profiles/r06/triad_ceiling.json:
    13 kernel forms x 5 occupancies, register and LDS-DMA loads, nt and
    default policies). Returns the best average rate of
    any triad form, the form, and the read-only / write-only ceilings of the
    same run, or None."""
    p = os.path.join(ROOT, "profiles", "r06", "triad_ceiling.json")
    try:
        with open(p) as f:
            rows = json.load(f)["rows"]
    except (OSError, ValueError, KeyError):
        return None
    return _ceiling_of(rows, "profiles/r06/triad_ceiling.json (scripts/ubench/ub_triad_ceiling.hip, 2^28 fp32, "
                             "hipEvents over 20 launches, same allocation layout as here; another box)")


def measure_triad_ceiling_live():
    """The same ceiling measured now, on this GPU: the quick mode of
    scripts/ubench/ub_triad_ceiling.bin (built by __graft_entry__.build())
    runs the read-only, write-only and four best triad forms at 1 and 2
    workgroups per CU in a child process (about 2 s). HBM rates differ by a
    few percent between boxes of the pool, so the line's frac_of_ceiling
    compares the kernel with the ceiling of the part it ran on. None if the
    binary is absent or fails (load_triad_ceiling() is the fallback)."""
    exe = os.path.join(ROOT, "scripts", "ubench", "ub_triad_ceiling.bin")
    if not os.access(exe, os.X_OK):
        return None
    try:
        r = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=120)
    except (OSError, subprocess.SubprocessError):
        return None
    if r.returncode:
        return None
    rows = []
    for line in r.stdout.splitlines():
        try:
            rows.append(json.loads(line))
        except ValueError:
            continue
    return _ceiling_of(rows, "live: scripts/ubench/ub_triad_ceiling.bin quick on this GPU (2^28 fp32, hipEvents "
                             "over 20 launches per form, 1 and 2 WG/CU)")


def _ceiling_of(rows, source):
    rows = [r for r in rows if isinstance(r, dict) and "form" in r and "gbs_avg" in r]
    tri = [r for r in rows if r["form"].startswith("triad")]
    if not tri:
        return None
    best = max(tri, key=lambda r: r["gbs_avg"])
    rd = max((r["gbs_avg"] for r in rows if r["form"].startswith("read2")), default=None)
    wr = max((r["gbs_avg"] for r in rows if r["form"].startswith("write1")), default=None)
    return {"gbs": best["gbs_avg"], "form": f"{best['form']}, {best['wg_per_cu']} WG/CU", "read2_gbs": rd,
            "write1_gbs": wr, "forms_measured": len(tri), "source": source}


def cpu_model() -> str:
    """The host CPU's model name (/proc/cpuinfo), for the baseline's provenance."""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return None


def cpu_allotment():
    """What this process may actually run on, with the evidence: the affinity
    mask, the cgroup CPU quota (v2 cpu.max or v1 cfs_quota/period of this
    process's cpu cgroup), the cpuset, and the job's designated share
    (OMP_NUM_THREADS, which the GPU box sets to the lease's CPU share). The
    worker count the reference would use is HCLIB_WORKERS or nprocs
    (src/hclib-locality-graph.c:585-595); here the baseline uses the CPUs the
    process is allowed, i.e. min(affinity, quota), further limited to the
    designated share only if one is set, and says which bound applied."""
    aff = len(os.sched_getaffinity(0))
    quota, qsrc = None, None
    cg = {}
    for line in (_read("/proc/self/cgroup") or "").splitlines():
        parts = line.split(":", 2)
        if len(parts) == 3:
            for ctl in parts[1].split(",") or [""]:
                cg[ctl] = parts[2]
    v2 = _read(f"/sys/fs/cgroup{cg.get('', '/')}/cpu.max".replace("//", "/")) or _read("/sys/fs/cgroup/cpu.max")
    if v2:
        q, per = (v2.split() + ["100000"])[:2]
        qsrc = f"cgroup v2 cpu.max = {v2!r}"
        if q != "max":
            quota = int(q) / int(per)
    else:
        base = "/sys/fs/cgroup/cpu" + (cg.get("cpu", "/") if cg.get("cpu", "/") != "/" else "")
        q, per = _read(base + "/cpu.cfs_quota_us"), _read(base + "/cpu.cfs_period_us")
        if q is not None and per is not None:
            qsrc = f"cgroup v1 {base}/cpu.cfs_quota_us = {q}, cfs_period_us = {per}"
            if int(q) > 0:
                quota = int(q) / int(per)
    cpuset = None
    for path in ("/sys/fs/cgroup/cpuset.cpus.effective", "/sys/fs/cgroup/cpuset/cpuset.effective_cpus",
                 "/sys/fs/cgroup/cpuset/cpuset.cpus"):
        cpuset = _read(path)
        if cpuset:
            break
    allowed = aff if quota is None else max(1, min(aff, int(quota)))
    omp = os.environ.get("OMP_NUM_THREADS")
    override = os.environ.get("HCLIB_BENCH_CPU_THREADS")
    if override:
        threads, source = max(1, int(override)), "HCLIB_BENCH_CPU_THREADS"
    elif omp and 0 < int(omp) < allowed:
        threads, source = int(omp), (f"OMP_NUM_THREADS={omp}: the job's designated CPU share, below the "
                                     f"{allowed} CPUs affinity/quota would allow")
    else:
        threads, source = allowed, ("cgroup quota" if quota is not None and int(quota) < aff else "affinity mask")
    return {"affinity_cpus": aff, "cgroup_quota": quota, "cgroup_source": qsrc, "cpuset": cpuset,
            "omp_num_threads": omp, "host_cpus_visible": os.cpu_count(), "allowed_cpus": allowed,
            "threads": threads, "threads_source": source}


def cpu_t3l(threads, min_seconds, max_searches=200):
    """Back-to-back full T3L searches on the CPU port until >= min_seconds of
    search time; returns (nodes/s, searches, seconds)."""
    import ctypes as C

    from oracle import loader as L

    lib = L.cpu_runtime()
    p = L.parse_uts_args(T3L)
    total_s, searches = 0.0, 0
    while searches == 0 or (total_s < min_seconds and searches < max_searches):
        n, lv, d, sec = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        assert lib.ohc_uts(threads, C.byref(p), C.byref(n), C.byref(lv), C.byref(d), C.byref(sec)) == 0
        assert (n.value, lv.value, d.value) == T3L_GOLD, "CPU baseline miscounted"
        total_s += sec.value
        searches += 1
    return T3L_GOLD[0] * searches / total_s, searches, total_s


def cpu_baseline(allot, min_seconds=10.0):
    """Host-CPU HClib (oracle/ C restatement, "port") on T3L at the allowed
    worker count (cpu_allotment) and with one worker (nprocs and 1).
    Bounded samples: back-to-back full T3L searches until >= min_seconds of
    search time at the allowed count; one full search at 1 worker."""
    threads = allot["threads"]
    v, searches, total_s = cpu_t3l(threads, min_seconds)
    v1, s1, t1 = cpu_t3l(1, 0.0, max_searches=1)
    out = {"value": v, "unit": "nodes/s", "cores": threads, "kind": "port", "cpu_model": cpu_model(),
           "threads": threads, "one_worker_nodes_per_s": v1, "one_worker_s": t1,
           "sample": f"{searches} back-to-back full UTS T3L searches (111,345,631 nodes each) on "
                     f"oracle/hclib_cpu.c, {threads} worker threads, {total_s:.2f} s of search time; "
                     f"1 worker: {s1} search, {t1:.2f} s"}
    out.update({k: allot[k] for k in ("affinity_cpus", "cgroup_quota", "cgroup_source", "cpuset",
                                      "omp_num_threads", "host_cpus_visible", "allowed_cpus",
                                      "threads_source")})
    # provenance of the port as a baseline: the
    # reference runtime is not built here; the round-3 review built it and
    # timed it beside this port on T3L
    out["reference_cross_check"] = {
        "source": "round-3 review (VERDICT.md): reference built out of tree with its CMake, test/uts/UTS.cpp "
                  "with the survey's driver shims, T3L; both runs on the review's 8-core Xeon build container, "
                  "not on this GPU box's host",
        "host": "8-core Xeon build container (no GPU); the port-vs-reference ratio is specific to that host",
        "reference_nodes_per_s_8_workers": [22.6e6, 24.4e6], "port_nodes_per_s_8_workers": [35.5e6, 40.2e6],
        "reference_nodes_per_s_1_worker": 3.88e6, "port_nodes_per_s_1_worker": 3.9e6,
        "port_over_reference_8_workers": 1.6,
        "note": "the port is the faster CPU baseline: GPU/CPU ratios against it understate the GPU's lead "
                "over the reference runtime"}
    return out


def cpu_configs(threads, s1, s2, gpu):
    """The same CPU runtime (oracle/, "port") on the other BASELINE configs,
    so each GPU figure has its host-CPU counterpart from the same box and
    run: fib(30) async/finish, SW 64K tile DAG (promises/futures), UTS T1
    (best of 5), forasync triad on 2^26 fp32 (bounded: 768 MiB of host
    arrays). Best of 2 each unless stated."""
    import ctypes as C

    import numpy as np

    from oracle import loader as L

    lib = L.cpu_runtime()
    out = {"cores": threads, "kind": "port"}
    best = []
    for _ in range(2):
        sec = C.c_double()
        assert lib.ohc_fib(threads, 30, 0, C.byref(sec)) == 832040
        best.append(sec.value)
    out["fib30"] = {"tasks_per_s": 2692537 / min(best), "s": min(best),
                    "gpu_over_cpu": gpu["fib30_gpu"]["tasks_per_s"] / (2692537 / min(best))}
    best = []
    for _ in range(2):
        sec = C.c_double()
        sc = lib.ohc_sw(threads, s1, len(s1), s2, len(s2), 256, 256, C.byref(sec))
        assert sc == 128772, sc
        best.append(sec.value)
    cells = 65536.0 * 65536.0
    out["sw_64k"] = {"cells_per_s": cells / min(best), "s": min(best),
                     "gpu_over_cpu": gpu["sw_64k"]["cells_per_s"] / (cells / min(best))}
    # UTS T1 (BASELINE config 2): best of 5 full searches (~4.1 M nodes each)
    p = L.parse_uts_args(T1)
    best = []
    for _ in range(5):
        nn, lv, d, sec = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        assert lib.ohc_uts(threads, C.byref(p), C.byref(nn), C.byref(lv), C.byref(d), C.byref(sec)) == 0
        assert (nn.value, lv.value, d.value) == T1_GOLD, "CPU T1 miscounted"
        best.append(sec.value)
    out["uts_t1"] = {"nodes_per_s": T1_GOLD[0] / min(best), "s": min(best),
                     "gpu_over_cpu": gpu["uts_t1_1gpu"]["nodes_per_s"] / (T1_GOLD[0] / min(best))}
    n = 1 << 26
    rng = np.random.default_rng(1)
    b = rng.random(n, dtype=np.float32)
    c = rng.random(n, dtype=np.float32)
    a = np.empty(n, dtype=np.float32)
    fp = C.POINTER(C.c_float)
    best = []
    for _ in range(2):
        sec = C.c_double()
        lib.ohc_triad(threads, a.ctypes.data_as(fp), b.ctypes.data_as(fp), c.ctypes.data_as(fp),
                      C.c_float(3.0), n, -1, 0, C.byref(sec))
        best.append(sec.value)
    assert np.array_equal(a, b + np.float32(3.0) * c)
    out["forasync_triad_2p26"] = {"GB_per_s": 12 * n / min(best) / 1e9, "s": min(best),
                                  "gpu_over_cpu": gpu["forasync_triad_2p28"]["GB_per_s"] /
                                  (12 * n / min(best) / 1e9)}
    return out


def sharded_sw(H, rank, world, be, steps=2):
    """SW 64K sharded by tile columns (hclib_amd/dist.py ShardedSw): each rank
    one band, right columns passed on per block of tile rows over RCCL.
    Whole-job cells/s over the slowest rank; band upload outside the timed
    region. SW is span-bound (511 dependent tile anti-diagonals), so this
    shows the exchange path, not a speed-up."""
    from hclib_amd import dist

    s1 = H.sw_map(open(os.path.join(ROOT, "tests/golden/sw/string1-huge.txt"), "rb").read())[:65536]
    s2 = H.sw_map(open(os.path.join(ROOT, "tests/golden/sw/string2-huge.txt"), "rb").read())[:65536]
    k = int(os.environ.get("HCLIB_BENCH_SW_BLOCK_ROWS", "0")) or dist.sw_block_rows(256, 256, world)
    # The band columns move rank to rank over RCCL point-to-point (xGMI) on a
    # multi-GPU node; HCLIB_BENCH_SW_EXCHANGE=gloo stages them through host
    # memory instead (the path the shared-device rehearsal and the CPU tests
    # exercise). The RCCL path cannot run on a 1-GPU box (two RCCL ranks need
    # two devices): if it raises, the leg falls back to gloo and says why.
    xbe = os.environ.get("HCLIB_BENCH_SW_EXCHANGE", be)

    def make_job(xb, group, abort):
        return dist.ShardedSw(s1, s2, 256, 256, rank, world, xb, block_rows=k, group=group, abort=abort)

    # the ranks agree on any fallback through the rendezvous store and a gloo
    # control group (dist.sw_exchange): never one-sided, never on an RCCL
    # group an error may have aborted
    res = dist.sw_exchange(make_job, rank, world, xbe, (128772, 65536), steps=steps)
    out = {"workload": f"test/smithwaterman 64K x 64K, 256x256 tiles, {world} column bands, "
                       f"{k} tile rows per exchanged block",
           "exchange": "RCCL send/recv (xGMI)" if res["exchange"] == "nccl" else
                       "gloo send/recv staged through host memory",
           "scaling": "strong", "bound": "span"}
    if "failed" in res:
        out["failed"] = res["failed"]
        return out
    best = res["ms"]
    out.update({"cells_per_s": 65536.0 * 65536.0 / (best * 1e-3), "ms": best, "score": 128772,
                "bit_exact": True})
    if "fallback" in res:
        out["fallback"] = res["fallback"]
    return out


def dump_outputs(dirname, counts, nodes_per_rank):
    """--dump-outputs: what the last timed step returned to its caller, one
    .npy per array (float64: every count is far below 2^53, so exact). The
    search has no input data (the tree grows from T3L's published parameters),
    so two builds given the same arguments must write the same arrays.
    Scheduler statistics and timings, which differ run to run, are left out."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    # whole-job (nodes, leaves, max_depth); at N = 1 exactly H.uts(T3L)'s counts
    np.save(os.path.join(dirname, "counts.npy"), np.asarray(counts, dtype=np.float64))
    # the nodes each rank's search returned (one entry at N = 1)
    np.save(os.path.join(dirname, "nodes_per_rank.npy"), np.asarray(nodes_per_rank, dtype=np.float64))


def _free_port() -> int:
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(argv, n, cmd=None, timeout_s=None, grace_s=60.0, out=None):
    """`python bench.py --gpus N` with no launcher around it (WORLD_SIZE
    unset): start N fresh rank processes (RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* set, one GPU each), wait for all of them, re-print rank 0's JSON
    line and return the worst exit status. This process never imports torch
    or touches the GPU and never execs: the ranks are children. If a rank
    fails, the others get `grace_s` to finish (a rank that lost its peer sits
    in a collective until the group timeout) and are then killed; the whole
    job is bounded by `timeout_s` (HCLIB_BENCH_LAUNCH_TIMEOUT_S, 3600 s).
    `cmd` (tests) replaces [python, bench.py]; `out` receives the line.
    The reference's distributed UTS is launched the same way, one process per
    PE by its launcher (test/performance-regression/full-apps/uts/
    uts_hclib_shmem_opt.cpp:98-140)."""
    import signal
    import subprocess
    import threading

    out = out or sys.stdout
    if timeout_s is None:
        timeout_s = float(os.environ.get("HCLIB_BENCH_LAUNCH_TIMEOUT_S", "3600"))
    cmd = cmd or [sys.executable, "-u", os.path.abspath(__file__)]
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                    "GROUP_RANK": "0", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # rank 0's stdout is read here (its JSON line); the others' stdout
        # goes to this process's stderr, so stdout carries one line only
        procs.append(subprocess.Popen(cmd + list(argv), env=env, stdout=subprocess.PIPE if r == 0 else 2,
                                      start_new_session=True))
    line = [None]

    def read_rank0():
        for raw in procs[0].stdout:
            s = raw.decode(errors="replace").rstrip("\n")
            try:
                obj = json.loads(s)
            except ValueError:
                obj = None
            if isinstance(obj, dict) and "metric" in obj:
                line[0] = obj
            else:
                print(s, file=sys.stderr, flush=True)
    reader = threading.Thread(target=read_rank0, daemon=True)
    reader.start()

    def kill_all():
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, signal.SIGKILL)  # the rank's own session (start_new_session)
                except OSError:
                    pass
    t0 = time.monotonic()
    failed_at = None
    while any(p.poll() is None for p in procs):
        now = time.monotonic()
        if failed_at is None and any(p.poll() not in (None, 0) for p in procs):
            failed_at = now
            log(f"self_launch: rank(s) {[i for i, p in enumerate(procs) if p.poll() not in (None, 0)]} failed; "
                f"the others get {grace_s:g} s")
        if (failed_at is not None and now - failed_at > grace_s) or now - t0 > timeout_s:
            log("self_launch: killing the remaining ranks")
            kill_all()
            break
        time.sleep(0.05)
    codes = [p.wait() for p in procs]
    reader.join(5.0)
    if line[0] is not None:
        line[0]["launcher"] = f"bench.py self-launch: {n} rank processes, MASTER 127.0.0.1:{port}"
        print(json.dumps(line[0]), file=out, flush=True)
    # worst status: a signal (negative code) as 128 + signal, as a shell reports it
    worst = 0
    for c in codes:
        c = 128 - c if c < 0 else c
        worst = max(worst, c)
    if line[0] is None and worst == 0:
        worst = 1  # every rank exited 0 but rank 0 printed no line
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--split", type=int, default=1,
                    help="depth at which T3L's nodes are hashed to ranks (the levels above are replicated)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything else the line can carry: the other "
                         "BASELINE configs, the rooflines, the atomics figures, the host-CPU baselines and, "
                         "at N > 1, T(1) and the sharded legs (a plain run reports the headline only)")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the extra legs (at N > 1 only T(1) is still measured)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float64)")
    ap.add_argument("--backend", default="nccl",
                    help="collective backend (nccl = RCCL; gloo only for rehearsals)")
    ap.add_argument("--share-device", action="store_true",
                    help="rehearsal on a 1-GPU box: every rank uses device 0 (with --backend gloo)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    # the headline needs the timed steps only; every other leg is --full's
    extras = args.full and not args.no_extras
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around us: become one (before any torch / HIP call)
        sys.exit(self_launch(sys.argv[1:], args.gpus))

    import torch  # noqa: F401  (one HIP runtime for torch + the module)

    from hclib_amd import dist

    be = args.backend
    rank, world, local = dist.init_from_env(be, share_device=args.share_device)
    if args.share_device and world > 1:
        # a rehearsal with every rank on one GPU: the ranks' persistent grids
        # must be resident together, else a work-sharing launch
        # waits for a rank whose kernel cannot start
        os.environ.setdefault("HCLIB_HIP_WAVES_PER_CU", "2")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    import hclib_amd as H

    H.init(0 if args.share_device else local)

    for _ in range(args.warmup):
        r = uts_step(H, rank, world, args.split)
    dist.barrier(world, be)
    t0 = time.perf_counter()
    kernel_ms = []
    last = None
    for _ in range(args.steps):
        r = uts_step(H, rank, world, args.split)
        kernel_ms.append(r["kernel_ms"])
        last = r
    dist.barrier(world, be)
    elapsed = dist.max_over_ranks(time.perf_counter() - t0, world, be)
    tot = dist.combine_counts(last["nodes"], last["leaves"], last["max_depth"], world, be)
    if tot != T3L_GOLD:
        raise SystemExit(f"T3L mismatch: {tot} != {T3L_GOLD}")
    value = T3L_GOLD[0] * args.steps / elapsed
    per_rank_ms = dist.gather_floats(sum(kernel_ms) / len(kernel_ms), world, be)
    per_rank_nodes = dist.gather_floats(float(last["nodes"]), world, be)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, tot, per_rank_nodes)
    t3l_one = None
    if world > 1 and args.full:
        # T(1): the whole tree on each GPU alone, outside the timed region
        dist.barrier(world, be)
        t1 = time.perf_counter()
        H.uts(T3L)
        t3l_one = dist.max_over_ranks(time.perf_counter() - t1, world, be)
    # N > 1: every optional leg runs under a wall-clock guard (dist.LegGuard):
    # a leg that stalls (a rank lost in a collective, a kernel that never
    # returns) is reported as failed in the line, the remaining legs are
    # skipped on every rank, and the line still prints within the bound
    legs = dist.LegGuard(world, float(os.environ.get("HCLIB_BENCH_LEG_TIMEOUT_S", "120")),
                         device=(0 if args.share_device else local) if be == "nccl" or args.share_device else None) \
        if world > 1 and args.full else None
    guarded = (lambda name, fn: legs.run(name, fn)) if legs else (lambda name, fn: fn())
    wide = guarded("wide_tree", lambda: wide_tree(H, rank, world, be)) if extras else None
    shard_tri = None
    if world > 1 and extras:
        # the 2^28 triad block-sharded over the ranks (no
        # exchange); whole-job GB/s over the slowest rank's launch time
        def sharded_triad():
            n_local = (1 << 28) // world
            tr = measure_triad(H, n=n_local, sync=lambda: dist.barrier(world, be))
            ms = dist.max_over_ranks(tr["ms"], world, be)
            ok = dist.max_over_ranks(0.0 if tr["bit_exact"] else 1.0, world, be) == 0.0
            return {"workload": f"hclib_forasync 1-D triad, 2^28 fp32 block-sharded over {world} GPU(s)",
                    "GB_per_s": 12 * n_local * world / ms / 1e6, "ms": ms, "scaling": "strong",
                    "bit_exact": ok}
        shard_tri = guarded("forasync_sharded", sharded_triad)
    shard_sw = None
    if world > 1 and extras:
        shard_sw = guarded("sw_sharded", lambda: sharded_sw(H, rank, world, be))
    skewed = None
    if world > 1 and extras and os.environ.get("HCLIB_BENCH_SHARE_WORK", "1") != "0":
        skewed = guarded("uts_work_sharing", lambda: skewed_sharing(H, rank, world, be))
    # a stall anywhere (this rank's guard, or another rank's flag in the
    # store) ends every rank the same way: no orderly shutdown (a leg's thread
    # may still sit in a collective) and a non-zero exit status, so torchrun
    # and the driver see the run as failed; rank 0 prints its line first
    stalled = bool(legs and (legs.stalled or legs.peer_stalled()))
    if rank != 0:
        if stalled:
            os._exit(3)
        dist.shutdown(world)
        return

    out = {
        "metric": "UTS nodes/sec (tasks/sec) at 1/2/4/8 MI355X vs host-CPU HClib; forasync HBM GB/s",
        "value": value,
        "unit": "nodes/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed * 1e3 / args.steps,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "u32",
        "data": "synthetic (UTS trees are generated from their published parameters; no dataset)",
        "config": {
            "workload": (f"test/uts T3L ({T3L}) sharded over {world} GPUs, split depth {args.split}" if world > 1
                         else f"test/uts T3L ({T3L}) searched whole on 1 GPU (no split)"),
            "nodes": T3L_GOLD[0],
            "bit_exact": True,
            "uts_kernel_ms_rank0": sum(kernel_ms) / len(kernel_ms),
            "parallelism": f"shard{world} (hash-partitioned frontier, RCCL all-reduce of counts)",
            "bound": "span: 17,844 dependent SHA-1 levels; no partition can shorten the critical path, "
                     "so strong-scaling efficiency on T3L tends to 1/N (DESIGN.md §6)",
        },
        "collectives": dist.describe(world, be),
        "kernel_ms_per_rank": per_rank_ms,
        "nodes_per_rank": [int(n) for n in per_rank_nodes],
    }
    if t3l_one is not None:
        out["ms_one_gpu"] = t3l_one * 1e3
        out["efficiency"] = t3l_one / (world * elapsed / args.steps)
    if stalled:
        out["legs_stalled"] = True
    if wide:
        out["wide_tree"] = wide
    if shard_tri:
        out["forasync_sharded"] = shard_tri
    if shard_sw:
        out["sw_sharded"] = shard_sw
    if skewed:
        out["uts_work_sharing"] = skewed
    if world == 1 and extras:
        tri = measure_triad(H)
        traffic = load_pmc_traffic()
        out["roofline"] = {
            "bound": "hbm",
            "kernel": "k_triad_f32 (hclib_forasync 1-D triad, BASELINE config 1)",
            "achieved": tri["gbs"],
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": tri["gbs"] / HBM_PEAK_GBS,
            "traffic": traffic,
            "algorithmic_bytes_per_launch": tri["bytes"],
            "avg_launch_ms": tri["ms"],
            "launch_ms_min": tri["launch_ms_min"],
            "launch_ms_median": tri["launch_ms_median"],
            "frac_best_launch": tri["gbs_best"] / HBM_PEAK_GBS,
            "frac_median_launch": tri["gbs_median"] / HBM_PEAK_GBS,
            "bit_exact": tri["bit_exact"],
        }
        ceil = measure_triad_ceiling_live() or load_triad_ceiling()
        if ceil:
            # what the 2R + 1W mix reaches at best on this part (no kernel
            # form measured faster), beside the 8 TB/s spec peak
            out["roofline"].update({"ceiling_measured": ceil["gbs"], "frac_of_ceiling": tri["gbs"] / ceil["gbs"],
                                    "ceiling_form": ceil["form"], "ceiling_read_only": ceil["read2_gbs"],
                                    "ceiling_write_only": ceil["write1_gbs"], "ceiling_source": ceil["source"]})
        # UTS kernel bound: span (critical path of dependent SHA-1s)
        uts_ms = out["config"]["uts_kernel_ms_rank0"]
        out["uts_span"] = {
            "bound": "span", "levels": T3L_GOLD[2],
            "ns_per_level": uts_ms * 1e6 / T3L_GOLD[2],
        }
        if wide:
            # the wide tree's kernel against its VALU ceiling: one rng_spawn
            # SHA-1 per node is the unavoidable work, and the chip's rate of
            # that exact instruction stream (measured here, every lane
            # chaining spawns back to back) is the peak
            cal = [(H.sha1_calibrate(ch, wpc, 2000)[0], ch, wpc) for ch, wpc in ((1, 12), (2, 12), (1, 16))]
            peak, ch, wpc = max(cal)
            ach = 1635119272 / (wide["kernel_ms_per_rank"][0] * 1e-3)
            # the same ceiling priced from the per-instruction issue costs
            # measured on this part (profiles/r04/ub_valu2.log, 4 waves per
            # SIMD): the compiled SHA-1's mix (uts_sha1.h: 221 alignbit, 142
            # add3 at 4.27 SIMD-cycles; 133 bitop3 at 2.64; 58 xor, 21 add at
            # 2.42) = ~2,092 SIMD-cycles per wave-SHA-1 = 64 SHA-1 per SIMD
            # per 2,092 cycles over every SIMD at the clock
            simd_cycles = 221 * 4.27 + 142 * 4.27 + 133 * 2.64 + 58 * 2.42 + 21 * 2.42
            issue_peak = 256 * 4 * 64 / simd_cycles * 2.4e9
            out["roofline_uts"] = {
                "bound": "valu", "kernel": "k_uts_search (UTS T1XL, throughput-bound wide tree)",
                "achieved": ach, "peak": peak, "unit": "nodes/s", "frac": ach / peak,
                "peak_issue_model": issue_peak, "frac_issue_model": ach / issue_peak,
                "issue_model": "uts_sha1.h's 575 VALU at the measured per-instruction issue costs "
                               "(ub_valu2.log): %.0f SIMD-cycles per wave-SHA-1, 1,024 SIMDs, 2.4 GHz" % simd_cycles,
                "peak_source": f"hclib_hip_sha1_calibrate: the rng_spawn SHA-1 of uts_sha1.h back to back, "
                               f"best of {[(round(c[0] / 1e9, 1), c[1], c[2]) for c in cal]} "
                               f"(G SHA-1/s, chains per lane, waves per CU)",
            }
        t1 = min((H.uts(T1) for _ in range(3)), key=lambda r: r["kernel_ms"])
        assert (t1["nodes"], t1["leaves"], t1["max_depth"]) == T1_GOLD
        # one untimed warm-up launch each (first-launch allocation and clocks),
        # then the launch reported, as every other config here
        H.fib(30)
        fv, fst = H.fib(30)
        assert fv == 832040
        s1 = H.sw_map(open(os.path.join(ROOT, "tests/golden/sw/string1-huge.txt"), "rb").read())[:65536]
        s2 = H.sw_map(open(os.path.join(ROOT, "tests/golden/sw/string2-huge.txt"), "rb").read())[:65536]
        H.sw(s1, s2, 256, 256)
        score, swst = H.sw(s1, s2, 256, 256)
        assert score == 128772
        # the same DAG as the reference writes it (3 futures / 3 puts per
        # tile) on the generic device promise machinery
        os.environ["HCLIB_HIP_SW_SCHED"] = "dag"
        H.sw(s1, s2, 256, 256)
        dscore, dagst = H.sw(s1, s2, 256, 256)
        del os.environ["HCLIB_HIP_SW_SCHED"]
        assert dscore == 128772
        t1_rate = T1_GOLD[0] / (t1["kernel_ms"] * 1e-3)
        out["configs"] = {
            # roofline_frac: T1 against the same SHA-1 issue ceiling as
            # roofline_uts (a 4.1 M-node tree: its launch ramp and drain show
            # here)
            "uts_t1_1gpu": {"nodes_per_s": t1_rate, "kernel_ms": t1["kernel_ms"],
                            "roofline_frac": t1_rate / out["roofline_uts"]["peak"] if "roofline_uts" in out else None},
            "forasync_triad_2p28": {"GB_per_s": tri["gbs"], "ms": tri["ms"]},
            "fib30_gpu": {"tasks_per_s": fst["tasks"] / (fst["kernel_ms"] * 1e-3),
                          "tasks": fst["tasks"], "kernel_ms": fst["kernel_ms"]},
            "sw_64k": {"cells_per_s": swst["cells_per_s"], "kernel_ms": swst["kernel_ms"],
                       "score": score},
            "sw_64k_promise_dag": {"cells_per_s": dagst["cells_per_s"], "kernel_ms": dagst["kernel_ms"],
                                   "tile_tasks_per_s": 65536 / (dagst["kernel_ms"] * 1e-3),
                                   "score": dscore},
        }
        out["atomics"] = measure_atomics(H, fst)
        allot = cpu_allotment()
        out["cpu_baseline"] = cpu_baseline(allot)
        out["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
        out["gpu_over_one_cpu_worker"] = value / out["cpu_baseline"]["one_worker_nodes_per_s"]
        out["cpu_configs"] = cpu_configs(allot["threads"], s1, s2, out["configs"])
    print(json.dumps(out), flush=True)
    if stalled:
        os._exit(3)
    dist.shutdown(world)


if __name__ == "__main__":
    main()
