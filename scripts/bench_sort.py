"""BOTS sort on dynamic device dataflow (hclib_hip_sort_i64) beside torch.sort
on the device, in one process.

    python scripts/bench_sort.py [--steps 5] [--warmup 1] [--out profiles/r09/sort.json]

Configurations: the reference's default (n = 32 Mi keys, its own permutation,
cutoffs 2048 / 2048) and n = 1 Mi at the same cutoffs. kernel_ms is the
library's own figure (device events around the one launch: no copies), the
mean of `steps` launches after `warmup`. torch.sort runs on the same int64
tensor on the device between two device events: the context figure (a radix
sort of the vendor's; this sort is the reference's task program, one wave per
task). Each record carries the call tree's task counts and the pool bound.
Writes one JSON document and prints it. No number here gates anything."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 20, 1 << 25])
    ap.add_argument("--out", default=os.path.join("profiles", "r09", "sort.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H

    if not torch.cuda.is_available():
        sys.exit("bench_sort: no GPU (this benchmark has no CPU path)")
    H.init(0)
    doc = {"bench": "sort", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "merge_cutoff": 2048, "sort_cutoff": 2048, "configs": []}
    for n in a.sizes:
        t0 = time.perf_counter()
        keys = H.sort_bots_input(n)
        gen_s = time.perf_counter() - t0
        for _ in range(a.warmup):
            H.sort(keys)
        ms, st, out = [], None, None
        for _ in range(a.steps):
            out, st = H.sort(keys)
            ms.append(st["kernel_ms"])
        mean = sum(ms) / len(ms)
        rec = {"n": n, "input": "bots permutation", "input_gen_s": round(gen_s, 2),
               "sorted": bool(np.array_equal(out, np.arange(n))),
               "kernel_ms": round(mean, 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
               "mkeys_per_s": round(n / (mean * 1e3), 1),
               "counts": {k: st[k] for k in ("tasks", "sort_leaf", "sort_split", "merge_leaf", "merge_split",
                                             "merge_empty", "finishes", "check_ins")},
               "us_per_task_per_wave": round(mean * 1e3 * H.num_cus() * 8 / st["tasks"], 3),
               "pool_bound": H.sort_bounds(n)}
        # where the waves' time went in the last launch: per task class the
        # summed body time (check-out included; the worker's acquire and its
        # wait for a ticket are the remainder)
        ticks, waves = H.sort_last_ticks(), H.num_cus() * int(os.environ.get("HCLIB_HIP_SORT_WAVES_PER_CU", 8))
        total = ms[-1] * 1e-3 * 1e8 * waves
        ntask = dict(st, merge_phase=st["sort_split"])
        rec["wave_time"] = {k: {"tasks": ntask[k], "mean_us": round(v / max(ntask[k], 1) / 100, 2),
                                "share": round(v / total, 4)} for k, v in ticks.items()}
        rec["wave_time"]["outside_bodies_share"] = round(1 - sum(ticks.values()) / total, 4)
        if n == max(a.sizes):
            # the same launch with fewer persistent waves per CU (8 is the default: 8 x 16 KB of LDS)
            rec["waves_per_cu"] = {}
            for wpc in (2, 4):
                os.environ["HCLIB_HIP_SORT_WAVES_PER_CU"] = str(wpc)
                H.sort(keys)
                rec["waves_per_cu"][str(wpc)] = round(min(H.sort(keys)[1]["kernel_ms"] for _ in range(2)), 4)
            del os.environ["HCLIB_HIP_SORT_WAVES_PER_CU"]
            rec["waves_per_cu"]["8"] = rec["kernel_ms_min"]
            # the leaves' other store form: plain stores and a release fence in every check-out
            os.environ["HCLIB_HIP_SORT_SC1"] = "0"
            H.sort(keys)
            rec["plain_stores_and_release_ms"] = round(min(H.sort(keys)[1]["kernel_ms"] for _ in range(3)), 4)
            del os.environ["HCLIB_HIP_SORT_SC1"]
        x = torch.from_numpy(keys).cuda()
        for _ in range(a.warmup):
            torch.sort(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            y = torch.sort(x).values
        e1.record()
        e1.synchronize()
        t_ms = e0.elapsed_time(e1) / a.steps
        rec["torch_sort"] = {"ms": round(t_ms, 4), "mkeys_per_s": round(n / (t_ms * 1e3), 1),
                             "equal_to_ours": bool(np.array_equal(y.cpu().numpy(), out))}
        doc["configs"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
