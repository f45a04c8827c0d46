"""N-Queens on the work-stealing scheduler (hclib_hip_nqueens), both forms, beside
fib(30) on the same scheduler, in one process.

    python scripts/bench_nqueens.py [--steps 5] [--warmup 1] [--out profiles/r11/nqueens.json]

Configurations: n = 14 (the BOTS default size, app-desc.h) and n = 12
(nqueens.cpp's default); the BOTS form with every call spawning (d = n) and at
task depth 3 (BOTS_CUTOFF_DEF_VALUE), the flat form with every call spawning.
The BOTS form also runs with its scopes in HBM only (HCLIB_HIP_NQUEENS_LOCAL=0)
and, at the smaller size, with the conflicting placements as items
(HCLIB_HIP_NQUEENS_SPAWN_ALL=1, the reference's n asyncs per call). Per
configuration: the mean and range of `steps` launches after `warmup`,
kernel_ms (the library's own figure: device events around the one launch; the
host's count of the scopes is outside it), tasks/s by the reference's task
count, items/s by what the device ran, busy_frac, chunks pushed and stolen.
fib(30)'s tasks/s from the same process is the context figure. Writes one JSON
document and prints it. No number here gates anything."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(vals, digits=4):
    return {"mean": round(sum(vals) / len(vals), digits), "min": round(min(vals), digits),
            "max": round(max(vals), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="*", default=[12, 14])
    ap.add_argument("--out", default=os.path.join("profiles", "r11", "nqueens.json"))
    a = ap.parse_args()

    import torch

    import hclib_amd as H

    if not torch.cuda.is_available():
        sys.exit("bench_nqueens: no GPU (this benchmark has no CPU path)")
    H.init(0)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                           "nqueens_goldens.json")) as f:
        table = json.load(f)["solutions"]
    doc = {"bench": "nqueens", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "workers": H.num_cus() * int(os.environ.get("HCLIB_HIP_WAVES_PER_CU", 3)), "configs": []}

    def run(n, form, d, env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            for _ in range(a.warmup):
                H.nqueens(n, form, d)
            rs = [H.nqueens(n, form, d) for _ in range(a.steps)]
        finally:
            for k in env or {}:
                del os.environ[k]
        r = rs[-1]
        ms = [x["kernel_ms"] for x in rs]
        mean = sum(ms) / len(ms)
        rec = {"n": n, "form": form, "task_depth": d if d else n, "env": env or {},
               "correct": all(x["solutions"] == table[n - 1] for x in rs), "solutions": r["solutions"],
               "tasks": r["tasks"], "items": r["items"], "scopes": r["scopes"], "joins": r["joins"],
               "kernel_ms": _stats(ms), "mtasks_per_s": round(r["tasks"] / (mean * 1e3), 3),
               "mitems_per_s": round(r["items"] / (mean * 1e3), 3),
               "busy_frac": _stats([x["busy_frac"] for x in rs], 3),
               "chunks_pushed": _stats([x["chunks_pushed"] for x in rs], 1),
               "chunks_stolen": _stats([x["chunks_stolen"] for x in rs], 1)}
        doc["configs"].append(rec)
        print(json.dumps(rec), flush=True)

    for n in a.sizes:
        run(n, "bots", 0)
        run(n, "bots", 3)
        run(n, "flat", 0)
        run(n, "bots", 0, {"HCLIB_HIP_NQUEENS_LOCAL": "0"})
        if n == min(a.sizes):
            run(n, "bots", 0, {"HCLIB_HIP_NQUEENS_SPAWN_ALL": "1"})
    # context: fib(30) on the same scheduler in the same process
    for _ in range(a.warmup):
        H.fib(30)
    fs = [H.fib(30) for _ in range(a.steps)]
    fms = [s["kernel_ms"] for _, s in fs]
    doc["fib30"] = {"value": fs[-1][0], "tasks": fs[-1][1]["tasks"], "kernel_ms": _stats(fms),
                    "mtasks_per_s": round(fs[-1][1]["tasks"] / (sum(fms) / len(fms) * 1e3), 1),
                    "busy_frac": _stats([s["busy_frac"] for _, s in fs], 3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
