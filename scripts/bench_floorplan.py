"""BOTS floorplan on the work-stealing scheduler (hclib_hip_floorplan), pruned and
exhaustive, beside fib(30) and flat N-Queens n = 12 on the same scheduler, in
one process.

    python scripts/bench_floorplan.py [--steps 5] [--warmup 1] [--out profiles/r16/floorplan.json]

Rows: each fixture named by --fixtures (default: mid) with pruning on and off.
Per row: the mean and range of `steps` launches after `warmup`, kernel_ms (the
library's own figure: device events around the one launch), items/s by what
the device ran, busy_frac, chunks pushed and stolen, and the spread of `tasks`
over the launches (pruned: it depends on the schedule; exhaustive: one value).
Every launch's min_area is checked against the fixture's expect.json. fib(30)
and flat N-Queens n = 12 from the same process are the context figures. Writes
one JSON document and prints it. No number here gates anything."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(vals, digits=4):
    return {"mean": round(sum(vals) / len(vals), digits), "min": round(min(vals), digits),
            "max": round(max(vals), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fixtures", nargs="*", default=["mid"])
    ap.add_argument("--out", default=os.path.join("profiles", "r16", "floorplan.json"))
    a = ap.parse_args()

    import torch

    import hclib_amd as H

    if not torch.cuda.is_available():
        sys.exit("bench_floorplan: no GPU (this benchmark has no CPU path)")
    H.init(0)
    gold = os.path.join(ROOT, "tests", "golden", "floorplan")
    doc = {"bench": "floorplan", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "workers": H.num_cus() * int(os.environ.get("HCLIB_HIP_WAVES_PER_CU", 3)), "bound_read": "per item",
           "configs": []}

    for name in a.fixtures:
        cells, _ = H.floorplan_read_input(os.path.join(gold, name + ".input"))
        with open(os.path.join(gold, name + ".expect.json")) as f:
            exp = json.load(f)
        for prune in (True, False):
            for _ in range(a.warmup):
                H.floorplan(cells, prune=prune)
            rs = [H.floorplan(cells, prune=prune) for _ in range(a.steps)]
            ms = [x["kernel_ms"] for x in rs]
            rec = {"fixture": name, "prune": prune, "cells": len(cells),
                   "correct": all(x["min_area"] == exp["opt"] for x in rs), "min_area": rs[-1]["min_area"],
                   "tasks_U": exp["U"]["tasks"], "tasks_L": exp["L"]["tasks"],
                   "tasks": _stats([x["tasks"] for x in rs], 1), "tasks_each": [x["tasks"] for x in rs],
                   "kernel_ms": _stats(ms),
                   "mitems_per_s": round(sum(x["items"] / (x["kernel_ms"] * 1e3) for x in rs) / len(rs), 3),
                   "busy_frac": _stats([x["busy_frac"] for x in rs], 3),
                   "improvements": _stats([x["improvements"] for x in rs], 1),
                   "chunks_pushed": _stats([x["chunks_pushed"] for x in rs], 1),
                   "chunks_stolen": _stats([x["chunks_stolen"] for x in rs], 1)}
            if not rec["correct"]:
                sys.exit("bench_floorplan: %s min_area %s, expected %d" % (name, [x["min_area"] for x in rs], exp["opt"]))
            doc["configs"].append(rec)
            print(json.dumps(rec), flush=True)

    # context: fib(30) and flat N-Queens n = 12 on the same scheduler in the same process
    for _ in range(a.warmup):
        H.fib(30)
    fs = [H.fib(30) for _ in range(a.steps)]
    fms = [s["kernel_ms"] for _, s in fs]
    doc["fib30"] = {"value": fs[-1][0], "tasks": fs[-1][1]["tasks"], "kernel_ms": _stats(fms),
                    "mtasks_per_s": round(fs[-1][1]["tasks"] / (sum(fms) / len(fms) * 1e3), 1),
                    "busy_frac": _stats([s["busy_frac"] for _, s in fs], 3)}
    for _ in range(a.warmup):
        H.nqueens(12, "flat")
    qs = [H.nqueens(12, "flat") for _ in range(a.steps)]
    qms = [q["kernel_ms"] for q in qs]
    doc["nqueens12_flat"] = {"solutions": qs[-1]["solutions"], "items": qs[-1]["items"], "kernel_ms": _stats(qms),
                             "mitems_per_s": round(qs[-1]["items"] / (sum(qms) / len(qms) * 1e3), 1),
                             "busy_frac": _stats([q["busy_frac"] for q in qs], 3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
