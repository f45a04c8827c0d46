"""Rodinia SRAD on the device promise DAG (hclib_hip_srad), in one process.

    python scripts/bench_srad.py [--sides 2048 8192] [--rois 128 1024] [--iterations 2 100] [--blocks 16 32 64]
                                 [--launches 3] [--warmup 1] [--ceiling-tbs 6.26] [--max-tasks 8000000]
                                 [--budget-s 0] [--out profiles/r27/srad.json]

The image is the reference's own (hclib_hip_srad_image) at side x side; the
region of interest is 0..roi-1 squared, Rodinia's usual 128 and a second one of
1024 where the serial sum is long. kernel_ms is the library's own figure: device
events around the one launch (dag) or around all reduce and sweep kernels
(phases), no copies. Per side, ROI, iteration count, block and form: `warmup`
launches, then `launches`, reported as mean with min and max; tasks per second;
the plan's bytes_moved over time, and that as a fraction of the 2-read /
1-write triad ceiling `bench.py --full` measured on the same kind of box
(--ceiling-tbs, profiles/r06); and the dag form's mean over the phases form's at
the same block. Within one (side, ROI, iterations) every launch's image and
q0sqr are compared on their bits with the first launch's: the forms and blocks
must agree (tests/test_srad_gpu.py pins them to the reference at small sizes).
A configuration whose graph has more than --max-tasks tasks is not run, and
none is started once --budget-s seconds (0: no limit) have passed; both are
recorded as skipped. Writes one JSON document and prints it. No number here
gates anything."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _dumps(doc):
    """the document with one line per configuration"""
    cases = doc.pop("cases")
    head = json.dumps(doc, indent=1)[:-2] + ',\n "cases": [\n'
    parts = []
    for c in cases:
        configs = c.pop("configs")
        parts.append("  " + json.dumps(c)[:-1] + ', "configs": [\n' + ",\n".join("   " + json.dumps(x) for x in configs)
                     + "\n  ]}")
    return head + ",\n".join(parts) + "\n ]\n}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", nargs="+", type=int, default=[2048, 8192])
    ap.add_argument("--rois", nargs="+", type=int, default=[128, 1024])
    ap.add_argument("--iterations", nargs="+", type=int, default=[2, 100])
    ap.add_argument("--blocks", nargs="+", type=int, default=[16, 32, 64])
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--ceiling-tbs", type=float, default=6.26)
    ap.add_argument("--max-tasks", type=int, default=8000000)
    ap.add_argument("--budget-s", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join("profiles", "r27", "srad.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H

    if not torch.cuda.is_available():
        sys.exit("bench_srad: no GPU (this benchmark has no CPU path)")
    H.init(0)
    t_start = time.monotonic()
    doc = {"bench": "srad", "launches": a.launches, "warmup": a.warmup, "lambda": a.lam,
           "device": torch.cuda.get_device_name(0), "ceiling_tbs_2r1w": a.ceiling_tbs, "max_tasks": a.max_tasks,
           "budget_s": a.budget_s, "env": {k: v for k, v in os.environ.items() if k.startswith("HCLIB_HIP_")},
           "cases": []}
    for side in a.sides:
        j0 = H.srad_image(side, side)
        for roi_side in a.rois:
            roi = (0, roi_side - 1, 0, roi_side - 1)
            for niter in a.iterations:
                entry = {"side": side, "roi": list(roi), "iterations": niter, "bits_agree": True, "configs": []}
                first = None
                for block in a.blocks:
                    bnd = H.srad_bounds(side, side, roi, niter, block)
                    means = {}
                    for form in ("dag", "phases"):
                        base = {"block": block, "form": form, "tasks": bnd["tasks"], "awaits": bnd["awaits"]}
                        if form == "dag" and bnd["tasks"] > a.max_tasks:
                            entry["configs"].append(dict(base, skipped="more than --max-tasks tasks"))
                            continue
                        if a.budget_s and time.monotonic() - t_start > a.budget_s:
                            entry["configs"].append(dict(base, skipped="the time budget was spent"))
                            continue
                        ms = []
                        for i in range(a.warmup + a.launches):
                            got, st = H.srad(j0, roi, a.lam, niter, block, form)
                            if i >= a.warmup:
                                ms.append(st["kernel_ms"])
                        if first is None:
                            first = (got.view(np.uint32).copy(), st["q0sqr"].view(np.uint32).copy())
                        elif not (np.array_equal(got.view(np.uint32), first[0])
                                  and np.array_equal(st["q0sqr"].view(np.uint32), first[1])):
                            entry["bits_agree"] = False
                        mean = sum(ms) / len(ms)
                        means[form] = mean
                        row = dict(base, mean_ms=round(mean, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                                   ms_per_iteration=round(mean / niter, 4), bytes_moved=st["bytes_moved"],
                                   mtasks_per_s=round(st["tasks"] / (mean * 1e-3) / 1e6, 4),
                                   gbytes_per_s=round(st["bytes_moved"] / (mean * 1e-3) / 1e9, 2),
                                   fraction_of_ceiling=round(st["bytes_moved"] / (mean * 1e-3) / (a.ceiling_tbs * 1e12), 4),
                                   gcells_per_s=round(side * side * niter / (mean * 1e-3) / 1e9, 4))
                        entry["configs"].append(row)
                        print("#", side, roi_side, niter, json.dumps(row), flush=True)
                    if len(means) == 2:
                        entry["configs"].append({"block": block, "dag_over_phases": round(means["dag"] / means["phases"], 4)})
                doc["cases"].append(entry)
    doc["seconds"] = round(time.monotonic() - t_start, 1)

    text = _dumps(doc)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
