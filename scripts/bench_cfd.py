"""Rodinia CFD on the device promise DAG (hclib_hip_cfd), in one process.

    python scripts/bench_cfd.py [--grids 311x312 440x441] [--blocks 64 256 1024] [--iterations 5]
                                [--launches 10] [--warmup 2] [--layouts 0 1] [--ceiling-tbs 6.26]
                                [--out profiles/r24/cfd.json]

The meshes are generated (tests/cfd_ref.py generate: a torus of elements with
2 % wing faces, 2 % far-field faces and 2 % one-directional jumps) at about the
sizes of Rodinia's fvcorr.domn.097K and .193K, which this tree does not hold.
kernel_ms is the library's own figure: device events around the one launch
(dag) or around all 3 x iterations stage kernels (phases), no copies. Per mesh,
layout (HCLIB_HIP_CFD_LAYOUT: 0 = 8 doubles per element, 1 = an array per
variable), form and block: `warmup` launches, then `launches`, reported as
mean, min, max and the spread (max - min) / min; tasks per second; the plan's
bytes_moved over time, and that as a fraction of the 2-read / 1-write triad
ceiling `bench.py --full` measured on the same kind of box (--ceiling-tbs);
and the dag form's mean over the phases form's at the same block. Every
launch's state is compared on its bits with the numpy restatement where that
stays finite. Writes one JSON document and prints it. No number here gates
anything."""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _row(ms):
    return {"mean_ms": round(sum(ms) / len(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / min(ms), 4)}


def _dumps(doc):
    """the document with one line per configuration"""
    meshes = doc.pop("meshes")
    head = json.dumps(doc, indent=1)[:-2] + ',\n "meshes": [\n'
    parts = []
    for m in meshes:
        configs = m.pop("configs")
        parts.append("  " + json.dumps(m)[:-1] + ', "configs": [\n' + ",\n".join("   " + json.dumps(c) for c in configs)
                     + "\n  ]}")
    return head + ",\n".join(parts) + "\n ]\n}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", nargs="+", default=["311x312", "440x441"])
    ap.add_argument("--blocks", nargs="+", type=int, default=[64, 256, 1024])
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layouts", nargs="+", type=int, default=[0, 1])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ceiling-tbs", type=float, default=6.26)
    ap.add_argument("--out", default=os.path.join("profiles", "r24", "cfd.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H
    from tests import cfd_ref as R

    if not torch.cuda.is_available():
        sys.exit("bench_cfd: no GPU (this benchmark has no CPU path)")
    H.init(0)
    doc = {"bench": "cfd", "iterations": a.iterations, "launches": a.launches, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "ceiling_tbs_2r1w": a.ceiling_tbs,
           "env": {k: v for k, v in os.environ.items() if k.startswith("HCLIB_HIP_")}, "meshes": []}
    for grid in a.grids:
        gx, gy = (int(x) for x in grid.split("x"))
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "mesh.txt")
            R.write_mesh(R.generate(gx, gy, a.seed, 0.02, 0.02, 0.02), path)
            m = H.cfd_read_input(path)
        want = R.run(m, a.iterations)
        finite = bool(np.isfinite(want).all())
        entry = {"grid": grid, "nel": m["nel"], "nelr": m["nelr"], "restatement_finite": finite, "configs": []}
        for layout in a.layouts:
            os.environ["HCLIB_HIP_CFD_LAYOUT"] = str(layout)
            for block in a.blocks:
                bnd = H.cfd_bounds(m, a.iterations, block)
                means = {}
                for form in ("dag", "phases"):
                    ms = []
                    for i in range(a.warmup + a.launches):
                        got, st = H.cfd(m, a.iterations, block, form)
                        if finite:
                            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (grid, layout, block, form)
                        if i >= a.warmup:
                            ms.append(st["kernel_ms"])
                    row = _row(ms)
                    mean = row["mean_ms"]
                    means[form] = mean
                    row.update({"layout": layout, "block": block, "form": form, "tasks": st["tasks"],
                                "awaits": bnd["awaits"], "max_waiters": bnd["max_waiters"],
                                "bytes_moved": st["bytes_moved"],
                                "mtasks_per_s": round(st["tasks"] / (mean * 1e-3) / 1e6, 4),
                                "gbytes_per_s": round(st["bytes_moved"] / (mean * 1e-3) / 1e9, 2),
                                "fraction_of_ceiling": round(st["bytes_moved"] / (mean * 1e-3) / (a.ceiling_tbs * 1e12), 4),
                                "gelement_stages_per_s": round(m["nelr"] * st["stages"] / (mean * 1e-3) / 1e9, 4)})
                    if form == "phases":
                        row["us_per_stage"] = round(mean * 1e3 / st["stages"], 3)
                    entry["configs"].append(row)
                entry["configs"].append({"layout": layout, "block": block,
                                         "dag_over_phases": round(means["dag"] / means["phases"], 4)})
        doc["meshes"].append(entry)
    os.environ.pop("HCLIB_HIP_CFD_LAYOUT", None)

    text = _dumps(doc)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
