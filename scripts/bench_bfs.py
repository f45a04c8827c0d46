"""Rodinia BFS on the work-stealing scheduler (hclib_hip_bfs), in one process.

    python scripts/bench_bfs.py [--log2n 20] [--launches 10] [--warmup 2] [--chain 20000]
                                [--out profiles/r22/bfs.json]

The graph has Rodinia's graph1MW_6 shape (tests/bfs_ref.py generate_fast: 2^20
vertices, every vertex draws 2 .. 4 partners, links go both ways, mean degree
about 6). kernel_ms is the library's own figure (device events around the one
launch, the pool reset included, no copies). Per form: `warmup` launches, then
`launches`, reported as mean, min, max and the spread (max - min) / min; edges
per second are the level form's relaxed (the degrees of the reached vertices
summed: every edge looked at once) over kernel time, for both forms, so the
async form's figure counts useful edges, not the ones it relaxes again. The
async form's relaxed over the level form's is the extra work its LIFO order
costs. Microseconds per level come from a chain (one vertex per level, so a
level is one vertex item, one edge item and one close through renew). Every
launch's cost array is checked against the numpy queue restatement. Writes one
JSON document and prints it. No number here gates anything."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _row(ms):
    return {"mean_ms": round(sum(ms) / len(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / min(ms), 4), "all_ms": [round(m, 4) for m in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chain", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join("profiles", "r22", "bfs.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H
    from tests import bfs_ref as R

    if not torch.cuda.is_available():
        sys.exit("bench_bfs: no GPU (this benchmark has no CPU path)")
    H.init(0)
    doc = {"bench": "bfs", "launches": a.launches, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "env": {k: v for k, v in os.environ.items() if k.startswith("HCLIB_HIP_")}}

    g = R.generate_fast(1 << a.log2n, 1, source=0)
    cost, sizes, relaxed = R.queue_fast(g)
    doc["graph"] = {"vertices": len(g["starting"]), "edges": len(g["edges"]), "reached": int((cost >= 0).sum()),
                    "levels": len(sizes), "frontier": sizes, "relaxed_level_form": relaxed}
    for form in ("level", "async"):
        ms, rel, stats = [], [], None
        for i in range(a.warmup + a.launches):
            r = H.bfs(g, form)
            assert np.array_equal(r["cost"], cost), form
            if i >= a.warmup:
                ms.append(r["kernel_ms"])
                rel.append(r["relaxed"])
                stats = r
        row = _row(ms)
        row["gedges_per_s"] = round(relaxed / (row["mean_ms"] * 1e-3) / 1e9, 4)
        row["relaxed_mean"] = round(sum(rel) / len(rel), 1)
        row["relaxed_over_level_form"] = round(row["relaxed_mean"] / relaxed, 4)
        row.update({k: stats[k] for k in ("levels", "reached", "items", "chunks_pushed", "chunks_stolen")})
        row["busy_frac"] = round(stats["busy_frac"], 4)
        doc[form] = row

    chain = R.graph([[v + 1] if v + 1 < a.chain else [] for v in range(a.chain)], 0)
    want = np.arange(a.chain, dtype=np.int32)
    doc["chain"] = {"vertices": a.chain}
    for form in ("level", "async"):
        ms = []
        for i in range(a.warmup + a.launches):
            r = H.bfs(chain, form)
            assert np.array_equal(r["cost"], want), form
            if i >= a.warmup:
                ms.append(r["kernel_ms"])
        row = _row(ms)
        del row["all_ms"]
        row["us_per_level"] = round(row["mean_ms"] * 1e3 / a.chain, 4)
        doc["chain"][form] = row

    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
