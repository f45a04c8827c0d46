"""The tiled Cholesky on the device promise DAG (hclib_hip_cholesky) against
torch.linalg.cholesky on the device and numpy on the host, in one process.

    python scripts/bench_cholesky.py [--steps 10] [--warmup 2] [--out profiles/r08/cholesky.json]

Configurations: the reference's own (run.sh: 500 / 20, exact mode) on a
generated SPD matrix, and 4096 / 64. kernel_ms is the
library's own figure (device events around the one DAG launch: no packing, no
copies), the mean of `steps` launches after `warmup`; GFLOP/s is (n^3 / 3) /
kernel time. torch.linalg.cholesky runs on the same float64 matrix on the
device between two device events (if this torch build provides it; the record
says so if not), numpy.linalg.cholesky on the host under a wall clock. The
500 / 20 record also carries the DAG's task and release counts and the time
per hop of its critical path: 3 nt dependent tasks (potrf, trsm, syrk per
step), bodies included. The 4096 record also says whether one launch at tile
128 gave the same bits as tile 64 (exact mode is tile-independent). Writes one
JSON document and prints it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r08", "cholesky.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H

    if not torch.cuda.is_available():
        sys.exit("bench_cholesky: no GPU (this benchmark has no CPU path)")
    H.init(0)

    def spd(n):
        b = np.random.default_rng(n).standard_normal((n, n))
        return b @ b.T + n * np.eye(n)

    def ours(mat, tile, mode):
        for _ in range(a.warmup):
            H.cholesky(mat, tile, mode)
        ms, st, l = [], None, None
        for _ in range(a.steps):
            l, st = H.cholesky(mat, tile, mode)
            ms.append(st["kernel_ms"])
        return l, st, ms

    def torch_dev(mat):
        try:
            x = torch.from_numpy(mat).cuda()
            for _ in range(a.warmup):
                torch.linalg.cholesky(x)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                y = torch.linalg.cholesky(x)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.steps, y.cpu().numpy()
        except Exception as e:  # this torch build has no device float64 Cholesky
            return None, f"{type(e).__name__}: {str(e)[:200]}"

    def numpy_host(mat):
        np.linalg.cholesky(mat)
        t0 = time.perf_counter()
        for _ in range(3):
            y = np.linalg.cholesky(mat)
        return (time.perf_counter() - t0) / 3 * 1e3, y

    doc = {"bench": "cholesky", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "configs": []}
    mats = {}
    for n, tile, mode in [(500, 20, "exact"), (4096, 64, "exact")]:
        mat = mats.setdefault(n, spd(n))
        flops = n ** 3 / 3
        l, st, ms = ours(mat, tile, mode)
        mean = sum(ms) / len(ms)
        rec = {"n": n, "tile": tile, "mode": mode, "kernel_ms": round(mean, 4), "kernel_ms_min": round(min(ms), 4),
               "kernel_ms_max": round(max(ms), 4), "gflops": round(flops / (mean * 1e6), 1),
               "tasks": st["tasks"], "puts": st["puts"], "releases": st["releases"],
               "by_kind": {k: st[k] for k in ("potrf", "trsm", "syrk", "gemm")}}
        nt = n // tile
        if n == 500:
            rec["critical_path_tasks"] = 3 * nt - 2
            rec["per_hop_us"] = round(mean * 1e3 / (3 * nt - 2), 3)
        t_ms, y = torch_dev(mat)
        if t_ms is None:
            rec["torch_linalg_cholesky"] = {"available": False, "why": y}
        else:
            rec["torch_linalg_cholesky"] = {"available": True, "ms": round(t_ms, 4),
                                            "gflops": round(flops / (t_ms * 1e6), 1),
                                            "max_abs_diff_to_ours": float(np.abs(np.tril(y) - l).max())}
        h_ms, yh = numpy_host(mat)
        rec["numpy_host"] = {"ms": round(h_ms, 3), "gflops": round(flops / (h_ms * 1e6), 1),
                             "max_abs_diff_to_ours": float(np.abs(yh - l).max())}
        if n == 4096:
            # exact mode does not depend on the tile size: one launch at tile
            # 128 must give the same bits (every word of every hand-off, under load)
            l2, st2 = H.cholesky(mat, 128, mode)
            rec["bit_identical_at_tile_128"] = bool(np.array_equal(l, l2))
            rec["tile_128_kernel_ms"] = round(st2["kernel_ms"], 4)
        doc["configs"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
