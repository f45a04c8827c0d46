"""Kastors jacobi on the device promise DAG (hclib_hip_jacobi), in one process.

    python scripts/bench_jacobi.py [--steps 3] [--warmup 1] [--grids 512:4 8192:64] [--blocks 32 64]
                                   [--fuses 1 2 4 0] [--ceiling-tbs 6.26] [--out profiles/r20/jacobi.json]

Every grid is the reference's Poisson problem (hclib_hip_jacobi_rhs). kernel_ms
is the library's own figure (device events around the one launch: no copies);
each row is `warmup` launches, then `steps`, reported as mean, min and max.
Per (grid, block) the fuse depths 1, 2, 4 and the largest the LDS holds (0 on
the command line) are run in turn, and where the block leaves room for more
than one workgroup per CU, each count of workgroups. A row carries the graph's
counts, cells and bytes per second (bytes_moved of hclib_hip_jacobi_bounds: per
task the clipped region of u, the cells of f and the block), that rate as a
fraction of the 2-read / 1-write ceiling `bench.py --full` measured on the same
box (--ceiling-tbs), the microseconds per superstep, and the time relative to
fuse 1 of the same grid and block. The yardstick for fuse 1 is that fraction;
the yardstick for fuse k is fuse 1.

Every timed result is checked: on the bits against the numpy restatement
(tests/jacobi_ref.py) up to --oracle-max-cells cell-iterations, otherwise on
the bits against the first fuse-1 result of the same grid (which is itself
checked for the boundary and, over a corner window, against the restatement).
As context only, the same sweeps as two torch slice expressions per iteration
on the device. Writes one JSON document and prints it. No number here gates
anything."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _row(ms):
    return {"mean_ms": round(sum(ms) / len(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grids", nargs="*", default=["512:4", "8192:64"], help="n:niter")
    ap.add_argument("--blocks", type=int, nargs="*", default=[32, 64])
    ap.add_argument("--fuses", type=int, nargs="*", default=[1, 2, 4, 0], help="0: the largest that fits")
    ap.add_argument("--ceiling-tbs", type=float, default=6.26)
    ap.add_argument("--oracle-max-cells", type=float, default=4e7)
    ap.add_argument("--out", default=os.path.join("profiles", "r20", "jacobi.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H
    from tests import jacobi_ref as R

    if not torch.cuda.is_available():
        sys.exit("bench_jacobi: no GPU (this benchmark has no CPU path)")
    H.init(0)

    doc = {"bench": "jacobi", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "ceiling_tbs_2r1w": a.ceiling_tbs, "default_fuse": R.DEFAULT_FUSE, "configs": []}
    for grid in a.grids:
        n, niter = (int(x) for x in grid.split(":"))
        f, unew0 = H.jacobi_rhs(n, n)
        oracle = R.sweep(f, unew0, niter) if float(n) * n * niter <= a.oracle_max_cells else None
        first = None  # the first fuse-1 result of this grid
        rec = {"n": n, "niter": niter, "cells": n * n, "rows": []}
        for block in a.blocks:
            if n % block:
                continue
            base_ms = None
            for fuse in a.fuses:
                fuse = fuse or min(block, (R.MAX_REGION - block) // 2)
                if fuse > block or block + 2 * fuse > R.MAX_REGION:
                    continue
                os.environ.pop("HCLIB_HIP_JACOBI_WGS_PER_CU", None)
                _, st0 = H.jacobi(f, unew0, block=block, niter=niter, fuse=fuse)  # also the first warm-up
                for wgs in sorted({1, 2, st0["wgs_per_cu"]} & set(range(1, st0["wgs_per_cu"] + 1)), reverse=True):
                    os.environ["HCLIB_HIP_JACOBI_WGS_PER_CU"] = str(wgs)
                    for _ in range(max(a.warmup - (wgs == st0["wgs_per_cu"]), 0)):
                        H.jacobi(f, unew0, block=block, niter=niter, fuse=fuse)
                    ms, checks = [], []
                    for _ in range(a.steps):
                        out, st = H.jacobi(f, unew0, block=block, niter=niter, fuse=fuse)
                        ms.append(st["kernel_ms"])
                        if oracle is not None:
                            checks.append(bool(np.array_equal(R.bits(out), R.bits(oracle))))
                        elif first is None:
                            # no full oracle: the boundary is f, and a corner window wide enough that niter
                            # sweeps cannot reach it from outside equals the restatement of that window
                            m = min(n, 2 * niter + 32)
                            edge = all(np.array_equal(R.bits(x), R.bits(y)) for x, y in
                                       ((out[0], f[0]), (out[-1], f[-1]), (out[:, 0], f[:, 0]), (out[:, -1], f[:, -1])))
                            win = R.sweep(f[:m, :m], unew0[:m, :m], niter, 1.0 / (n - 1), 1.0 / (n - 1))
                            k = m - niter - 1  # cells the window's false boundary has not reached
                            checks.append(edge and bool(np.array_equal(R.bits(out[:k, :k]), R.bits(win[:k, :k]))))
                            first = out
                        else:
                            checks.append(bool(np.array_equal(R.bits(out), R.bits(first))))
                        del out
                    mean = sum(ms) / len(ms)
                    if fuse == 1 and wgs == st0["wgs_per_cu"]:
                        base_ms = mean
                    row = {"block": block, "fuse": fuse, "wgs_per_cu": st["wgs_per_cu"], "kernel": _row(ms),
                           "tasks": st["tasks"], "supersteps": st["supersteps"], "bytes_moved": st["bytes_moved"],
                           "gcells_per_s": round(n * n * niter / (mean * 1e6), 2),
                           "gbytes_per_s": round(st["bytes_moved"] / (mean * 1e6), 1),
                           "fraction_of_ceiling": round(st["bytes_moved"] / (mean * 1e-3) / (a.ceiling_tbs * 1e12), 4),
                           "us_per_superstep": round(mean * 1e3 / max(st["supersteps"], 1), 2),
                           "time_vs_fuse1": round(mean / base_ms, 4) if base_ms else None,
                           "check": ("bits equal the restatement" if oracle is not None else
                                     "bits equal the first fuse-1 result (whose boundary and corner window equal "
                                     "the restatement)") + ": %s" % all(checks)}
                    rec["rows"].append(row)
                    print(json.dumps(row), flush=True)
                os.environ.pop("HCLIB_HIP_JACOBI_WGS_PER_CU", None)
        # context: two slice expressions per iteration in torch
        dx = dy = 1.0 / (n - 1)
        tf, tu0 = torch.from_numpy(f).cuda(), torch.from_numpy(unew0).cuda()

        def torch_sweeps():
            u, v = tu0.clone(), torch.empty_like(tf)
            for _ in range(niter):
                v.copy_(tf)
                v[1:-1, 1:-1] = 0.25 * ((((u[:-2, 1:-1] + u[1:-1, 2:]) + u[1:-1, :-2]) + u[2:, 1:-1]) +
                                        (tf[1:-1, 1:-1] * dx) * dy)
                u, v = v, u
            return u

        torch_sweeps()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tu = torch_sweeps()
        e1.record()
        e1.synchronize()
        ref = oracle if oracle is not None else first
        rec["torch_slices_context"] = {
            "ms": round(e0.elapsed_time(e1), 4), "note": "eager kernels with temporaries, all niter iterations; not a target",
            "bits_equal_ours": bool(ref is not None and np.array_equal(R.bits(tu.cpu().numpy()), R.bits(ref)))}
        del tf, tu, first, oracle
        doc["configs"].append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
