"""BOTS Strassen on dynamic device dataflow (hclib_hip_strassen), in one process.

    python scripts/bench_strassen.py [--steps 5] [--warmup 1] [--sizes 32 128 512 1024 2048 4096]
                                     [--out profiles/r12/strassen.json]

Every size runs at the reference's cutoff, 64, on seeded standard-normal
inputs. kernel_ms is the library's own figure (device events around the one
launch: no copies); each row is `warmup` launches, then `steps`, reported as
mean, min and max. gflops is 2 n^3 / kernel time, the classical count, not what
Strassen executes. Each record carries the call tree's counts and, for the last
launch, where the waves' time went by task class. For n <= 1024 the result is
compared on the bits with the numpy restatement (tests/strassen_ref.py).
Also: the two store forms (write-through stores drained by the check-out;
plain stores released by a fence at the check-out), alternated in this one
process; band_rows at several settings, alone and crossed with the persistent
waves per CU (where the two defaults, which depend on the size of the tree,
come from). As context only, torch.matmul on the same float64
tensors on the device: another algorithm with another rounding, not a target.
Writes one JSON document and prints it. No number here gates anything."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _row(ms):
    return {"mean_ms": round(sum(ms) / len(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="*", default=[32, 128, 512, 1024, 2048, 4096])
    ap.add_argument("--bands", type=int, nargs="*", default=[4, 8, 16, 32, 64])
    ap.add_argument("--waves", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "strassen.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H
    from tests import strassen_ref as R

    if not torch.cuda.is_available():
        sys.exit("bench_strassen: no GPU (this benchmark has no CPU path)")
    H.init(0)

    def launches(x, y, band_rows=0, warmup=a.warmup, steps=a.steps):
        for _ in range(warmup):
            H.strassen(x, y, 0, band_rows)
        ms, out, st = [], None, None
        for _ in range(steps):
            out, st = H.strassen(x, y, 0, band_rows)
            ms.append(st["kernel_ms"])
        return ms, out, st

    doc = {"bench": "strassen", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "cutoff": 64, "configs": []}
    for n in a.sizes:
        rng = np.random.default_rng(n)
        x, y = rng.standard_normal((n, n)), rng.standard_normal((n, n))
        try:
            ms, out, st = launches(x, y)
        except H.HclibError as e:  # an arena the device cannot hold
            doc["configs"].append({"n": n, "error": str(e)})
            print(json.dumps(doc["configs"][-1]), flush=True)
            continue
        rec = {"n": n, "input": "standard_normal, seed n", "kernel": _row(ms),
               "gflops_classical_2n3": round(2.0 * n ** 3 / (sum(ms) / len(ms) * 1e6), 1),
               "counts": {k: st[k] for k in ("tasks", "splits", "base", "tiles", "pre_bands", "combine_bands",
                                             "finishes", "check_ins", "workspace_bytes")},
               "bounds": H.strassen_bounds(n), "default_band_rows": R.default_band_rows(n),
               "default_waves_per_cu": H.strassen_waves_per_cu(n)}
        rec["bits_equal_restatement"] = R.same_bits(out, R.multiply(x, y)) if n <= 1024 else "not checked (CPU time)"
        # where the waves' time went in the last launch: per task class the
        # summed body time (check-out included; the worker's acquire, its
        # payload read and its wait for a ticket are the remainder)
        ticks, waves = H.strassen_last_ticks(), H.num_cus() * H.strassen_waves_per_cu(n)
        total = ms[-1] * 1e-3 * 1e8 * waves
        ntask = {"multiply": st["base"] + st["tiles"], "pre": st["pre_bands"], "combine": st["combine_bands"],
                 "split": st["splits"], "fork": st["splits"], "post": st["splits"]}
        rec["wave_time"] = {k: {"tasks": ntask[k], "mean_us": round(v / max(ntask[k], 1) / 100, 2),
                                "share": round(v / total, 4)} for k, v in ticks.items()}
        rec["wave_time"]["outside_bodies_share"] = round(1 - sum(ticks.values()) / total, 4)
        if n >= 512:
            # the two store forms, alternated launch by launch
            forms = {"1": [], "0": []}
            for rep in range(a.steps + 1):
                for form in ("1", "0"):
                    os.environ["HCLIB_HIP_STRASSEN_SC1"] = form
                    c2, s2 = H.strassen(x, y)
                    if rep:
                        forms[form].append(s2["kernel_ms"])
                    elif not R.same_bits(c2, out):
                        rec["store_forms_differ"] = True
            del os.environ["HCLIB_HIP_STRASSEN_SC1"]
            rec["store_forms"] = {"write_through_drained": _row(forms["1"]), "plain_released": _row(forms["0"])}
            rec["band_rows"] = {}
            for br in a.bands:
                bms, c3, s3 = launches(x, y, br, 1, 3)
                rec["band_rows"][str(br)] = dict(_row(bms), tasks=s3["tasks"], same_bits=R.same_bits(c3, out))
            # persistent waves per CU x band_rows (0 = the default): where both defaults come from
            rec["waves_per_cu_x_band_rows"] = {}
            for wpc in a.waves:
                os.environ["HCLIB_HIP_STRASSEN_WAVES_PER_CU"] = str(wpc)
                rec["waves_per_cu_x_band_rows"][str(wpc)] = {
                    str(br): _row(launches(x, y, br, 1, 3)[0]) for br in [0] + a.bands}
            del os.environ["HCLIB_HIP_STRASSEN_WAVES_PER_CU"]
        tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        for _ in range(max(a.warmup, 1)):
            tz = torch.matmul(tx, ty)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            tz = torch.matmul(tx, ty)
        e1.record()
        e1.synchronize()
        t_ms = e0.elapsed_time(e1) / a.steps
        rec["torch_matmul_f64_context"] = {"ms": round(t_ms, 4), "gflops": round(2.0 * n ** 3 / (t_ms * 1e6), 1),
                                           "max_abs_diff_to_ours": float(np.abs(tz.cpu().numpy() - out).max())}
        del tx, ty, tz
        doc["configs"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
