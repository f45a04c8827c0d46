"""BOTS fft on dynamic device dataflow (hclib_hip_fft), in one process.

    python scripts/bench_fft.py [--steps 5] [--warmup 1] [--logs 13 17 21 25] [--cross-log 21 ...]
                                [--ceiling-tbs 6.26] [--out profiles/r19/fft.json]

Every size is a power of two on seeded standard-normal inputs with the
library's own twiddle table. kernel_ms is the library's own figure (device
events around the one launch: no copies); each row is `warmup` launches, then
`steps`, reported as mean, min and max. The yardstick is a traffic floor:
every pass reads and writes each (re, im) pair once, 32 n bytes, and
`bytes_moved` counts the passes of the graph (hclib_hip_fft_bounds); it is
divided by the kernel time and by the 2-read / 1-write ceiling `bench.py
--full` measured on the same box (--ceiling-tbs; profiles/r06 has 6.26 to
6.51 TB/s). Each record carries the graph's counts and, for the last launch,
where the waves' time went by task class. Sizes up to 2^21 are compared on the
bits with the numpy restatement (tests/fft_ref.py); larger ones are bounded
against numpy.fft.fft, and the record says which was done. At --cross-log the
defaults are crossed: cutoff x band x persistent waves per CU. As context only,
torch.fft.fft on the same complex128 tensor on the device: another algorithm
with another rounding, not a target. Writes one JSON document and prints it.
No number here gates anything."""
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
    ap.add_argument("--logs", type=int, nargs="*", default=[13, 17, 21, 25])
    ap.add_argument("--cross-log", type=int, nargs="*", default=[21])
    ap.add_argument("--cutoffs", type=int, nargs="*", default=[512, 2048, 8192])
    ap.add_argument("--bands", type=int, nargs="*", default=[64, 256, 1024])
    ap.add_argument("--waves", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--ceiling-tbs", type=float, default=6.26)
    ap.add_argument("--oracle-max-log", type=int, default=21)
    ap.add_argument("--out", default=os.path.join("profiles", "r19", "fft.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H
    from tests import fft_ref as R

    if not torch.cuda.is_available():
        sys.exit("bench_fft: no GPU (this benchmark has no CPU path)")
    H.init(0)

    def launches(x, w, cutoff=0, band=0, warmup=a.warmup, steps=a.steps):
        for _ in range(warmup):
            H.fft(x, w, cutoff, band)
        ms, out, st = [], None, None
        for _ in range(steps):
            out, st = H.fft(x, w, cutoff, band)
            ms.append(st["kernel_ms"])
        return ms, out, st

    def fraction(bytes_moved, ms):
        return round(bytes_moved / (ms * 1e-3) / (a.ceiling_tbs * 1e12), 4)

    doc = {"bench": "fft", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "ceiling_tbs_2r1w": a.ceiling_tbs, "configs": []}
    for lg in a.logs:
        n = 1 << lg
        rng = np.random.default_rng(lg)
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        w = H.fft_twiddles(n)
        ms, out, st = launches(x, w)
        mean = sum(ms) / len(ms)
        rec = {"n": n, "log2n": lg, "input": "standard_normal, seed log2 n", "factors": st["factors"],
               "cutoff": st["cutoff"], "band": st["band"], "kernel": _row(ms),
               "bytes_moved": st["bytes_moved"], "passes": st["bytes_moved"] // (32 * n),
               "tbytes_per_s": round(st["bytes_moved"] / (mean * 1e-3) / 1e12, 4),
               "fraction_of_ceiling": fraction(st["bytes_moved"], mean),
               "counts": {k: st[k] for k in ("tasks", "leaves", "calls", "unsh_bands", "twid_bands", "finishes",
                                             "check_ins")},
               "bounds": H.fft_bounds(n)}
        if lg <= a.oracle_max_log:
            rec["check"] = "bits equal the restatement: %s" % bool(np.array_equal(R.bits(out), R.bits(R.fft(x, w))))
        else:
            ref = np.fft.fft(x)
            rec["check"] = "bounded against numpy.fft.fft (the restatement's time): max |diff| / max |ref| = %.3e" % (
                float(np.abs(out - ref).max() / np.abs(ref).max()))
            del ref
        # where the waves' time went in the last launch: per task class the summed body time (check-out
        # included; the worker's acquire, its payload read and its wait for a ticket are the remainder)
        ticks = H.fft_last_ticks()
        waves = H.num_cus() * min(max(int(os.environ.get("HCLIB_HIP_FFT_WAVES_PER_CU", 4 if lg > 22 else 1)), 1), 8)
        total = ms[-1] * 1e-3 * 1e8 * waves
        ntask = {"leaf": st["leaves"], "unsh": st["unsh_bands"], "twid": st["twid_bands"], "call": st["calls"],
                 "fork": st["finishes"] // 2, "post": st["finishes"] // 2}
        rec["wave_time"] = {k: {"tasks": ntask[k], "mean_us": round(v / max(ntask[k], 1) / 100, 2),
                                "share": round(v / total, 4)} for k, v in ticks.items()}
        rec["wave_time"]["outside_bodies_share"] = round(1 - sum(ticks.values()) / total, 4)
        if lg in a.cross_log:
            # cutoff x band x persistent waves per CU: where the defaults come from
            rec["waves_x_cutoff_x_band"] = {}
            for wpc in a.waves:
                os.environ["HCLIB_HIP_FFT_WAVES_PER_CU"] = str(wpc)
                rec["waves_x_cutoff_x_band"][str(wpc)] = {
                    "%d/%d" % (cutoff, band): _row(launches(x, w, cutoff, band, 1, 3)[0])
                    for cutoff in a.cutoffs for band in a.bands}
            del os.environ["HCLIB_HIP_FFT_WAVES_PER_CU"]
        tx = torch.from_numpy(x).cuda()
        for _ in range(max(a.warmup, 1)):
            tz = torch.fft.fft(tx)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            tz = torch.fft.fft(tx)
        e1.record()
        e1.synchronize()
        rec["torch_fft_c128_context"] = {"ms": round(e0.elapsed_time(e1) / a.steps, 4),
                                         "note": "another algorithm and rounding, not a target",
                                         "max_abs_diff_to_ours": float(np.abs(tz.cpu().numpy() - out).max())}
        del tx, tz, x, w, out
        doc["configs"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
