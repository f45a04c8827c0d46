"""Bandwidth of the reducing forasync (hclib_hip_forasync_reduce) against
torch.sum on the same tensor, in one process.

    python scripts/bench_reduce.py [--log2n 28] [--steps 20] [--warmup 3] [--rounds 3]
                                   [--sweep 2:4,4:4,8:2]

Sums 2^log2n f32 (2^28 = 1 GiB, four times the Infinity Cache) with
hclib_amd.forasync_reduce into a privatised atomic, and with torch.sum as an
independent implementation of the same read-only stream. Each figure is the
mean of `steps` back-to-back launches between two device events, after
`warmup` launches; the two are timed alternately `rounds` times and the best
round of each is the headline (every round is kept in the line). Prints one
JSON line. The atomic's gather is outside the timed window (it is one
workgroup over the slots; its time is reported separately as gather_ms).
HCLIB_HIP_REDUCE_BLOCKS_PER_CU / HCLIB_HIP_REDUCE_UNROLL select the launch
shape of the library's kernel; --sweep times a list of blocks-per-CU:unroll
pairs the same way (one JSON line each, the library's default last)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sweep", default="")
    a = ap.parse_args()

    import torch

    import hclib_amd as H

    if not torch.cuda.is_available():
        sys.exit("bench_reduce: no GPU (this benchmark has no CPU path)")
    H.init(0)
    n = 1 << a.log2n
    # integers in [0, 15]: 2^28 of them sum to < 2^32 — exact in f64, and the
    # f32 results of both implementations can be compared with the exact sum
    x = torch.randint(0, 16, (n,), device="cuda", dtype=torch.int32).to(torch.float32)
    exact = x.double().sum().item()
    stream = torch.cuda.current_stream().cuda_stream
    dom = [(0, n, 1, -1)]
    atom = H.Atomic("float32", "sum", 0.0)

    def ours():
        H.forasync_reduce(atom, x.data_ptr(), dom, H.FORASYNC_MODE_RECURSIVE, stream)

    sink = torch.zeros(1, device="cuda")

    def theirs():
        torch.sum(x, dim=0, keepdim=True, out=sink)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for cfg in [c for c in a.sweep.split(",") if c]:  # the library reads the knobs at every launch
        bpc, unroll = cfg.split(":")
        os.environ["HCLIB_HIP_REDUCE_BLOCKS_PER_CU"], os.environ["HCLIB_HIP_REDUCE_UNROLL"] = bpc, unroll
        ts = [timed(ours) for _ in range(a.rounds)]
        print(json.dumps({"bench": "forasync_reduce_sweep", "blocks_per_cu": int(bpc), "unroll": int(unroll),
                          "reduce_ms_rounds": [round(t, 5) for t in ts],
                          "reduce_GBps": round(n * 4 / 1e9 / (min(ts) * 1e-3), 1)}), flush=True)
    if a.sweep:
        del os.environ["HCLIB_HIP_REDUCE_BLOCKS_PER_CU"], os.environ["HCLIB_HIP_REDUCE_UNROLL"]
    t_ours, t_torch = [], []
    for _ in range(a.rounds):
        atom.reset(stream)
        t_ours.append(timed(ours))
        t_torch.append(timed(theirs))
    # one launch from reset: the value, and the gather's own time
    atom.reset(stream)
    ours()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = torch.zeros(1, device="cuda")
    e0.record()
    atom.gather_async(out.data_ptr(), stream)
    e1.record()
    e1.synchronize()
    gather_ms = e0.elapsed_time(e1)
    value = out.item()
    theirs()
    torch_value = sink.item()
    atom.close()

    gbytes = n * 4 / 1e9
    best_ours, best_torch = min(t_ours), min(t_torch)
    print(json.dumps({
        "bench": "forasync_reduce_sum_f32", "n": n, "bytes": n * 4, "steps": a.steps, "warmup": a.warmup,
        "reduce_ms": round(best_ours, 5), "reduce_GBps": round(gbytes / (best_ours * 1e-3), 1),
        "torch_sum_ms": round(best_torch, 5), "torch_sum_GBps": round(gbytes / (best_torch * 1e-3), 1),
        "ratio_to_torch": round(best_torch / best_ours, 4),
        "reduce_ms_rounds": [round(t, 5) for t in t_ours], "torch_sum_ms_rounds": [round(t, 5) for t in t_torch],
        "gather_ms": round(gather_ms, 5),
        "value": value, "torch_value": torch_value, "exact": exact,
        "blocks_per_cu": int(os.environ.get("HCLIB_HIP_REDUCE_BLOCKS_PER_CU", "0")) or "default",
        "unroll": int(os.environ.get("HCLIB_HIP_REDUCE_UNROLL", "0")) or "default",
        "device": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
