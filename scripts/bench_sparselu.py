"""BOTS SparseLU on the device promise DAG (hclib_hip_sparselu) at the
reference's default size, 50 x 50 blocks of 100 x 100 floats from genmat,
beside the two floors that bound it.

    python scripts/bench_sparselu.py [--steps 10] [--warmup 2] [--out profiles/r10/sparselu.json]
                                     [--variant-lib NAME=PATH ...]

kernel_ms is the library's own figure (device events around the one DAG
launch: no packing, no copies): mean and median of `steps` launches after
`warmup`, for one and for two workgroups per CU (HCLIB_HIP_SPARSELU_WGS); the
record says which one the library takes by default. GFLOP/s counts the
reference's operations (include/hclib_hip.h). The results of the default
launch and of a launch with either workgroup count are compared bit for bit
with the numpy restatement of the reference's loops (tests/sparselu_ref.py),
outside the timing.

No time is fixed in advance; the figure stands beside two floors:
  chain floor       the same S and B on a block-tridiagonal mask, whose graph
                    is the dependent chain alone (lu0, then fwd and bdiv side
                    by side, then bmod, per step: 3 * 49 + 1 = 148 tasks deep):
                    its kernel time, and that time per hop;
  throughput floor  the bmod flops of the default size divided by the rate of
                    the bmod body alone on resident blocks
                    (hclib_hip_sparselu_bmod_rate), every CU busy.
--variant-lib runs the headline again in a fresh process on another build of
the library (python -m hclib_amd.build --variant slu_scalar: the bmod inner
step kept off the packed f32 VALU) and records it beside the default build.

Context only: torch.linalg.lu_factor on the assembled dense 5,000 x 5,000
float32 matrix in the same process. It pivots and treats the matrix as dense,
so it is a different computation; no pass or fail hangs on it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, B = 50, 100
CHAIN = 3 * (S - 1) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "sparselu.json"))
    ap.add_argument("--variant-lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--child", action="store_true", help="headline and throughput floor only, one JSON line")
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H
    from tests import sparselu_ref as R

    if not torch.cuda.is_available():
        sys.exit("bench_sparselu: no GPU (this benchmark has no CPU path)")
    H.init(0)

    def timed(mask, blocks, wgs):
        os.environ["HCLIB_HIP_SPARSELU_WGS"] = str(wgs)
        try:
            for _ in range(a.warmup):
                H.sparselu(mask, blocks, B)
            ms, out = [], None
            for _ in range(a.steps):
                out = H.sparselu(mask, blocks, B)
                ms.append(out[2]["kernel_ms"])
        finally:
            del os.environ["HCLIB_HIP_SPARSELU_WGS"]
        st = out[2]
        mean = sum(ms) / len(ms)
        flops = st["gflops"] * st["kernel_ms"] * 1e6
        return out, {"wgs_per_cu": st["wgs_per_cu"], "kernel_ms_mean": round(mean, 4),
                     "kernel_ms_median": round(statistics.median(ms), 4), "kernel_ms_min": round(min(ms), 4),
                     "kernel_ms_max": round(max(ms), 4), "gflops": round(flops / (mean * 1e6), 1)}

    mask, blocks = H.sparselu_genmat(S, B)
    plan = H.sparselu_plan(mask, graph=False)
    bmod_flops = plan["bmod"] * 2.0 * B ** 3
    head, floors, outs = {}, {}, {}
    for wgs in (1, 2):
        outs[str(wgs)], head[str(wgs)] = timed(mask, blocks, wgs)
        ms, gf = H.sparselu_bmod_rate(B, wgs, 64)
        floors[str(wgs)] = {"bmod_gflops": round(gf, 1), "throughput_floor_ms": round(bmod_flops / (gf * 1e6), 4)}
    outs["default"] = H.sparselu(mask, blocks, B)
    st = outs["default"][2]
    default_wgs = st["wgs_per_cu"]
    if a.child:
        print(json.dumps({"headline": head, "throughput": floors, "default_wgs_per_cu": default_wgs}))
        return

    doc = {"bench": "sparselu", "S": S, "B": B, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "cus": H.num_cus(),
           "blocks_in": plan["blocks_in"], "blocks_out": plan["blocks_out"],
           "by_kind": {k: plan[k] for k in ("lu0", "fwd", "bdiv", "bmod")}, "tasks": plan["tasks"],
           "puts": st["puts"], "releases": st["releases"], "critical_path_tasks": CHAIN,
           "default_wgs_per_cu": default_wgs, "headline": head, "throughput_floor": floors}

    # the chain floor: the block-tridiagonal mask of the same S and B
    tmask, tblocks = R.masked_input(R.tridiagonal_mask(S), B, 50100)
    chain = {}
    for wgs in (1, 2):
        (_, _, tst), rec = timed(tmask, tblocks, wgs)
        rec.pop("gflops")
        rec["tasks"] = tst["tasks"]
        rec["per_hop_us"] = round(rec["kernel_ms_mean"] * 1e3 / CHAIN, 3)
        chain[str(wgs)] = rec
    doc["chain_floor"] = chain
    d = str(default_wgs)
    c_ms, t_ms = chain[d]["kernel_ms_mean"], floors[d]["throughput_floor_ms"]
    doc["binding_floor"] = "chain" if c_ms >= t_ms else "throughput"
    doc["headline_over_binding_floor"] = round(head[d]["kernel_ms_mean"] / max(c_ms, t_ms), 3)

    for spec in a.variant_lib:
        name, path = spec.split("=", 1)
        env = dict(os.environ, HCLIB_AMD_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup",
                            str(a.warmup)], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"bench_sparselu: variant {name} failed:\n{r.stdout}\n{r.stderr}")
        doc.setdefault("variants", {})[name] = json.loads(r.stdout.strip().splitlines()[-1])

    # bit for bit against the restatement, once, outside the timing
    want_mask, want = R.reference_genmat(S, B)
    # (the library's default launch, and the last timed launch of either workgroup count)
    doc["bit_identical_to_restatement"] = {k: bool(np.array_equal(o[0], want_mask) and R.same_bits(o[1], want))
                                           for k, o in outs.items()}
    doc["result_is_finite"] = bool(np.isfinite(want).all())

    # context only: a pivoting dense LU of the assembled matrix (a different computation)
    try:
        dense = np.zeros((S * B, S * B), dtype=np.float32)
        q = 0
        for ii in range(S):
            for jj in range(S):
                if mask[ii, jj]:
                    dense[ii * B:(ii + 1) * B, jj * B:(jj + 1) * B] = blocks[q]
                    q += 1
        x = torch.from_numpy(dense).cuda()
        for _ in range(a.warmup):
            torch.linalg.lu_factor(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            torch.linalg.lu_factor(x)
        e1.record()
        e1.synchronize()
        doc["torch_linalg_lu_factor_dense_5000"] = {"available": True, "ms": round(e0.elapsed_time(e1) / a.steps, 4),
                                                    "note": "pivots, dense: a different computation"}
    except Exception as e:
        doc["torch_linalg_lu_factor_dense_5000"] = {"available": False, "why": f"{type(e).__name__}: {str(e)[:200]}"}

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
