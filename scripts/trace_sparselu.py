"""Where the SparseLU launch spends its chain: per-task stamps of the promise
DAG (hx_dag.h kDagTraceWords, 100 MHz device clock), by task kind.

    python -m hclib_amd.build --variant trace
    HCLIB_AMD_LIB=hclib_amd/lib/trace/libhclib_amd.so python scripts/trace_sparselu.py \
        [--out profiles/r10/sparselu_trace.txt]

Needs the library's trace build (the default build records no stamps). Runs
the default size (50 x 50 blocks of 100 x 100 from genmat) and the
block-tridiagonal mask of the same size (the dependent chain alone), each with
one and with two workgroups per CU, one warm-up launch and one traced launch,
and reports per kind: the body's time (start of the task to every wave
drained), the put's time, and the time from a task's release to its start. The
stamps cost a few stores per task; kernel_ms of a traced launch is not a
benchmark figure."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S, B = 50, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "sparselu_trace.txt"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import hclib_amd as H
    from tests import sparselu_ref as R

    if not torch.cuda.is_available():
        sys.exit("trace_sparselu: no GPU")
    H.init(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    tmp = os.path.abspath(a.out) + ".stamps"
    lines = [f"SparseLU {S} / {B}, per-task stamps by kind (us); library {os.path.basename(os.path.dirname(H.LIB_PATH))}"]
    inputs = [("tridiagonal (the chain alone)", R.masked_input(R.tridiagonal_mask(S), B, 50100)),
              ("genmat (the default size)", H.sparselu_genmat(S, B))]
    for name, (mask, blocks) in inputs:
        kinds = H.sparselu_plan(mask)["payload"][:, 0]
        for wgs in ("1", "2"):
            os.environ["HCLIB_HIP_SPARSELU_WGS"] = wgs
            H.sparselu(mask, blocks, B)
            os.environ["HCLIB_HIP_DAG_TRACE"] = tmp
            try:
                _, _, st = H.sparselu(mask, blocks, B)
            finally:
                del os.environ["HCLIB_HIP_DAG_TRACE"], os.environ["HCLIB_HIP_SPARSELU_WGS"]
            if not os.path.exists(tmp):
                sys.exit("trace_sparselu: no stamps were written: load the trace build through HCLIB_AMD_LIB")
            tr = np.fromfile(tmp, dtype=np.uint64).reshape(-1, 16).astype(np.int64)
            os.remove(tmp)
            lines.append(f"{name}, {wgs} workgroup(s) per CU: {st['tasks']} tasks, kernel {st['kernel_ms']:.3f} ms, "
                         f"first start to last put {(tr[:, 3].max() - tr[:, 1].min()) / 100.0:.1f} us")
            for kind, kname in enumerate(H.SPARSELU_KINDS):
                sel = kinds == kind
                if not sel.any():
                    continue
                body = (tr[sel, 2] - tr[sel, 1]) / 100.0
                put = (tr[sel, 3] - tr[sel, 2]) / 100.0
                rel = tr[sel, 0]
                wait = ((tr[sel, 1] - rel) / 100.0)[rel > 0]
                lines.append("  %-5s n = %5d  body mean %7.2f min %7.2f max %7.2f | put mean %5.2f | "
                             "release to start mean %6.2f | kept by its releaser %.2f" % (
                                 kname, int(sel.sum()), body.mean(), body.min(), body.max(), put.mean(),
                                 wait.mean() if len(wait) else float("nan"), tr[sel, 4].mean()))
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
