"""Interleaved A/B of (library, environment) configurations on one UTS tree
(development aid; the policy A/B of one build's knobs, beside ab_libs_t3l.py's
A/B of two builds):

    python scripts/ab_env_uts.py T3L 6 off=hclib_amd/lib/libhclib_amd.so,HCLIB_HIP_NARROW_SHED=0 \
        half=hclib_amd/lib/libhclib_amd.so,HCLIB_HIP_NARROW_SHED=1 ...

Each configuration runs in a process of its own (six launches: the best, all
six, and the narrow loop's shed counters and the hand-off waves' counters of
the last), ROUNDS times, the configurations interleaved."""
import json
import os
import statistics
import subprocess
import sys

tree, rounds, cfgs = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
code = r'''
import os, sys, json
sys.path.insert(0, os.getcwd())
import torch
import hclib_amd as H
sys.path.insert(0, "scripts")
from uts_probe import TREES
H.init(0)
a, n = TREES[sys.argv[1]]
ms = []
for _ in range(6):
    r = H.uts(a)
    assert r["nodes"] == n
    ms.append(round(r["kernel_ms"], 3))
c = H.last_shed_counters() if hasattr(H.lib(), "hclib_hip_last_shed_counters") else {}
cc = H.last_comm_counters() if hasattr(H.lib(), "hclib_hip_last_comm_counters") else {}
print(json.dumps({"ms": ms, "shed": c, "comm": cc}))
'''
res = {}
for rnd in range(rounds):
    for cfg in cfgs:
        name, rest = cfg.split("=", 1)
        parts = rest.split(",")
        env = dict(os.environ, HCLIB_AMD_LIB=os.path.abspath(parts[0]))
        env.update(kv.split("=", 1) for kv in parts[1:])
        out = subprocess.run([sys.executable, "-c", code, tree], env=env, capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            print(name, "FAILED rc", out.returncode, out.stderr[-2000:], flush=True)
            sys.exit(1)
        d = json.loads(out.stdout.strip().splitlines()[-1])
        res.setdefault(name, []).append(min(d["ms"]))
        print(tree, rnd, name, "best", min(d["ms"]), "all", d["ms"], "shed", d["shed"], "comm", d.get("comm", {}),
              flush=True)
for name, v in res.items():
    print(f"{tree} {name}: median of bests {statistics.median(v):.3f} min {min(v):.3f} max {max(v):.3f} ms {v}")
