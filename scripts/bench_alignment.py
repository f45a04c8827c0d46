"""BOTS alignment on dynamic device dataflow (hclib_hip_alignment) on a seeded
set shaped like the BOTS large input: 100 protein-like sequences, lengths
drawn around a few hundred, in a few families so that alignments are long.

    python scripts/bench_alignment.py [--steps 10] [--warmup 2] [--out profiles/r18/alignment.json]
                                      [--write-aa set.aa]

Reports the median kernel_ms of `steps` launches (at least 10) after `warmup`
at the default cutoff, DP cells (n * m summed over the pairs) per second,
tasks, and the last launch's wave time by task class (last_ticks, 100 MHz
ticks). Two yardsticks from the same process: the same set with the cutoff
above every area (one task per pair: what spawning buys), and the lone-wave
sweep rate: the set's two longest sequences as a one-pair input, cutoff above
every area, so one wave runs the pair alone; times the resident waves it is
the ceiling the all-pairs run is reported against. The scores of every launch
must be equal (any cutoff). --write-aa writes the set as a Pearson file, for
timing the reference's serial program on it on a CPU. The set is not
committed. No number here gates anything."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AA = "ACDEFGHIKLMNPQRSTVWY"
ABOVE = 1 << 30


def generate(nseqs=100, seed=2026, families=5):
    """nseqs sequences as strings: `families` random bases of 250..700 residues, each member a copy with 25 % of
    its places substituted, dropped or doubled and cut to a length drawn from 0.5 .. 1.0 of the base's."""
    rng = random.Random(seed)
    bases = ["".join(rng.choice(AA) for _ in range(rng.randint(250, 700))) for _ in range(families)]
    out = []
    for k in range(nseqs):
        base = bases[k % families]
        s = []
        for c in base:
            r = rng.random()
            if r < 0.15:
                s.append(rng.choice(AA))
            elif r < 0.20:
                continue
            elif r < 0.25:
                s += [c, rng.choice(AA)]
            else:
                s.append(c)
        n = int(len(base) * rng.uniform(0.5, 1.0))
        start = rng.randint(0, max(0, len(s) - n))
        out.append("".join(s[start:start + n]))
    return out


def write_aa(path, seqs):
    with open(path, "w") as f:
        f.write("Number of sequences is %d\n" % len(seqs))
        for k, s in enumerate(seqs):
            f.write(">seq%d\n" % k)
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nseqs", type=int, default=100)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "alignment.json"))
    ap.add_argument("--write-aa", default="")
    a = ap.parse_args()
    seqs = generate(a.nseqs, a.seed)
    if a.write_aa:
        write_aa(a.write_aa, seqs)
        print("wrote", a.write_aa, len(seqs), "sequences,", sum(len(s) for s in seqs), "residues")
        return

    import torch

    import hclib_amd as H

    if not torch.cuda.is_available():
        sys.exit("bench_alignment: no GPU (this benchmark has no CPU path)")
    H.init(0)
    steps = max(a.steps, 10)
    matrix = H.alignment_read_matrix(os.path.join(ROOT, "tests", "golden", "alignment", "gon250.matrix"))
    codes = [[H.ALIGNMENT_CODES.index(c) for c in s] for s in seqs]
    wpc = int(os.environ.get("HCLIB_HIP_ALIGNMENT_WAVES_PER_CU", 4))
    waves = H.num_cus() * wpc
    doc = {"bench": "alignment", "steps": steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "nseqs": len(seqs), "seed": a.seed, "lengths": {"min": min(map(len, seqs)), "max": max(map(len, seqs)),
                                                            "mean": round(sum(map(len, seqs)) / len(seqs), 1)},
           "resident_waves": waves, "configs": []}
    ref = None
    for label, cutoff in (("default", 0), ("one task per pair", ABOVE)):
        for _ in range(a.warmup):
            H.alignment(codes, matrix, cutoff)
        rs = [H.alignment(codes, matrix, cutoff) for _ in range(steps)]
        ref = ref or rs[0]["scores"]
        if any(r["scores"] != ref for r in rs):
            sys.exit("bench_alignment: scores differ between launches")
        ms = sorted(r["kernel_ms"] for r in rs)
        med = statistics.median(ms)
        ticks = H.alignment_last_ticks()
        rec = {"cutoff": rs[0]["cutoff"], "label": label, "pairs": rs[0]["pairs"], "tasks": rs[0]["tasks"],
               "cells": rs[0]["cells"], "diff_calls": rs[0]["diff_calls"], "spawn_tasks": rs[0]["spawn_tasks"],
               "kernel_ms": {"median": round(med, 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)},
               "gcells_per_s": round(rs[0]["cells"] / (med * 1e6), 4), "last_ticks": ticks,
               "wave_ms_by_class": {k: round(v / 1e5, 3) for k, v in ticks.items()},
               "busy_frac": round(sum(ticks.values()) / 1e5 / (med * waves), 4)}
        doc["configs"].append(rec)
        print(json.dumps(rec), flush=True)
    # the lone wave: the two longest sequences, one pair, one task
    two = sorted(codes, key=len)[-2:]
    for _ in range(a.warmup):
        H.alignment(two, matrix, ABOVE)
    rs = [H.alignment(two, matrix, ABOVE) for _ in range(steps)]
    med = statistics.median(r["kernel_ms"] for r in rs)
    lone = rs[0]["cells"] / (med * 1e6)
    doc["lone_wave"] = {"lengths": [len(q) for q in two], "cells": rs[0]["cells"], "kernel_ms_median": round(med, 4),
                        "gcells_per_s": round(lone, 5), "ceiling_gcells_per_s": round(lone * waves, 3)}
    doc["fraction_of_ceiling"] = round(doc["configs"][0]["gcells_per_s"] / (lone * waves), 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
