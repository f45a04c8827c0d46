"""The UTS path table: one small tree per launch variant of
hclib_hip_uts_search (hclib_amd/csrc/uts.hip) — the four numChildren lookup
modes, the plain and the filtering / histogram kernel, the three seeding
paths, the child counts on either side of the scheduler's pieces — with the
counts of the serial oracle (oracle/uts_oracle.c) pinned here, and the
sharded configurations each tree is searched in.

tests/test_uts_host.py holds the table to the oracle (and the oracle's shard
walk to a Python restatement) without a GPU; tests/test_uts_paths_gpu.py
holds the device to the oracle, per tree and per shard.

A helper, not a test module."""
import collections
import ctypes as C
import functools

from oracle import loader as L

Row = collections.namedtuple("Row", "key args nodes leaves depth mode what")

# mode: what hclib_hip_uts_last_launch must report. rules_lds needs at most
# 64 depth rules and 4 distinct threshold tables (kUtsLdsRules, kUtsLdsThr);
# a BIN tree is `bin`; a GEO tree of one table above a depth >= 2 and leaves
# below is `geo_fixed`.
ROWS = [
    Row("lds_linear4", "-t 1 -a 0 -d 4 -b 30 -r 1", 161380, 143212, 4, "rules_lds", "4 GEO tables in LDS"),
    Row("lds_hybrid", "-t 2 -a 0 -d 8 -f 0.5 -b 8 -q 0.23 -m 4 -r 4", 17927, 13561, 54, "rules_lds",
        "GEO and BIN rules in LDS"),
    Row("lds_hybrid_fixed", "-t 2 -a 3 -d 8 -f 0.5 -b 4 -q 0.23 -m 4 -r 1", 9136, 6869, 73, "rules_lds",
        "one table, then BIN rules"),
    Row("lds_balanced120", "-t 3 -d 2 -b 120 -r 3", 14521, 14400, 2, "rules_lds",
        "BALANCED, 120 children (not capped at 100)"),
    Row("glb_expdec", "-t 1 -a 1 -d 10 -b 6 -r 1", 39074, 19833, 29, "rules_global", "non-stationary rule table"),
    Row("glb_cyclic", "-t 1 -a 2 -d 10 -b 6 -r 9", 67978, 40502, 51, "rules_global", "cyclic"),
    # (-r 40: with -r 34 every depth-1 node falls to shard 1 of 2)
    Row("glb_linear12", "-t 1 -a 0 -d 12 -b 4 -r 40", 19648, 10684, 12, "rules_global", "linear, 12 tables"),
    Row("glb_hybrid", "-t 2 -a 0 -d 12 -b 5 -r 1 -q 0.234375 -m 4", 63640, 47815, 100, "rules_global", "hybrid"),
    Row("glb_hybrid_m120", "-t 2 -a 0 -d 12 -b 5 -r 1 -q 0.004 -m 120", 9648, 8041, 10, "rules_global",
        "hybrid, m capped at 100"),
    Row("fix_b200", "-t 1 -a 3 -d 2 -b 200 -r 1", 7947, 7846, 2, "geo_fixed",
        "root capped at 100, dense threshold buckets"),
    Row("fix_b40", "-t 1 -a 3 -d 3 -b 40 -r 4", 81475, 79286, 3, "geo_fixed", "seeded, wide levels"),
    Row("lds_fixed_d1", "-t 1 -a 3 -d 1 -b 40 -r 4", 64, 63, 1, "rules_lds", "-a 3 that is not geo_fixed (geo_depth 1)"),
    Row("one_balanced", "-t 3 -d 0 -b 5 -r 3", 1, 1, 0, "rules_lds", "root with no children"),
    Row("one_bin", "-t 0 -b 0 -q 0.2 -m 4 -r 1", 1, 1, 0, "bin", "root with no children"),
    Row("one_geo", "-t 1 -a 0 -d 4 -b 30 -r 2", 1, 1, 0, "rules_lds", "root with no children"),
    Row("bin_b2_5", "-t 0 -b 2.5 -q 0.2 -m 4 -r 1", 7, 5, 2, "bin", "fractional b_0"),
    Row("bin_m1", "-t 0 -b 2000 -q 0.9 -m 1 -r 1", 19698, 2000, 73, "bin", "m = 1"),
    Row("bin_m2", "-t 0 -b 2000 -q 0.49 -m 2 -r 1", 86485, 44242, 196, "bin", "m = 2"),
    Row("bin_m3", "-t 0 -b 2000 -q 0.33 -m 3 -r 1", 154980, 103986, 396, "bin", "m = 3"),
    Row("bin_m4", "-t 0 -b 2000 -q 0.245 -m 4 -r 1", 112725, 85043, 241, "bin", "m = 4"),
    Row("bin_m6", "-t 0 -b 2000 -q 0.165 -m 6 -r 1", 278769, 232640, 386, "bin", "m = 6"),
    Row("bin_m7", "-t 0 -b 2000 -q 0.141 -m 7 -r 1", 173620, 149102, 214, "bin", "m = 7"),
    Row("bin_m9", "-t 0 -b 2000 -q 0.11 -m 9 -r 1", 249933, 222384, 215, "bin", "m = 9, more children than pieces"),
    Row("bin_m12", "-t 0 -b 2000 -q 0.082 -m 12 -r 1", 171981, 157815, 171, "bin", "m = 12"),
    Row("bin_m0", "-t 0 -b 2000 -q 0.5 -m 0 -r 1", 2001, 2000, 1, "bin", "m = 0"),
    Row("bin_m100", "-t 0 -b 500 -q 0.0098 -m 100 -r 1", 701, 698, 2, "bin", "m = 100"),
    Row("bin_m150", "-t 0 -b 2000 -q 0.005 -m 150 -r 2", 3701, 3683, 5, "bin", "m capped at 100"),
    Row("bin_b70000", "-t 0 -b 70000 -q 0.12 -m 5 -r 3", 175211, 154168, 18, "bin",
        "level 1 wider than the seeding's level buffer"),
    Row("bin_g3", "-t 0 -b 2000 -q 0.19 -m 5 -r 11 -g 3", 35161, 28528, 70, "bin", "-g 3"),
    Row("lds_linear4_g3", "-t 1 -a 0 -d 4 -b 30 -r 1 -g 3", 161380, 143212, 4, "rules_lds", "-g 3 (same tree as -g 1)"),
    Row("glb_linear12_g3", "-t 1 -a 0 -d 12 -b 4 -r 40 -g 3", 19648, 10684, 12, "rules_global", "-g 3"),
    Row("lds_balanced5", "-t 3 -d 6 -b 5 -r 3", 19531, 15625, 6, "rules_lds", "BALANCED, constant rules only"),
]
BY_KEY = {r.key: r for r in ROWS}
assert len(BY_KEY) == len(ROWS)

MAX_NODES = 300000  # no tree of the table is larger: the suite stays quick

# the trees searched in shards, per shard against the oracle's shard walk
SHARD_KEYS = ["lds_linear4", "lds_hybrid", "lds_hybrid_fixed", "lds_balanced120",
              "glb_expdec", "glb_cyclic", "glb_linear12", "glb_hybrid",
              "lds_balanced5", "fix_b40", "bin_m3", "bin_m9", "bin_g3", "bin_b70000"]

# the seeding expands at most this many levels (hx_sched.h kSeedMaxLevels):
# a BIN shard split at 23 or deeper filters in the worker loop (FEAT = 1)
SEED_MAX_LEVELS = 24
# BIN rows whose sharded searches cannot seed to the split at any depth: the
# root's children alone (70,000) pass half the seeding's 65,544-slot buffer
BIN_SEED_TOO_WIDE = {"bin_b70000"}

# whole-tree searches on 1 and 4 waves
SMALL_GRID_KEYS = ["bin_m3", "fix_b40", "glb_cyclic"]


def shard_configs(row):
    """(nshards, split): shallow splits, a split at the deepest level, one
    past the tree (every node is above it, so shard 0 counts the whole tree
    and the seeding runs into empty levels), and on BIN trees one past the
    seeding's level bound."""
    cfgs = [(2, 1), (3, 2), (8, 4), (3, row.depth), (2, row.depth + 2)]
    if row.mode == "bin":
        cfgs.append((4, SEED_MAX_LEVELS - 1))
    return cfgs


def expect_shard_launch(row, split):
    """(feat, seeded) of a sharded launch without a histogram, or None where
    the table does not pin it. Rule-table trees filter in the worker loop.
    A BIN shard seeds exactly to its split and runs the plain kernel where
    the seeding reaches (split + 1 < 24 levels) and its levels fit. The
    fixed-shape row's levels (63, 2,177 and 79,234 slots against a buffer
    of 8 x 32,768 + 65,536 on the full grid) fit at every split."""
    if row.mode in ("rules_lds", "rules_global"):
        return (1, None)
    if row.mode == "bin":
        if split + 1 < SEED_MAX_LEVELS and row.key not in BIN_SEED_TOO_WIDE:
            return (0, 1)
        return (1, 0)
    if row.mode == "geo_fixed":
        return (0, 1)
    return None


@functools.lru_cache(maxsize=None)
def params(key):
    return L.parse_uts_args(BY_KEY[key].args)


@functools.lru_cache(maxsize=None)
def serial(key):
    """((nodes, leaves, depth), per-level histogram of depth + 1 entries) —
    computed once, shared by every test that needs it."""
    row = BY_KEY[key]
    counts, hist = L.uts_serial(params(key), row.depth + 1)
    return counts, tuple(hist)


@functools.lru_cache(maxsize=None)
def serial_shard(key, shard, nshards, split):
    counts, hist = L.uts_serial_shard(params(key), shard, nshards, split, BY_KEY[key].depth + 1)
    return counts, tuple(hist)


# ---- a pure-Python restatement of the shard rule, for tiny trees only
TINY = ["-t 2 -a 3 -d 8 -f 0.5 -b 4 -q 0.23 -m 4 -r 32",  # 287 nodes, depth 11: GEO then BIN levels
        "-t 1 -a 2 -d 4 -b 3 -r 9",                       # 576 nodes, depth 21: cyclic GEO
        "-t 0 -b 500 -q 0.0098 -m 100 -r 1"]              # 701 nodes, depth 2: a wide BIN root
TINY_CONFIGS = [(2, 1), (3, 2), (4, 3), (5, 1)]  # (a split past a tree's depth leaves it all to shard 0)


def python_shard_walk(p, shard, nshards, split, levels):
    """The partition of DESIGN.md section 6 from rng_spawn and numChildren
    alone: (nodes, leaves, depth), histogram."""
    nodes = leaves = depth = 0
    hist = [0] * levels
    stack = [(L.rng_init(p.root_id), 0, p.type)]
    while stack:
        st, h, typ = stack.pop()
        if nshards > 1 and h == split and st[0] % nshards != shard:
            continue  # a foreign node: neither counted nor expanded
        nc = L.uts_num_children(p, typ, h, st)
        if nshards == 1 or h >= split or shard == 0:
            nodes += 1
            leaves += nc <= 0
            depth = max(depth, h)
            if h < levels:
                hist[h] += 1
        ctype = L.oracle().ora_uts_child_type(C.byref(p), h)
        for i in range(max(nc, 0)):
            ch = st
            for _ in range(p.compute_gran):
                ch = L.rng_spawn(st, i)
            stack.append((ch, h + 1, ctype))
    return (nodes, leaves, depth), hist
