"""CPU-side checks of the UTS path table (tests/uts_ref.py): every row's
pinned counts against the serial oracle, the oracle's shard walk
(ora_uts_serial_shard) against the serial walk, against a pure-Python
restatement on tiny trees and against the golden SHA-1 state vectors (which
32-bit word picks a node's shard), the library's host mirror of numChildren
against the oracle where -m passes 100, and the conditions that keep every
sharded case from being vacuous. No GPU."""
import pytest

import hclib_amd as H
from oracle import loader as L
from tests import uts_ref as R

SHARDED = [(k, n, s) for k in R.SHARD_KEYS for n, s in R.shard_configs(R.BY_KEY[k])]


@pytest.mark.parametrize("key", [r.key for r in R.ROWS])
def test_table_counts_equal_the_serial_oracle(key):
    row = R.BY_KEY[key]
    counts, hist = R.serial(key)
    assert counts == (row.nodes, row.leaves, row.depth)
    assert sum(hist) == row.nodes and hist[0] == 1 and hist[-1] > 0
    assert row.nodes <= R.MAX_NODES


@pytest.mark.parametrize("key", [r.key for r in R.ROWS])
def test_one_shard_is_the_serial_walk(key):
    assert R.serial_shard(key, 0, 1, 0) == R.serial(key)
    # (the split is not looked at with one shard)
    assert R.serial_shard(key, 0, 1, 2) == R.serial(key)


def test_shard_walk_refuses_what_the_device_refuses():
    p, r = R.params("bin_b2_5"), L.UtsResult()
    import ctypes as C

    for shard, nshards, split in [(0, 0, 1), (-1, 2, 1), (2, 2, 1), (0, 2, 0)]:
        assert L.oracle().ora_uts_serial_shard(C.byref(p), shard, nshards, split, C.byref(r), None, 0) == -2


@pytest.mark.parametrize("key,nshards,split", SHARDED)
def test_shards_partition_the_tree(key, nshards, split):
    (nodes, leaves, depth), hist = R.serial(key)
    parts = [R.serial_shard(key, s, nshards, split) for s in range(nshards)]
    assert sum(c[0] for c, _ in parts) == nodes
    assert sum(c[1] for c, _ in parts) == leaves
    assert max(c[2] for c, _ in parts) == depth
    assert tuple(sum(col) for col in zip(*(h for _, h in parts))) == hist
    # the levels above the split belong to shard 0 alone
    top = min(split, depth + 1)
    assert parts[0][1][:top] == hist[:top]
    for c, h in parts[1:]:
        assert not any(h[:top])
        assert c[0] == sum(h[top:])
    if split <= 2:
        # not vacuous: the split level is divided among at least two shards
        assert sum(1 for _, h in parts if h[split] > 0) >= 2, [h[split] for _, h in parts]
    if split > depth:
        assert parts[0] == R.serial(key) and all(c == (0, 0, 0) for c, _ in parts[1:])


@pytest.mark.parametrize("args", R.TINY)
def test_shard_walk_equals_a_python_restatement(args):
    p = L.parse_uts_args(args)
    (nodes, _, depth), _ = L.uts_serial(p)
    assert nodes <= 1000
    assert R.python_shard_walk(p, 0, 1, 0, depth + 1) == L.uts_serial(p, depth + 1)
    for nshards, split in R.TINY_CONFIGS:
        owners = 0
        for s in range(nshards):
            want = R.python_shard_walk(p, s, nshards, split, depth + 1)
            got = L.uts_serial_shard(p, s, nshards, split, depth + 1)
            assert got == want, (args, s, nshards, split)
            owners += split <= depth and want[1][split] > 0
        assert owners >= 2 or split > depth, (args, nshards, split)


def test_shard_word_is_the_first_digest_word(golden):
    """state[0] of `state[0] % nshards` is bytes 0..3 of the reference's
    20-byte state, big-endian: the golden vectors' first eight hex digits.
    A BIN tree of a root and one leaf child (-b 1 -q 0) is owned, at split
    1, by the shard that word of the child's golden state names."""
    for v in golden("uts_goldens.json")["sha1"]:
        root = L.rng_init(v["seed"])
        assert root[0] == int(v["root"][:8], 16)
        for i, h in v["children"].items():
            assert L.rng_spawn(root, int(i))[0] == int(h[:8], 16)
        p = L.parse_uts_args(f"-t 0 -b 1 -q 0 -m 0 -r {v['seed']}")
        assert L.uts_serial(p)[0] == (2, 1, 1)
        for nshards in (2, 3, 7, 8):
            owner = int(v["children"]["0"][:8], 16) % nshards
            for s in range(nshards):
                want = (1 if s == 0 else 0) + (1 if s == owner else 0)
                assert L.uts_serial_shard(p, s, nshards, 1)[0][0] == want, (v["seed"], nshards, s)


@pytest.mark.parametrize("key", ["bin_m150", "glb_hybrid_m120", "bin_m100", "lds_balanced120"])
def test_host_mirror_caps_bin_rule_children_at_100(key):
    """hclib_hip_uts_num_children_host (the rule tables the device reads,
    evaluated on the host) against the oracle's numChildren at every node
    of the tree: a BIN-rule node of -m 150 or -m 120 has 100 children
    (uts.c:225-274 truncates to MAXNUMCHILDREN); BALANCED keeps its 120."""
    row, p = R.BY_KEY[key], R.params(key)
    hp = H.parse_uts_args(row.args)
    frontier, seen, most, full_below_root = [(L.rng_init(p.root_id), 0, p.type)], 0, 0, 0
    import ctypes as C

    while frontier:
        st, h, typ = frontier.pop()
        want = L.uts_num_children(p, typ, h, st)
        assert H.uts_num_children_host(hp, h, st) == want, (key, h, st)
        seen += 1
        most = max(most, want)
        full_below_root += h > 0 and want == 100
        ctype = L.oracle().ora_uts_child_type(C.byref(p), h)
        frontier.extend((L.rng_spawn(st, i), h + 1, ctype) for i in range(max(want, 0)))
    assert seen == row.nodes
    assert most == {"bin_m150": 2000, "glb_hybrid_m120": 100, "bin_m100": 500, "lds_balanced120": 120}[key]
    if key != "lds_balanced120":
        # the walk met BIN-rule nodes that spawn: 100 children each
        assert full_below_root >= 1, full_below_root


def test_a_stale_oracle_library_is_rebuilt():
    """loader.ensure_built looks for the newest entry point, not only for the
    files: a library without it counts as not built."""
    import os
    import tempfile

    assert L._has_symbol(os.path.join(L.BUILD, "liboracle.so"), b"ora_uts_serial_shard")
    with tempfile.NamedTemporaryFile() as f:
        f.write(b"\x7fELF ora_uts_serial ora_rng_spawn")
        f.flush()
        assert not L._has_symbol(f.name, b"ora_uts_serial_shard")
    assert not L._has_symbol(os.path.join(L.BUILD, "no_such.so"), b"ora_uts_serial_shard")
