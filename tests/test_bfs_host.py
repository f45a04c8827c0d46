"""Rodinia BFS on the host alone: the fixtures of tests/golden/bfs are the
recorded files; both restatements of tests/bfs_ref.py reproduce every
result.txt of the compiled reference byte for byte and agree with each other on
seeded random graphs; hclib_hip_bfs_read_input reads what the reference's
fscanf sequence reads; every graph for which the reference's behaviour is
undefined is refused as EINVAL before a device is looked for; and
hclib_hip_bfs_bounds equals the arena laid out by hand. No GPU."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import hclib_amd as H
from tests import bfs_ref as R

GOLD = R.GOLD
EINVAL = -2

SHA256 = {
    "chain.result.txt": "24d44ebf0504016aad3050b8bf147003cc3527e2b3300f1eeedf96202f0647f2",
    "chain.txt": "0fbd62e99b9d10cb727eed4a5997ef9811f28e941b0a74fb31de94e92ebf2bcf",
    "clash.result.txt": "fcb11508bf667441b10c9247fa044d42009625050ba85a6636ed0b91bfd132b9",
    "clash.txt": "152cfd9df2c59d9b50c4edcdefacd7dc6ace284a2eca0dc78816bcea9d7ae2a2",
    "rand4k.result.txt": "478afb3b0fb2befc98bf1a6245336b688232bfb319b7acc7a5ec009f40205be4",
    "rand4k.txt": "f838a53ca147a42451d68097b22e8889c462141aacf5c1b5e080331552f671ea",
    "sinks.result.txt": "fbf90c6b272de4f507b51af43ec76318d18d9bb2681bf0b2e40e83a1ba6b4354",
    "sinks.txt": "9bc94038d5146b4ec0ad5a58b6b2efe010d5b0f19f489b2abcd10b74367a0625",
    "star.result.txt": "9428ef595ce61bd43074752fddae215a4eb1aa995669ef8df7038f5eb7afd7e3",
    "star.txt": "fd4491931db4f9e8f9b023a8a0f1654f89ae87f3f628a74f1e632d9497c5eda0",
    "tiny.result.txt": "bbbd57f7b3c20bb0fe9b7d3b249dd2b8cc816524475a2f4563ab56884b2183b8",
    "tiny.txt": "df85fbd1ea50c764a6a5135a98e9fb60ae64e32f7bc99f25a2a4bd69af773350",
}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("starting", "degree", "edges")) and a["source"] == b["source"]


def test_fixtures_are_the_recorded_files():
    # the text the reference read and wrote; all but tiny are kept as <name>.gz
    assert sorted(f[:-3] if f.endswith(".gz") else f for f in os.listdir(GOLD)) == sorted(SHA256)
    for name, want in SHA256.items():
        assert hashlib.sha256(R.fixture_bytes(name)).hexdigest() == want, name


def test_fixture_inputs_are_what_the_generators_write(tmp_path):
    for name, make in R.FIXTURES.items():
        p = str(tmp_path / (name + ".txt"))
        R.write_graph(make(), p)
        assert open(p, "rb").read() == R.fixture_bytes(name + ".txt"), name


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_restatements_reproduce_the_references_result(name):
    g = R.read_graph(R.fixture_file(name + ".txt"))
    gold = R.fixture_bytes(name + ".result.txt").decode()
    cost, frontiers, relaxed = R.queue(g)
    assert R.format_result(cost) == gold
    swept, k = R.sweeps(g)
    assert R.format_result(swept) == gold and k == len(frontiers)
    fast, sizes, frelaxed = R.queue_fast(g)
    assert np.array_equal(fast, cost) and sizes == [len(f) for f in frontiers] and frelaxed == relaxed
    assert relaxed == int(g["degree"][cost >= 0].sum())
    for d, f in enumerate(frontiers):
        assert sorted(f) == np.flatnonzero(cost == d).tolist()


def test_fixtures_exercise_what_they_are_named_for():
    q = {n: R.queue(R.read_graph(R.fixture_file(n + ".txt"))) for n in R.FIXTURES}
    assert q["tiny"][0].tolist() == [0, 1, 1, 2, -1]
    assert [len(f) for f in q["chain"][1]] == [1] * 200
    assert [len(f) for f in q["star"][1]] == [1, 3000]  # 3000 children > 64 * 8 pieces
    g = R.read_graph(R.fixture_file("sinks.txt"))
    assert [len(f) for f in q["sinks"][1]] == [1, 8, 300] and not g["degree"][q["sinks"][1][2]].any()
    g = R.read_graph(R.fixture_file("clash.txt"))
    assert [len(f) for f in q["clash"][1]] == [1, 64, 63] and q["clash"][2] == 64 * 129 + 64 * 65
    assert all(v in g["edges"][g["starting"][v]:g["starting"][v] + g["degree"][v]] for v in range(128))  # self-loops
    g = R.read_graph(R.fixture_file("rand4k.txt"))
    assert g["source"] == 1234 and (q["rand4k"][0] < 0).sum() == 37 and 5.5 < g["degree"].mean() < 6.5


def test_restatements_agree_on_seeded_random_graphs():
    for seed in range(50):
        n = 1 + (seed * 37) % 300
        g = R.generate(n, seed, source=seed % n, isolated=min(seed % 5, n - 1))
        if seed % 7 == 0:  # a directed variant: drop every third edge of every list
            adj = [g["edges"][s:s + d].tolist()[::3] for s, d in zip(g["starting"], g["degree"])]
            g = R.graph(adj, g["source"])
        a, k = R.sweeps(g)
        b, frontiers, relaxed = R.queue(g)
        c, sizes, _ = R.queue_fast(g)
        assert np.array_equal(a, b) and np.array_equal(b, c) and k == len(frontiers) == len(sizes), seed
        assert relaxed == int(g["degree"][b >= 0].sum())
    g = R.generate_fast(5000, 3, source=11)
    assert np.array_equal(R.queue(g)[0], R.queue_fast(g)[0]) and 5.5 < g["degree"].mean() < 6.5


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_read_input_round_trips_every_fixture(name, tmp_path):
    path = R.fixture_file(name + ".txt")
    g = H.bfs_read_input(path)
    assert _same(g, R.read_graph(path)) and _same(g, R.FIXTURES[name]())
    assert all(g[k].dtype == np.int32 for k in ("starting", "degree", "edges"))
    again = str(tmp_path / "again.txt")
    R.write_graph(g, again)
    assert open(again, "rb").read() == open(path, "rb").read()


def test_read_input_refusals(tmp_path):
    lib = H.lib()
    counts = (C.c_int64 * 3)()
    assert lib.hclib_hip_bfs_read_input(os.fsencode(str(tmp_path / "absent.txt")), None, None, None, counts) == EINVAL
    assert b"cannot be opened" in lib.hclib_hip_last_error()
    assert lib.hclib_hip_bfs_read_input(None, None, None, None, counts) == EINVAL
    tiny = os.fsencode(os.path.join(GOLD, "tiny.txt"))
    assert lib.hclib_hip_bfs_read_input(tiny, None, None, None, None) == EINVAL
    for text, word in (("", b"node count"), ("3\n0 1\n1 1\n", b"node 2"), ("2\n0 1\n1 1\n", b"source"),
                       ("2\n0 1\n1 1\n0\n", b"edge count"), ("2\n0 1\n1 1\n0\n2\n1 5\n0\n", b"edge 1"),
                       ("-4\n", b"node count")):
        p = tmp_path / "bad.txt"
        p.write_text(text)
        assert lib.hclib_hip_bfs_read_input(os.fsencode(str(p)), None, None, None, counts) == EINVAL, text
        assert word in lib.hclib_hip_last_error(), lib.hclib_hip_last_error()
    # arrays sized for another file
    a = np.zeros(8, dtype=np.int32)
    counts[0], counts[1], counts[2] = 4, 6, 0
    assert lib.hclib_hip_bfs_read_input(tiny, a.ctypes.data, a.ctypes.data, a.ctypes.data, counts) == EINVAL
    assert b"node count differs" in lib.hclib_hip_last_error()
    counts[0], counts[1] = 5, 7
    assert lib.hclib_hip_bfs_read_input(tiny, a.ctypes.data, a.ctypes.data, a.ctypes.data, counts) == EINVAL
    assert b"edge count differs" in lib.hclib_hip_last_error()
    assert lib.hclib_hip_bfs_read_input(tiny, a.ctypes.data, None, a.ctypes.data, counts) == EINVAL


def test_every_refusal_is_einval_without_a_device():
    lib = H.lib()
    out2 = (C.c_uint64 * 2)()
    res = H.BfsResult()
    good = R.FIXTURES["tiny"]()
    cost = np.zeros(8, dtype=np.int32)

    def both(word, form=0, n_nodes=None, n_edges=None, null=(), **change):
        g = dict(good, **{k: np.array(v, dtype=np.int32) for k, v in change.items() if k != "source"})
        src = change.get("source", good["source"])
        p = {k: None if k in null else g[k].ctypes.data for k in ("starting", "degree", "edges")}
        n = len(g["starting"]) if n_nodes is None else n_nodes
        m = len(g["edges"]) if n_edges is None else n_edges
        assert lib.hclib_hip_bfs_bounds(p["starting"], p["degree"], n, p["edges"], m, src, form, out2) == EINVAL, word
        assert word in lib.hclib_hip_last_error(), lib.hclib_hip_last_error()
        assert lib.hclib_hip_bfs(p["starting"], p["degree"], n, p["edges"], m, src, form, cost.ctypes.data, C.byref(res),
                                 None, None) == EINVAL, word
        assert word in lib.hclib_hip_last_error(), lib.hclib_hip_last_error()

    both(b"NULL", null=("starting",))
    both(b"NULL", null=("degree",))
    both(b"edges is NULL", null=("edges",))
    both(b"n_nodes", n_nodes=0)
    both(b"n_nodes", n_nodes=-3)
    both(b"n_nodes", n_nodes=1 << 24)
    both(b"n_edges", n_edges=-1)
    both(b"source", source=5)
    both(b"source", source=-1)
    both(b"degree", degree=[2, 1, -1, 1, 1])
    both(b"degree", degree=[2, 1, 1 << 24, 1, 1])
    both(b"are outside", degree=[2, 1, 1, 1, 2])  # starting + degree > n_edges
    both(b"are outside", n_edges=5)
    both(b"are outside", starting=[0, 2, -1, 4, 5])
    both(b"are outside", starting=[0, 2, 3, 4, 6])
    both(b"leads to vertex", edges=[1, 2, 3, 3, 0, 5])
    both(b"leads to vertex", edges=[1, 2, 3, -1, 0, 0])
    both(b"form", form=2)
    both(b"form", form=-1)
    p = [good[k].ctypes.data for k in ("starting", "degree", "edges")]
    args = (p[0], p[1], 5, p[2], 6, 0)
    assert lib.hclib_hip_bfs_bounds(*args, 0, None) == EINVAL
    assert lib.hclib_hip_bfs(*args, 0, None, C.byref(res), None, None) == EINVAL
    assert lib.hclib_hip_bfs(*args, 0, cost.ctypes.data, None, None, None) == EINVAL
    assert lib.hclib_hip_bfs(*args, 1, cost.ctypes.data, C.byref(res), None, cost.ctypes.data) == EINVAL  # async, order
    assert b"order" in lib.hclib_hip_last_error()
    # the binding's own checks
    with pytest.raises(ValueError):
        H.bfs(good, "bottom-up")
    with pytest.raises(ValueError):
        H.bfs_bounds(dict(good, degree=good["degree"][:4]))
    with pytest.raises(H.HclibError, match="source"):
        H.bfs_bounds(dict(good, source=7))


def test_bounds_equal_the_layout_by_hand():
    def al(b):
        return (b + 255) // 256 * 256

    graphs = [R.FIXTURES[n]() for n in R.FIXTURES] + [R.graph([[]], 0), R.graph([[0, 0, 0]], 0)]
    for g in graphs:
        n, m = len(g["starting"]), len(g["edges"])
        shared = 256 + 3 * al(4 * n) + al(4 * m)
        assert H.bfs_bounds(g, "async") == {"arena_bytes": shared, "items": n + m}
        assert H.bfs_bounds(g, "level") == {"arena_bytes": shared + al(4 * n) + al(4 * (n + 2)), "items": n + m}
        # the bound holds with equality exactly where every vertex is reached
        cost, frontiers, relaxed = R.queue(g)
        reached = sum(len(f) for f in frontiers)
        assert reached + relaxed <= n + m and (reached + relaxed == n + m) == (reached == n)
