"""Rodinia BFS restated in Python, and the graphs the tests run it on.

Two restatements of test/performance-regression/full-apps/rodinia/bfs:

  sweeps(g)  the reference's schedule, literally (bfs.ref.cpp:128-183): four
             arrays, per level one sweep over every vertex that relaxes the
             edges of the masked ones and one that moves the updating mask into
             the mask and the visited set, until a level changes nothing.
             Returns (cost, k), k the reference's sweep count.
  queue(g)   a queue BFS: (cost, frontiers, relaxed) with frontiers the list of
             vertex lists per level and relaxed the degrees of the reached
             vertices summed (every edge of a reached vertex is looked at once).

A graph is {"starting", "degree", "edges", "source"}: vertex v owns
edges[starting[v] : starting[v] + degree[v]] (Node, bfs.ref.cpp:32-36).

The fixtures under tests/golden/bfs are the graphs of FIXTURES written with
write_graph, and the result.txt the compiled reference wrote for each. All but
`tiny` are kept gzip-compressed (<name>.txt.gz, <name>.result.txt.gz: the text
is one number or one cost per line, tens of thousands of lines);
fixture_bytes and fixture_file give the text back. `python -m tests.bfs_ref
<dir>` writes the inputs again, byte for byte; pack() compresses a file the
way the committed ones were.
"""
import atexit
import gzip
import os
import random
import shutil
import sys
import tempfile

import numpy as np

MIN_EDGES, MAX_INIT_EDGES, MIN_WEIGHT, MAX_WEIGHT = 2, 4, 1, 10  # Rodinia's graphgen


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bfs")
_unpacked = None


def fixture_bytes(fname):
    """the bytes of tests/golden/bfs/<fname>, kept plain or as <fname>.gz"""
    p = os.path.join(GOLD, fname)
    if os.path.exists(p):
        return open(p, "rb").read()
    return gzip.open(p + ".gz", "rb").read()


def fixture_file(fname):
    """a path to tests/golden/bfs/<fname> as plain text: the file itself, or its
    .gz unpacked into a folder that lives as long as the process"""
    global _unpacked
    p = os.path.join(GOLD, fname)
    if os.path.exists(p):
        return p
    if _unpacked is None:
        _unpacked = tempfile.mkdtemp(prefix="bfs_golden_")
        atexit.register(shutil.rmtree, _unpacked, True)
    out = os.path.join(_unpacked, fname)
    if not os.path.exists(out):
        with open(out, "wb") as f:
            f.write(fixture_bytes(fname))
    return out


def pack(path):
    """<path> -> <path>.gz, reproducibly (no name, no time in the header)"""
    with open(path, "rb") as f, open(path + ".gz", "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as z:
            z.write(f.read())
    os.remove(path)


def graph(adj, source):
    """adjacency lists -> the CSR the reference reads"""
    deg = np.array([len(a) for a in adj], dtype=np.int32)
    start = np.zeros(len(adj), dtype=np.int32)
    if len(adj) > 1:
        start[1:] = np.cumsum(deg[:-1], dtype=np.int64)
    edges = np.array([h for a in adj for h in a], dtype=np.int32)
    return {"starting": start, "degree": deg, "edges": edges, "source": int(source)}


def sweeps(g):
    st, dg, ed, n = g["starting"].tolist(), g["degree"].tolist(), g["edges"].tolist(), len(g["starting"])
    mask, updating, visited = [False] * n, [False] * n, [False] * n
    mask[g["source"]] = visited[g["source"]] = True
    cost = [-1] * n
    cost[g["source"]] = 0
    k = 0
    while True:
        stop = False
        for tid in range(n):
            if mask[tid]:
                mask[tid] = False
                for i in range(st[tid], st[tid] + dg[tid]):
                    v = ed[i]
                    if not visited[v]:
                        cost[v] = cost[tid] + 1
                        updating[v] = True
        for tid in range(n):
            if updating[tid]:
                mask[tid] = visited[tid] = stop = True
                updating[tid] = False
        k += 1
        if not stop:
            break
    return np.array(cost, dtype=np.int32), k


def queue(g):
    st, dg, ed, n = g["starting"], g["degree"], g["edges"], len(g["starting"])
    cost = np.full(n, -1, dtype=np.int32)
    cost[g["source"]] = 0
    level, frontiers, relaxed = [g["source"]], [], 0
    while level:
        frontiers.append(level)
        nxt = []
        for v in level:
            relaxed += int(dg[v])
            for h in ed[st[v]:st[v] + dg[v]].tolist():
                if cost[h] < 0:
                    cost[h] = cost[v] + 1
                    nxt.append(h)
        level = nxt
    return cost, frontiers, relaxed


def queue_fast(g):
    """queue() with a level's edges gathered by numpy, for graphs of 2^17 vertices and more"""
    st, dg, ed, n = g["starting"].astype(np.int64), g["degree"].astype(np.int64), g["edges"], len(g["starting"])
    cost = np.full(n, -1, dtype=np.int32)
    cost[g["source"]] = 0
    level, sizes, relaxed, d = np.array([g["source"]], dtype=np.int64), [], 0, 0
    while level.size:
        sizes.append(int(level.size))
        cnt = dg[level]
        relaxed += int(cnt.sum())
        idx = np.repeat(st[level] - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(int(cnt.sum()))
        heads = np.unique(ed[idx])
        level = heads[cost[heads] < 0].astype(np.int64)
        d += 1
        cost[level] = d
    return cost, sizes, relaxed


def generate(n, seed, source=0, isolated=0):
    """A graph as Rodinia's graphgen makes them: every vertex draws 2 .. 4
    partners, each link goes both ways (so the mean degree is about 6). The
    last `isolated` vertices take no part: no path leads to them."""
    rng = random.Random(seed)
    live = n - isolated
    adj = [[] for _ in range(n)]
    for v in range(live):
        for _ in range(rng.randint(MIN_EDGES, MAX_INIT_EDGES)):
            w = rng.randrange(live)
            adj[v].append(w)
            adj[w].append(v)
    return graph(adj, source)


def generate_fast(n, seed, source=0):
    """generate() with numpy's generator, for graphs too large for lists"""
    rng = np.random.RandomState(seed)
    cnt = rng.randint(MIN_EDGES, MAX_INIT_EDGES + 1, size=n)
    tail = np.repeat(np.arange(n, dtype=np.int64), cnt)
    head = rng.randint(0, n, size=tail.size).astype(np.int64)
    a, b = np.concatenate((tail, head)), np.concatenate((head, tail))
    by = np.argsort(a, kind="stable")
    deg = np.bincount(a, minlength=n).astype(np.int32)
    start = np.zeros(n, dtype=np.int32)
    start[1:] = np.cumsum(deg[:-1])
    return {"starting": start, "degree": deg, "edges": b[by].astype(np.int32), "source": int(source)}


def _tiny():
    return graph([[1, 2], [3], [3], [0], [0]], 0)  # nothing leads to 4


def _chain():
    return graph([[v + 1] if v < 199 else [] for v in range(200)], 0)


def _star():
    return graph([list(range(1, 3001))] + [[0] for _ in range(3000)], 0)


def _sinks():
    # 0 -> 1 .. 8 -> 300 sinks, each edge one way: the last level has no edge at all
    mid = [[9 + 40 * (v - 1) + i for i in range(40)] for v in range(1, 9)]
    mid[7] = mid[7][:20]
    return graph([list(range(1, 9))] + mid + [[] for _ in range(300)], 0)


def _clash():
    # complete bipartite 64 x 64 with a self-loop on every vertex and every edge
    # of the left side doubled: 64 lanes claim one vertex in one batch
    left, right = list(range(64)), list(range(64, 128))
    adj = [[v] + right + right for v in left] + [[v] + left for v in right]
    return graph(adj, 0)


def _rand4k():
    return generate(4096, 20, source=1234, isolated=37)


FIXTURES = {"tiny": _tiny, "chain": _chain, "star": _star, "sinks": _sinks, "clash": _clash, "rand4k": _rand4k}


def write_graph(g, path, seed=7):
    """Rodinia's text format (what bfs.ref.cpp:84-121 reads); the weights, which
    the reference drops, are graphgen's 1 .. 10"""
    rng = random.Random(seed)
    with open(path, "w") as f:
        f.write("%d\n" % len(g["starting"]))
        for s, d in zip(g["starting"].tolist(), g["degree"].tolist()):
            f.write("%d %d\n" % (s, d))
        f.write("\n%d\n\n%d\n" % (g["source"], len(g["edges"])))
        for h in g["edges"].tolist():
            f.write("%d %d\n" % (h, rng.randint(MIN_WEIGHT, MAX_WEIGHT)))


def read_graph(path):
    """the reference's fscanf sequence: whitespace-separated integers"""
    t = [int(x) for x in open(path).read().split()]
    n = t[0]
    pairs = np.array(t[1:1 + 2 * n], dtype=np.int32).reshape(n, 2)
    src, m = t[1 + 2 * n], t[2 + 2 * n]
    ed = np.array(t[3 + 2 * n:3 + 2 * n + 2 * m], dtype=np.int32).reshape(m, 2)
    return {"starting": pairs[:, 0].copy(), "degree": pairs[:, 1].copy(), "edges": ed[:, 0].copy(), "source": src}


def format_result(cost):
    """result.txt as the reference writes it (bfs.ref.cpp:189-192)"""
    return "".join("%d) cost:%d\n" % (i, c) for i, c in enumerate(np.asarray(cost).tolist()))


if __name__ == "__main__":
    for name, make in FIXTURES.items():
        write_graph(make(), os.path.join(sys.argv[1], name + ".txt"))
