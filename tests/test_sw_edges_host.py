"""ora_sw_edges (oracle/sw_oracle.c), the reference that tests/test_sw_edges_gpu.py
compares every SW tile's bottom row, right column and corner with, pinned
three ways without a GPU: against ora_sw_score's last row / last column of
the matrix cut at every tile row and tile column, against a plain Python DP,
and against the reference program's published scores."""
import os

import numpy as np
import pytest

from oracle import loader as L
from tests.conftest import GOLD

SHAPES = [(8, 8, 4, 4), (40, 30, 1, 1), (48, 36, 8, 6), (120, 90, 17, 13), (70, 200, 1, 64), (200, 70, 64, 1),
          (300, 130, 100, 130)]


def _seqs(n1, n2, seed):
    rng = np.random.default_rng(seed)
    return (bytes(rng.integers(1, 5, n1, dtype=np.int8).tobytes()),
            bytes(rng.integers(1, 5, n2, dtype=np.int8).tobytes()))


def _python_dp(s1, s2):
    """H[0..R][0..W] of smith_waterman.cpp's recurrence, cell by cell."""
    m = [[-1] * 5] + [[-1] + [2 if a == b else (-2 if (a + b) % 2 == 0 else -4) for b in range(1, 5)]
                      for a in range(1, 5)]
    h = [[-c for c in range(len(s1) + 1)]] + [[-r] + [0] * len(s1) for r in range(1, len(s2) + 1)]
    for r in range(1, len(s2) + 1):
        for c in range(1, len(s1) + 1):
            h[r][c] = max(h[r][c - 1] - 1, h[r - 1][c] - 1, h[r - 1][c - 1] + m[s2[r - 1]][s1[c - 1]])
    return h


def test_python_dp_scores_are_the_reference_matrix():
    """The Python DP's score table is alignment_score_matrix
    (smith_waterman.cpp:36-43): match 2, transition (A<->G, C<->T) -2,
    transversion -4 — and gives the published tiny score."""
    a = open(os.path.join(GOLD, "sw", "string1-tiny.txt"), "rb").read()
    b = open(os.path.join(GOLD, "sw", "string2-tiny.txt"), "rb").read()
    s1, s2 = L.sw_map(a)[:8], L.sw_map(b)[:8]
    assert _python_dp(s1, s2)[8][8] == 12
    assert _python_dp(bytes([1, 2, 3, 4]), bytes([3]))[1] == [-1, -2, -3, 0, -1]  # G vs A C G T


@pytest.mark.parametrize("n1,n2,tw,th", SHAPES)
def test_edges_are_the_last_row_and_column_of_every_cut(n1, n2, tw, th):
    s1, s2 = _seqs(n1, n2, n1 + n2)
    score, rows, cols, corners = L.sw_edges(s1, s2, tw, th)
    ntw, nth = n1 // tw, n2 // th
    assert rows.shape == (nth, ntw * tw) and cols.shape == (ntw, nth * th) and corners.shape == (nth, ntw)
    assert score == L.sw_score(s1, s2, tw, th) == rows[-1, -1] == cols[-1, -1] == corners[-1, -1]
    for i in range(nth):  # the matrix cut below tile row i: its last row
        _, lr, _ = L.sw_score(s1, s2[: (i + 1) * th], tw, th, want_edges=True)
        assert rows[i].tolist() == lr[1:], i
    for j in range(ntw):  # the matrix cut right of tile column j: its last column
        _, _, lc = L.sw_score(s1[: (j + 1) * tw], s2, tw, th, want_edges=True)
        assert cols[j].tolist() == lc[1:], j
    for i in range(nth):
        for j in range(ntw):
            assert corners[i, j] == rows[i, (j + 1) * tw - 1] == cols[j, (i + 1) * th - 1]


@pytest.mark.parametrize("n1,n2,tw,th", [(23, 19, 5, 3), (12, 9, 1, 1)])
def test_edges_against_a_python_dp(n1, n2, tw, th):
    s1, s2 = _seqs(n1, n2, 7)
    score, rows, cols, corners = L.sw_edges(s1, s2, tw, th)
    ntw, nth = n1 // tw, n2 // th
    W, R = ntw * tw, nth * th
    h = _python_dp(s1[:W], s2[:R])
    assert score == h[R][W]
    assert rows.tolist() == [h[(i + 1) * th][1:] for i in range(nth)]
    assert cols.tolist() == [[h[r][(j + 1) * tw] for r in range(1, R + 1)] for j in range(ntw)]
    assert corners.tolist() == [[h[(i + 1) * th][(j + 1) * tw] for j in range(ntw)] for i in range(nth)]


def test_one_by_one_tiles_make_every_cell_an_edge():
    s1, s2 = _seqs(12, 9, 3)
    _, rows, cols, corners = L.sw_edges(s1, s2, 1, 1)
    h = np.array(_python_dp(s1, s2))[1:, 1:]
    assert np.array_equal(rows, h) and np.array_equal(cols, h.T) and np.array_equal(corners, h)


@pytest.mark.parametrize("size", ["tiny", "medium"])
def test_last_value_is_the_published_score(golden, size):
    g = golden("sw_goldens.json")["published"][size]
    a = open(os.path.join(GOLD, "sw", f"string1-{size}.txt"), "rb").read()
    b = open(os.path.join(GOLD, "sw", f"string2-{size}.txt"), "rb").read()
    s1, s2 = L.sw_map(a), L.sw_map(b)
    score, rows, cols, corners = L.sw_edges(s1, s2, g["tile_w"], g["tile_h"])
    assert score == rows[-1, -1] == cols[-1, -1] == corners[-1, -1] == g["score"]
