"""Every Smith-Waterman tile body and schedule against the oracle's tile
edges, not one score. The recurrence is a max, and a max hides a wrong cell
unless that cell lies on an optimal path to something compared; so every
tile's bottom row, right column and corner (the reference's three promises
per tile, smith_waterman.cpp:212-226) are read back (hclib_hip_sw_edges,
hclib_hip_sw_band_bottoms) and compared with ora_sw_edges — the plain
recurrence, pinned without a GPU by tests/test_sw_edges_host.py — value for
value, on random inputs, all-match inputs and inputs whose optimal path runs
off the diagonal. Each path's mask of filled arrays is asserted too: a path
must not silently stop reporting its right columns.

Compared per path:            bottoms  rights  corners
  queue, dag-wave, dag-wg, dag-pk  x       x       x
  rows1, band-rows                 x       -       x (the bottom row's last)
  band sessions                    x       (the band's right column)
With tw = 1 and th = 1 every matrix cell is a compared edge cell on queue,
dag-wave and rows1 ((40, 30, 1, 1)); th = 1 alone makes every cell a bottom
row ((200, 130, 64, 1)), tw = 1 alone a right column ((130, 200, 1, 64), and
under dag-wg / dag-pk the tw = 1 shapes below)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hclib_amd as H  # noqa: E402
from oracle import loader as L  # noqa: E402
from tests.test_gpu import _sw_bands_in_order  # noqa: E402

FAMILIES = ("random", "match", "shifted")
FORMS = (11, 12, 14, 21, 22, 211, 212, 214, 411, 412, 414)
ALL, NO_RIGHTS = (True, True, True), (True, False, True)


@pytest.fixture(scope="module", autouse=True)
def device():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    H.init(0)
    yield


@functools.lru_cache(maxsize=None)
def _inputs(n1, n2, tw, th, family):
    """random: seeded; match: one letter in both sequences (+4 in G on every
    diagonal); shifted: s2 = s1 moved by about a third of a tile, so the
    optimal path runs beside the diagonal, through cells a score never sees."""
    rng = np.random.default_rng(5 + n1 * 31 + n2)
    if family == "match":
        return bytes([1]) * n1, bytes([1]) * n2
    if family == "shifted":
        d = max(1, (tw if tw >= 3 else th) // 3)
        base = rng.integers(1, 5, max(n1, n2) + d, dtype=np.int8).tobytes()
        return bytes(base[:n1]), bytes(base[d:d + n2])
    return (bytes(rng.integers(1, 5, n1, dtype=np.int8).tobytes()),
            bytes(rng.integers(1, 5, n2, dtype=np.int8).tobytes()))


@functools.lru_cache(maxsize=None)
def _oracle(n1, n2, tw, th, family):
    """ora_sw_edges, once per input: shared by every path, never modified."""
    out = L.sw_edges(*_inputs(n1, n2, tw, th, family), tw, th)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _same(got, want, what, tag):
    assert got.shape == want.shape and got.dtype == np.int32, (what, tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        k = tuple(int(x) for x in bad[0])
        pytest.fail(f"{what} differ at {len(bad)} of {got.size} values; first at {k}: got {got[k]}, "
                    f"oracle {want[k]} ({tag})")


def _compare(shape, family, path, mask, form=0):
    """One run: the path and form that ran, the mask, the score, and every
    array the mask reports, against the oracle."""
    n1, n2, tw, th = shape
    s1, s2 = _inputs(n1, n2, tw, th, family)
    want_score, rows, cols, corners = _oracle(n1, n2, tw, th, family)
    score, st, e = H.sw_edges(s1, s2, tw, th)
    tag = (shape, family, path, form)
    assert (e["path"], e["form"]) == (path, form), tag
    assert tuple(e[k] is not None for k in ("bottoms", "rights", "corners")) == mask, tag
    assert score == want_score and st["tiles"] == (n1 // tw) * (n2 // th), (tag, score, want_score)
    _same(e["bottoms"], rows, "bottom rows [tile row][column]", tag)
    if mask[1]:
        _same(e["rights"], cols, "right columns [tile column][row]", tag)
    _same(e["corners"], corners, "corners [tile row][tile column]", tag)


# ------------------------------------------------------------ one-wave tile
ONE_WAVE = [(40, 30, 1, 1), (200, 130, 64, 1), (130, 200, 1, 64), (300, 200, 17, 13), (260, 210, 65, 70),
            (1000, 777, 64, 300)]
ROWS1_ONLY = [(256, 512, 64, 256), (384, 512, 128, 256),  # the progressive hand-off applies
              (300, 512, 100, 256)]                        # ... and does not (tw % 64)


@pytest.mark.parametrize("shape", ONE_WAVE, ids=str)
@pytest.mark.parametrize("sched", ["queue", "dag-wave"])
def test_one_wave_tile_on_counters_and_promises(shape, sched, monkeypatch):
    """sw_tile<false>: the queue schedule and the promise DAG's one-wave tile
    tasks keep the reference's three plain arrays; all three are compared."""
    monkeypatch.setenv("HCLIB_HIP_SW_SCHED", "queue" if sched == "queue" else "dag")
    monkeypatch.setenv("HCLIB_HIP_SW_DAG_WAVE", "1")
    for family in FAMILIES:
        _compare(shape, family, sched, ALL)


@pytest.mark.parametrize("shape", ONE_WAVE + ROWS1_ONLY, ids=str)
@pytest.mark.parametrize("progressive", ["0", "1"])
def test_one_wave_tile_rows(shape, progressive, monkeypatch):
    """sw_tile<true>: the one-wave row schedule publishes bottom rows as
    granules, whole (0) or in 64-column chunks (1, where th = 256 and
    tw % 64 == 0); right columns stay in LDS, corners are the rows' last."""
    monkeypatch.setenv("HCLIB_HIP_SW_SCHED", "rows1")
    monkeypatch.setenv("HCLIB_HIP_SW_PROGRESSIVE", progressive)
    for family in FAMILIES:
        _compare(shape, family, "rows1", NO_RIGHTS)


# ----------------------------------------------------- multi-wave band rows
def _form_for(form, th):
    """sw_pick_form's fallback: four rows per lane need th % 256 == 0, two
    th % 128 == 0; else the same skew and hand-off with fewer rows (the C++
    rule itself is checked without a GPU by tests/test_sw_plan.py)."""
    if form > 400 and th % 256:
        form -= 200
    if form > 200 and th % 128:
        form -= 200
    return form


def test_form_fallback_rule():
    assert [_form_for(f, 256) for f in FORMS] == list(FORMS)
    assert [_form_for(f, 128) for f in FORMS] == [11, 12, 14, 21, 22, 211, 212, 214, 211, 212, 214]
    assert [_form_for(f, 896) for f in FORMS] == [11, 12, 14, 21, 22, 211, 212, 214, 211, 212, 214]
    for th in (64, 192):
        assert [_form_for(f, th) for f in FORMS] == [11, 12, 14, 21, 22, 11, 12, 14, 11, 12, 14]


BANDS = [(20, 128, 1, 64), (20, 256, 1, 128), (12, 512, 1, 256),  # tw = 1: under dag every column is compared
         (90, 192, 30, 64),      # below one 64-column chunk, three tile rows
         (195, 128, 65, 64),     # ragged last chunk
         (1300, 128, 650, 64),   # past the 512-column ring (wrap slot)
         (130, 896, 65, 896),    # 14 compute waves (one row per lane), 7 (two)
         (128, 384, 64, 192)]    # 3 waves; the 2xx and 4xx forms fall back


@pytest.mark.parametrize("shape", BANDS, ids=str)
@pytest.mark.parametrize("sched", ["rows", "dag"])
def test_multiwave_band_row_every_form(shape, sched, monkeypatch):
    """sw_band_row in all 11 (rows per lane, skew, hand-off) forms: under the
    row schedule (granules out, no right columns) and as the promise DAG's
    workgroup tile tasks (plain arrays, all three; the from-LDS left column
    and corner of a kept neighbour included). The form that ran is the one
    asked for, after sw_pick_form's fallback for th."""
    monkeypatch.setenv("HCLIB_HIP_SW_SCHED", sched)
    monkeypatch.setenv("HCLIB_HIP_SW_PK", "0")  # th = 256: the band body, not the packed one
    path, mask = ("band-rows", NO_RIGHTS) if sched == "rows" else ("dag-wg", ALL)
    for form in FORMS:
        monkeypatch.setenv("HCLIB_HIP_SW_FORM", str(form))
        for family in FAMILIES:
            _compare(shape, family, path, mask, _form_for(form, shape[3]))


def test_multiwave_default_forms(monkeypatch):
    """Without HCLIB_HIP_SW_FORM: 412 under the row schedule, 214 on the DAG."""
    shape = (128, 512, 64, 256)
    _compare(shape, "random", "band-rows", NO_RIGHTS, 412)
    monkeypatch.setenv("HCLIB_HIP_SW_SCHED", "dag")
    monkeypatch.setenv("HCLIB_HIP_SW_PK", "0")
    _compare(shape, "random", "dag-wg", ALL, 214)


# -------------------------------------------------------- packed-half body
@pytest.mark.parametrize("tw", [1, 63, 64, 65, 256, 257, 512])
def test_packed_half_body(tw, monkeypatch):
    """256-row tiles on the promise DAG, three tile rows and columns (left, up
    and diagonal futures; LDS-kept and global hand-offs): the packed-half body
    (tagged granules for all three outputs) and, on the same inputs, the int32
    band body. All-match inputs at tw = 512 reach the f16-exact bound of 2048."""
    monkeypatch.setenv("HCLIB_HIP_SW_SCHED", "dag")
    shape = (3 * tw + tw // 3, 768, tw, 256)
    for family in FAMILIES:
        monkeypatch.setenv("HCLIB_HIP_SW_PK", "1")
        _compare(shape, family, "dag-pk", ALL)
        monkeypatch.setenv("HCLIB_HIP_SW_PK", "0")
        _compare(shape, family, "dag-wg", ALL, 214)


# ----------------------------------------------------------- band sessions
@pytest.mark.parametrize("n1,n2,tw,th,nbands,block_rows", [(513, 1025, 17, 13, 5, 7), (1024, 512, 64, 256, 4, 1)])
def test_band_sessions_bottom_rows(n1, n2, tw, th, nbands, block_rows):
    """Column-band sessions (one-wave rows at th = 13, band rows at 256): each
    band's bottom rows are the oracle's rows over the band's columns, its
    right column the oracle's last column of the matrix cut at the band's edge."""
    for family in FAMILIES:
        s1, s2 = _inputs(n1, n2, tw, th, family)
        want_score, rows, cols, _ = _oracle(n1, n2, tw, th, family)
        got = []
        score, tiles, rights = _sw_bands_in_order(s1, s2, tw, th, nbands, block_rows,
                                                  before_end=lambda band, stream: got.append(
                                                      (band.j0, band.j1, band.bottoms(stream))))
        assert score == want_score and tiles == (n1 // tw) * (n2 // th), family
        assert len(got) == nbands and got[0][0] == 0 and got[-1][1] == n1 // tw
        for j0, j1, bottoms in got:
            _same(bottoms, rows[:, j0 * tw:j1 * tw], "band bottom rows [tile row][column]", (family, j0, j1))
        for j1, right in rights:
            if right is not None:
                _, _, col = L.sw_score(s1[:j1 * tw], s2, tw, th, want_edges=True)
                assert right == col[1:] == cols[j1 - 1].tolist(), (family, j1)
