"""Every launch variant of hclib_hip_uts_search against the serial oracle:
the trees of tests/uts_ref.py, each whole (the plain kernel), with its
per-level histogram (the FEAT = 1 kernel), in shards — every shard's own
counts and histogram against the oracle's shard walk, not only their sum —
and on one- and four-wave grids. The launch record
(hclib_hip_uts_last_launch) shows that each row ran the kernel it was
chosen for. All comparisons are exact; one test per tree holds all of that
tree's launches (a few hundred to 300,000 nodes each)."""
import pytest

pytestmark = pytest.mark.gpu

import hclib_amd as H  # noqa: E402
from tests import uts_ref as R  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def device():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    H.init(0)
    yield


@pytest.fixture(autouse=True)
def short_spin_limit(monkeypatch):
    # a lost hand-off comes back as an error in 3 s, not 20
    monkeypatch.setenv("HCLIB_HIP_SPIN_LIMIT_MS", "3000")


def _counts(r):
    return (r["nodes"], r["leaves"], r["max_depth"])


def _whole(row, **want):
    r = H.uts(row.args)
    shape = H.uts_last_launch()
    assert _counts(r) == (row.nodes, row.leaves, row.depth), (row.key, shape)
    assert shape["mode"] == row.mode and shape["feat"] == 0, (row.key, shape)
    for k, v in want.items():
        assert shape[k] == v, (row.key, k, shape)


def _histogram(row):
    counts, hist = R.serial(row.key)
    r = H.uts(row.args, max_levels=row.depth + 1)
    shape = H.uts_last_launch()
    assert _counts(r) == counts and tuple(r["levels"]) == hist, (row.key, shape)
    assert shape["mode"] == row.mode and shape["feat"] == 1, (row.key, shape)


def _shards(row, nshards, split):
    want_launch = R.expect_shard_launch(row, split)
    for s in range(nshards):
        counts, hist = R.serial_shard(row.key, s, nshards, split)
        where = (row.key, s, nshards, split)
        r = H.uts(row.args, s, nshards, split)
        shape = H.uts_last_launch()
        assert _counts(r) == counts, (where, shape)
        assert shape["mode"] == row.mode, (where, shape)
        if want_launch is not None:
            assert shape["feat"] == want_launch[0], (where, shape)
            if want_launch[1] is not None:
                assert shape["seeded"] == want_launch[1], (where, shape)
        # ... and with the per-level counts (the worker loop filters and counts)
        r = H.uts(row.args, s, nshards, split, max_levels=row.depth + 1)
        shape = H.uts_last_launch()
        assert _counts(r) == counts and tuple(r["levels"]) == hist, (where, shape)
        assert shape["mode"] == row.mode and shape["feat"] == 1, (where, shape)


@pytest.mark.parametrize("key", [r.key for r in R.ROWS])
def test_uts_tree(key, monkeypatch):
    row = R.BY_KEY[key]
    _whole(row)
    _histogram(row)
    if key == "glb_cyclic":
        # fewer levels than the tree has: the histogram is cut, the counts are not
        r = H.uts(row.args, max_levels=3)
        assert _counts(r) == R.serial(key)[0] and tuple(r["levels"]) == R.serial(key)[1][:3]
    if key in R.SHARD_KEYS:
        for nshards, split in R.shard_configs(row):
            _shards(row, nshards, split)
    if key in R.SMALL_GRID_KEYS:
        for grid in (1, 4):
            monkeypatch.setenv("HCLIB_HIP_GRID", str(grid))
            if key == "fix_b40":
                # one wave takes the root's 63 children (past its target of 16
                # slots) as its share; four waves (target 64) would pass that
                # level and be handed 2,177 / 4 slots each, more than half a
                # 512-item ring: that launch starts unseeded
                _whole(row, grid=grid, seeded=1 if grid == 1 else 0)
            else:
                _whole(row, grid=grid)
        monkeypatch.delenv("HCLIB_HIP_GRID")
    if key == "bin_m3":
        # two waves: a shard's part of the level past the split (~1,000
        # slots) is more than a quarter of each ring, so nothing is seeded
        # and the worker loop filters
        monkeypatch.setenv("HCLIB_HIP_GRID", "2")
        for s in range(2):
            r = H.uts(row.args, s, 2, 1)
            shape = H.uts_last_launch()
            assert _counts(r) == R.serial_shard(key, s, 2, 1)[0], (s, shape)
            assert (shape["grid"], shape["feat"], shape["seeded"]) == (2, 1, 0), (s, shape)
        monkeypatch.delenv("HCLIB_HIP_GRID")


def test_uts_seeding_knobs_refused_on_the_host(golden, monkeypatch):
    """A seeding / ring knob whose value cannot fit the ring is refused before
    the launch with a message that names it (128 slots per wave on T1 used to
    end in "device error 2 (LDS ring overflow)"), the next search is
    unaffected, and a value that fits (32) is still taken."""
    pub = golden("uts_goldens.json")["published"]["T1"]
    for knob, value in [("HCLIB_HIP_SEED_PER_WAVE", "128"), ("HCLIB_HIP_SEED_PER_WAVE", "0"),
                        ("HCLIB_HIP_SPILL_LO", "513"), ("HCLIB_HIP_SPILL_LO", "0"), ("HCLIB_HIP_UTS_RING", "300")]:
        monkeypatch.setenv(knob, value)
        with pytest.raises(H.HclibError, match=f"{knob}={value} "):
            H.uts(pub["args"])
        monkeypatch.delenv(knob)
    r = H.uts(pub["args"])
    assert _counts(r) == (pub["nodes"], pub["leaves"], pub["depth"])
    assert H.uts_last_launch()["seeded"] == 1
    monkeypatch.setenv("HCLIB_HIP_SEED_PER_WAVE", "32")
    r = H.uts(pub["args"])
    assert _counts(r) == (pub["nodes"], pub["leaves"], pub["depth"])
    shape = H.uts_last_launch()
    assert shape["seeded"] == 1 and shape["seed_target"] == 32 * shape["grid"], shape
