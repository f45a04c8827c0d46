"""The narrow loop's overflow exit (include/hclib_hip/hx_sched.h narrow_shed):
a level of a BIN tree that outgrows one batch inside the fixed-size narrow
loop keeps some spawners' children and writes the others' straight into idle
siblings' LDS inboxes. Every BIN row of tests/uts_ref.py that the fixed-size
loop runs (m <= 8) is searched whole with the exit on and off
(HCLIB_HIP_NARROW_SHED), on the default grid and on one workgroup of four
waves (three siblings), bin_m3 also in two shards: the counts equal the
serial oracle's exactly in every run, the exit's counters
(hclib_hip_last_shed_counters) are all 0 with it off, add up with it on
(exits = placed + fallbacks), and over the m >= 2 rows on four waves both
outcomes occur. Launches are a few hundred to 300,000 nodes each and run
once (shared by the tests below)."""
import functools
import os

import pytest

pytestmark = pytest.mark.gpu

import hclib_amd as H  # noqa: E402
from tests import uts_ref as R  # noqa: E402

OVERFLOWING = ["bin_m2", "bin_m3", "bin_m4", "bin_m6", "bin_m7", "bin_g3"]  # m >= 2: levels can outgrow a batch
QUIET = ["one_bin", "bin_b2_5", "bin_m1"]  # nothing to shed: no children, a 7-node tree, m = 1
GRIDS = [0, 4]  # 0: the default grid; 4: one workgroup, three siblings
KNOBS = ("HCLIB_HIP_NARROW_SHED", "HCLIB_HIP_NARROW_SHED_SIBS", "HCLIB_HIP_GRID", "HCLIB_HIP_SPIN_LIMIT_MS")


@pytest.fixture(scope="module", autouse=True)
def device():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    H.init(0)
    yield


@functools.lru_cache(maxsize=None)
def search(key, shed, grid, sibs=3, shard=0, nshards=1, split=0):
    """One launch under the given knobs: ((nodes, leaves, depth), shed counters, launch shape)."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    os.environ["HCLIB_HIP_NARROW_SHED"] = str(shed)
    os.environ["HCLIB_HIP_NARROW_SHED_SIBS"] = str(sibs)
    os.environ["HCLIB_HIP_SPIN_LIMIT_MS"] = "3000"  # a lost hand-off comes back as an error in 3 s, not 20
    if grid:
        os.environ["HCLIB_HIP_GRID"] = str(grid)
    else:
        os.environ.pop("HCLIB_HIP_GRID", None)
    try:
        r = H.uts(R.BY_KEY[key].args, shard, nshards, split)
        c = H.last_shed_counters()
        shape = H.uts_last_launch()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    print(f"{key} shed={shed} grid={grid} sibs={sibs} shard={shard}/{nshards}: {c} wpg={shape['workers_per_group']} "
          f"{r['kernel_ms']:.3f} ms")
    return (r["nodes"], r["leaves"], r["max_depth"]), c, shape


def _check_counters(c, shed, where):
    if not shed:
        assert all(v == 0 for v in c.values()), where
        return
    assert c["exits"] == c["placed"] + c["fallbacks"], where
    assert c["blocks"] >= c["placed"] and c["items"] >= c["blocks"], where
    assert c["items"] <= 64 * c["blocks"], where


@pytest.mark.parametrize("key", OVERFLOWING + QUIET)
def test_counts_exact_with_the_exit_on_and_off(key):
    want = R.serial(key)[0]
    for grid in GRIDS:
        for shed in (1, 0):
            counts, c, shape = search(key, shed, grid)
            where = (key, shed, grid, c, shape)
            assert counts == want, where
            assert shape["mode"] == "bin" and (not grid or (shape["grid"], shape["workers_per_group"]) == (4, 4)), where
            _check_counters(c, shed, where)
            if key in QUIET:
                # no level of these can outgrow a batch (m = 1: at most 64 children of 64 nodes)
                assert c["exits"] == 0 and c["blocks"] == 0, where


def test_shards_exact_with_the_exit_on_and_off():
    for s in range(2):
        want = R.serial_shard("bin_m3", s, 2, 1)[0]
        for grid in GRIDS:
            for shed in (1, 0):
                counts, c, shape = search("bin_m3", shed, grid, shard=s, nshards=2, split=1)
                assert counts == want, (s, shed, grid, c, shape)
                _check_counters(c, shed, (s, shed, grid, c, shape))


@pytest.mark.parametrize("rule", [2, 3])
def test_other_keep_rules_are_exact(rule):
    """Keep as many spawners as fit one batch (2), keep a quarter (3)."""
    for key in ("bin_m2", "bin_m7"):
        counts, c, shape = search(key, rule, 4)
        assert counts == R.serial(key)[0], (key, rule, c, shape)
        _check_counters(c, rule, (key, rule, c, shape))


def test_no_usable_sibling_falls_back_to_the_ring():
    """HCLIB_HIP_NARROW_SHED_SIBS=0: every overflow exit keeps its share and
    puts the rest onto the ring (the fallback of a lost claim or of no idle
    sibling, on every exit)."""
    counts, c, shape = search("bin_m4", 1, 4, sibs=0)
    assert counts == R.serial("bin_m4")[0], (c, shape)
    assert c["exits"] > 0 and c["fallbacks"] == c["exits"] and c["placed"] == c["blocks"] == c["items"] == 0, c


def test_both_outcomes_occur_on_four_waves():
    """Summed over the m >= 2 rows on one workgroup of four waves: some exits
    placed all their shed children with siblings, some fell back, and the two
    make up all exits. (A single row without an overflow is no failure.)"""
    tot = {"exits": 0, "placed": 0, "blocks": 0, "items": 0, "fallbacks": 0}
    for key in OVERFLOWING:
        _, c, _ = search(key, 1, 4)
        for k in tot:
            tot[k] += c[k]
    assert tot["placed"] > 0, tot
    assert tot["fallbacks"] > 0, tot
    assert tot["exits"] == tot["placed"] + tot["fallbacks"], tot
    assert tot["blocks"] >= tot["placed"] and tot["items"] > 0, tot
