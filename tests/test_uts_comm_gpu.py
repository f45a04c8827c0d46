"""The hand-off wave of a BIN workgroup (include/hclib_hip/hx_sched.h comm_wave;
HCLIB_HIP_UTS_COMM, bits 1 the give-away loop's outbox put, 2 narrow_shed's,
4 the wave's redirect to a sibling gone idle): a fifth wave that takes blocks
from the workers' outboxes and passes them on to a sibling or the HBM deques.
Every BIN row of tests/uts_ref.py the narrow-shed test runs is searched whole
with the knob at 0, 1, 2, 3 and 7, in workgroups of four and of two workers,
on the default grid, on one workgroup (grid 4) and on two (grid 8: deque
chunks change workgroup); bin_m3 also in two shards; and with the sibling
inboxes of the overflow exit capped at none, so that every shed child goes
through the outbox or the ring. Every launch's (nodes, leaves, depth) equals
the serial oracle's. The hand-off counters (hclib_hip_last_comm_counters) are
all 0 with the knob 0, outbox blocks equal the blocks passed on, items are at
most 64 a block, and over the m >= 2 rows on one workgroup both users of the
outbox have fired. Launches are a few hundred to 300,000 nodes each and run
once (shared by the tests below)."""
import functools
import os

import pytest

pytestmark = pytest.mark.gpu

import hclib_amd as H  # noqa: E402
from tests import uts_ref as R  # noqa: E402

OVERFLOWING = ["bin_m2", "bin_m3", "bin_m4", "bin_m6", "bin_m7", "bin_g3"]  # m >= 2: levels can outgrow a batch
QUIET = ["one_bin", "bin_b2_5", "bin_m1"]  # no children, a 7-node tree, m = 1
GRIDS = [0, 4, 8]  # the default grid; one workgroup of four; two (or, in pairs, two and four)
COMMS = [0, 1, 2, 3, 7]
WPGS = [4, 2]
KNOBS = ("HCLIB_HIP_UTS_COMM", "HCLIB_HIP_WPG", "HCLIB_HIP_NARROW_SHED_SIBS", "HCLIB_HIP_GRID",
         "HCLIB_HIP_SPIN_LIMIT_MS")


@pytest.fixture(scope="module", autouse=True)
def device():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    H.init(0)
    yield


@functools.lru_cache(maxsize=None)
def search(key, comm, grid, wpg=4, sibs=3, shard=0, nshards=1, split=0):
    """One launch under the given knobs: ((nodes, leaves, depth), comm counters, shed counters, launch shape)."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    os.environ["HCLIB_HIP_UTS_COMM"] = str(comm)
    os.environ["HCLIB_HIP_WPG"] = str(wpg)
    os.environ["HCLIB_HIP_NARROW_SHED_SIBS"] = str(sibs)
    os.environ["HCLIB_HIP_SPIN_LIMIT_MS"] = "3000"  # a lost hand-off comes back as an error in 3 s, not 20
    if grid:
        os.environ["HCLIB_HIP_GRID"] = str(grid)
    else:
        os.environ.pop("HCLIB_HIP_GRID", None)
    try:
        r = H.uts(R.BY_KEY[key].args, shard, nshards, split)
        c = H.last_comm_counters()
        s = H.last_shed_counters()
        shape = H.uts_last_launch()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    print(f"{key} comm={comm} grid={grid} wpg={wpg} sibs={sibs} shard={shard}/{nshards}: {c} shed {s} "
          f"{r['kernel_ms']:.3f} ms")
    return (r["nodes"], r["leaves"], r["max_depth"]), c, s, shape


def _check_counters(c, comm, where):
    if not comm:
        assert all(v == 0 for v in c.values()), where
        return
    assert c["main_blocks"] + c["shed_blocks"] == c["to_deque"] + c["to_sibling"], where
    assert c["main_blocks"] <= c["main_items"] <= 64 * c["main_blocks"], where
    assert c["shed_blocks"] <= c["shed_items"] <= 64 * c["shed_blocks"], where
    if not comm & 1:
        assert c["main_blocks"] == 0, where
    if not comm & 2:
        assert c["shed_blocks"] == 0, where
    if not comm & 4:
        assert c["to_sibling"] == 0, where


@pytest.mark.parametrize("key", OVERFLOWING + QUIET)
def test_counts_exact_under_every_setting(key):
    want = R.serial(key)[0]
    for wpg in WPGS:
        for grid in GRIDS:
            for comm in COMMS:
                counts, c, s, shape = search(key, comm, grid, wpg)
                where = (key, comm, grid, wpg, c, s, shape)
                assert counts == want, where
                assert shape["mode"] == "bin" and shape["workers_per_group"] == wpg, where
                assert not grid or shape["grid"] == grid, where  # the grid counts worker waves only
                _check_counters(c, comm, where)
                assert s["exits"] == s["placed"] + s["fallbacks"], where
                if key in QUIET:
                    assert c["shed_blocks"] == 0 and c["ring_exits"] == 0, where


def test_shards_exact_with_the_wave_on_and_off():
    for sh in range(2):
        want = R.serial_shard("bin_m3", sh, 2, 1)[0]
        for grid in GRIDS:
            for comm in COMMS:
                counts, c, s, shape = search("bin_m3", comm, grid, shard=sh, nshards=2, split=1)
                assert counts == want, (sh, comm, grid, c, shape)
                _check_counters(c, comm, (sh, comm, grid, c, shape))


@pytest.mark.parametrize("comm", [2, 3, 7])
def test_no_sibling_inbox_sends_the_shed_children_to_the_outbox(comm):
    """HCLIB_HIP_NARROW_SHED_SIBS=0 with the wave on: the sibling path places
    nothing (every exit is a fallback by the shed counters, which describe
    that path alone), the outbox takes what it can and the ring the rest."""
    for key in ("bin_m4", "bin_m7"):
        counts, c, s, shape = search(key, comm, 4, sibs=0)
        assert counts == R.serial(key)[0], (key, c, s, shape)
        _check_counters(c, comm, (key, c, s))
        assert s["exits"] > 0 and s["fallbacks"] == s["exits"] and s["placed"] == s["blocks"] == s["items"] == 0, s
        assert c["shed_blocks"] > 0, c
        assert c["ring_exits"] <= s["exits"], (c, s)


def test_the_shed_counters_keep_describing_the_sibling_path():
    """With the wave on, placed / blocks / items count sibling inboxes only
    and every exit is still either placed or a fallback."""
    for key in OVERFLOWING:
        for comm in (3, 7):
            _, c, s, _ = search(key, comm, 4)
            assert s["exits"] == s["placed"] + s["fallbacks"], (key, s)
            assert s["blocks"] >= s["placed"] and s["items"] <= 64 * s["blocks"], (key, s)
            assert c["ring_exits"] <= s["fallbacks"], (key, c, s)


def test_both_users_fire_on_one_workgroup():
    """Summed over the m >= 2 rows on one workgroup of four workers, with both
    users on: the give-away loop and the overflow exit have each filled
    outboxes, and every block was passed on."""
    tot = dict.fromkeys(("main_blocks", "main_items", "shed_blocks", "shed_items", "to_deque", "to_sibling", "busy",
                         "ring_exits"), 0)
    for key in OVERFLOWING:
        _, c, _, _ = search(key, 3, 4)
        for k in tot:
            tot[k] += c[k]
    assert tot["main_blocks"] > 0 and tot["main_items"] > 0, tot
    assert tot["shed_blocks"] > 0 and tot["shed_items"] > 0, tot
    assert tot["main_blocks"] + tot["shed_blocks"] == tot["to_deque"] + tot["to_sibling"], tot
