"""The narrow loop's overflow exit in two LDS round trips
(include/hclib_hip/hx_sched.h narrow_shed, inbox_fill, inbox_take): the exit
reads its parked record and every box's flags at once, claims a box with the
block's carry slots already on their way, writes 16-byte items, and the taker
reads {state, n} and its item in one trip. None of that may change what a
search computes or counts, so every BIN row of tests/uts_ref.py that sheds
(m >= 2; bin_m1 never does) is searched whole on one workgroup (grid 4), on
two (grid 8: outbox blocks reach a deque and are taken by the other
workgroup) and on the default grid, under every keep rule
(HCLIB_HIP_NARROW_SHED 1, 2, 3), every cap on sibling blocks
(HCLIB_HIP_NARROW_SHED_SIBS 1, 2, 3) and with and without the hand-off wave's
outbox (HCLIB_HIP_UTS_COMM 0, 2), and with the exit off. Per launch: nodes,
leaves and depth equal the serial oracle's; exits = placed + fallbacks; items
are at most 64 a block; the outbox blocks equal the blocks passed to a deque
plus those passed to a sibling; with the exit off every counter is 0. Over the
whole set an outbox block and an exit that reached the ring occur.

A third condition, an exit that wrote more than one sibling block (blocks >
exits in some launch), was tried against the parent commit's library and
dropped: no launch of these rows produces it under either library. These
near-critical trees outgrow a batch by a spawner or two, so an exit sheds
less than one block's worth (at most 64 / m spawners) nearly every time, and
a whole launch cannot average more than one sibling block an exit.

Launches are 35,000 to 280,000 nodes each and run once (shared by the tests
below); a lost block comes back as an error in 3 s, not as a hang."""
import functools
import itertools
import os

import pytest

pytestmark = pytest.mark.gpu

import hclib_amd as H  # noqa: E402
from tests import uts_ref as R  # noqa: E402

ROWS = ["bin_m2", "bin_m3", "bin_m4", "bin_m6", "bin_m7", "bin_g3"]
GRIDS = [4, 8, 0]  # one workgroup of four; two; the default grid
RULES = [1, 2, 3]
SIBS = [1, 2, 3]
COMMS = [0, 2]
KNOBS = ("HCLIB_HIP_NARROW_SHED", "HCLIB_HIP_NARROW_SHED_SIBS", "HCLIB_HIP_UTS_COMM", "HCLIB_HIP_GRID",
         "HCLIB_HIP_SPIN_LIMIT_MS")
ON = list(itertools.product(GRIDS, RULES, SIBS, COMMS))


@pytest.fixture(scope="module", autouse=True)
def device():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    H.init(0)
    yield


@functools.lru_cache(maxsize=None)
def search(key, grid, rule, sibs, comm):
    """One launch under the given knobs: ((nodes, leaves, depth), shed counters, hand-off counters, launch shape)."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    os.environ["HCLIB_HIP_NARROW_SHED"] = str(rule)
    os.environ["HCLIB_HIP_NARROW_SHED_SIBS"] = str(sibs)
    os.environ["HCLIB_HIP_UTS_COMM"] = str(comm)
    os.environ["HCLIB_HIP_SPIN_LIMIT_MS"] = "3000"  # a lost hand-off comes back as an error in 3 s, not 20
    if grid:
        os.environ["HCLIB_HIP_GRID"] = str(grid)
    else:
        os.environ.pop("HCLIB_HIP_GRID", None)
    try:
        r = H.uts(R.BY_KEY[key].args)
        s = H.last_shed_counters()
        c = H.last_comm_counters()
        shape = H.uts_last_launch()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    print(f"{key} grid={grid} rule={rule} sibs={sibs} comm={comm}: shed {s} comm {c} {r['kernel_ms']:.3f} ms")
    return (r["nodes"], r["leaves"], r["max_depth"]), s, c, shape


@pytest.mark.parametrize("key", ROWS)
def test_every_setting_is_exact_and_its_counters_add_up(key):
    want = R.serial(key)[0]
    for grid, rule, sibs, comm in ON:
        counts, s, c, shape = search(key, grid, rule, sibs, comm)
        where = (key, grid, rule, sibs, comm, s, c, shape)
        assert counts == want, where
        assert shape["mode"] == "bin" and shape["workers_per_group"] == 4, where
        assert not grid or shape["grid"] == grid, where
        assert s["exits"] == s["placed"] + s["fallbacks"], where
        assert s["items"] <= 64 * s["blocks"], where
        assert s["blocks"] >= s["placed"], where  # a placed exit wrote at least one sibling block
        assert c["main_blocks"] + c["shed_blocks"] == c["to_deque"] + c["to_sibling"], where
        assert c["shed_items"] <= 64 * c["shed_blocks"], where
        if not comm:
            assert all(v == 0 for v in c.values()), where


@pytest.mark.parametrize("key", ROWS)
def test_every_counter_is_zero_with_the_exit_off(key):
    want = R.serial(key)[0]
    for grid in GRIDS:
        for comm in COMMS:
            counts, s, c, shape = search(key, grid, 0, 3, comm)
            where = (key, grid, comm, s, c, shape)
            assert counts == want, where
            assert all(v == 0 for v in s.values()), where
            assert all(v == 0 for v in c.values()), where  # bit 2 of the knob: the outbox has no other user


def _all_on():
    for key in ROWS:
        for grid, rule, sibs, comm in ON:
            yield (key, grid, rule, sibs, comm), search(key, grid, rule, sibs, comm)


def test_an_outbox_block_occurs():
    """Some exit had spawners left after the siblings and wrote them to an outbox."""
    hits = [(k, c) for k, (_, s, c, _) in _all_on() if c["shed_blocks"] > 0]
    print(f"launches with an outbox block: {len(hits)}")
    assert hits
    # ... and on two workgroups some of them went through a deque
    assert any(k[1] == 8 and c["to_deque"] > 0 for k, c in hits)


def test_an_exit_that_reached_the_ring_occurs():
    """Without the outbox every fallback goes onto the ring; with it the hand-off counters say which did."""
    hits = [k for k, (_, s, c, _) in _all_on() if (c["ring_exits"] if k[4] else s["fallbacks"]) > 0]
    print(f"launches with an exit that reached the ring: {len(hits)}")
    assert any(k[4] == 0 for k in hits)
    assert any(k[4] == 2 for k in hits)


def test_sibling_blocks_occur_under_every_cap():
    """Under every cap on an exit's sibling blocks some exit is placed in full.
    (Prints the launches with more sibling blocks than exits: see the module's
    docstring for why none is asserted.)"""
    for sibs in SIBS:
        assert any(s["blocks"] > 0 and s["placed"] > 0 for k, (_, s, _, _) in _all_on() if k[3] == sibs), sibs
    multi = [k for k, (_, s, _, _) in _all_on() if s["blocks"] > s["exits"]]
    print(f"launches with more sibling blocks than exits: {len(multi)} {multi[:4]}")
