"""CPU-side checks of BOTS Health (hclib_hip_health*): the plain-Python
restatement of the reference (tests/health_ref.py) is pinned to full final
states recorded from the compiled reference, the library's host-side closed
forms (hclib_hip_health_bounds, what the launch allocates) equal the
restatement's counts, and the argument checks and exports work without a GPU.

The fixtures under tests/golden/health are the reference's own results.
health.ref.c and health.h were taken unchanged into a scratch program outside
this repository, with an empty app-desc.h, a bots.h that defines bots_message
(fprintf to stderr), bots_debug (nothing) and the two BOTS_RESULT_ values, and a
main that calls read_input_data, allocate_village(&top, NULL, NULL, sim_level,
0), sim_village_main_par(top) and get_results, compiled with `gcc -O3
-fno-toplevel-reorder` for baseline x86-64 without OpenMP, so that
sim_village_par runs serially. (-fno-toplevel-reorder keeps the globals in
source order: read_input_data reads the seed with %ld into an int32_t, and
the four bytes that spills over then land on sim_get_sick_p, which the same
fscanf fills next. Plain -O3 orders the globals the other way round and the
spill zeroes sim_convalescence_time. `gcc -O0` lays them out in source order too
and gives the same files.) <name>.state is the final state as little-endian
int32 words: villages, patients; per village in allocation order (a village,
then its children cities .. 1 with their subtrees) id, level, free_personnel and
the lengths of population, waiting, assess and inside; seed, time, time_left and
hosps_visited per patient id; then the four lists' ids, village by village.
<name>.input is the BOTS input file of the case: the ten settings and, from the
same run, the nine results that check_village prints. sha256:
  A.state        0c5b2ed574ab5aae057701cb36a816a75a2ff7cf22ba31486018a5c9899a20d0
  B.state        4c55a4d115516d732f1bad0f799ffce61d4e2e3f06ccec8b4971c305006705be
  D.state        30b92f3da9f756062f87504446ad28c446ee0ba1e79b9c228670313f955bca59
  E.state        b77cacd5c20b79b95fb730d92e3f38a3490b84c8e662b23ad4bf96080d4faa9b
  F.state        05bf564bb44e76e069ef0e9ba5b439772f7a04bc566e57b117db3956ca8ddc49
  chain.state    90d27a37a1b1ce675db52d8de38a7764aedcdd6329ac8d429d452d51135d5003
  negseed.state  eaf8067c7219069637d352e9955d86168a2ffdd56dfa47dd03732f6b99fb3cef
  A.input        8feef6547ed8f55139d10fe29345cfeff0bd42f7d3b7ec1463b2696a39ccbe03
  B.input        edc34ec0b1676c00cf7cd1677ac1211ce4abd97fcd2ebfaf73186fb96ca26dc0
  D.input        c6a6fa1196b2a84c53605850fc8ffae741b882bb9026b8e07ac268b67ac53ea7
  E.input        7c558ea455c27d0a279bb9db264de819cbaf9f37c6920286506d409f5fc0e064
  F.input        4b5b285452758a4c5600a7ae09f1259cab563f842914bee4efb338c90e2621df
  G.input        2fc56c71e83d3cb46ac58b3533656677819f5e396a47d4b0b28b65e836c74705
  chain.input    d55e2ac016c8a872dc9c5186f5d2328a724312296a4371510fd3e6bb396df5bb
  negseed.input  8cab36523ef5e7a8fb3d95c8f7081175065b24e57f9fd1fefb380a26c9a11af5"""
import ctypes as C
import hashlib
import math
import os

import pytest

import hclib_amd as H
from tests import health_ref as R

SHA256 = {
    "A.state": "0c5b2ed574ab5aae057701cb36a816a75a2ff7cf22ba31486018a5c9899a20d0",
    "B.state": "4c55a4d115516d732f1bad0f799ffce61d4e2e3f06ccec8b4971c305006705be",
    "D.state": "30b92f3da9f756062f87504446ad28c446ee0ba1e79b9c228670313f955bca59",
    "E.state": "b77cacd5c20b79b95fb730d92e3f38a3490b84c8e662b23ad4bf96080d4faa9b",
    "F.state": "05bf564bb44e76e069ef0e9ba5b439772f7a04bc566e57b117db3956ca8ddc49",
    "chain.state": "90d27a37a1b1ce675db52d8de38a7764aedcdd6329ac8d429d452d51135d5003",
    "negseed.state": "eaf8067c7219069637d352e9955d86168a2ffdd56dfa47dd03732f6b99fb3cef",
    "A.input": "8feef6547ed8f55139d10fe29345cfeff0bd42f7d3b7ec1463b2696a39ccbe03",
    "B.input": "edc34ec0b1676c00cf7cd1677ac1211ce4abd97fcd2ebfaf73186fb96ca26dc0",
    "D.input": "c6a6fa1196b2a84c53605850fc8ffae741b882bb9026b8e07ac268b67ac53ea7",
    "E.input": "7c558ea455c27d0a279bb9db264de819cbaf9f37c6920286506d409f5fc0e064",
    "F.input": "4b5b285452758a4c5600a7ae09f1259cab563f842914bee4efb338c90e2621df",
    "G.input": "2fc56c71e83d3cb46ac58b3533656677819f5e396a47d4b0b28b65e836c74705",
    "chain.input": "d55e2ac016c8a872dc9c5186f5d2328a724312296a4371510fd3e6bb396df5bb",
    "negseed.input": "8cab36523ef5e7a8fb3d95c8f7081175065b24e57f9fd1fefb380a26c9a11af5",
}
STATES = sorted(k[:-6] for k in SHA256 if k.endswith(".state"))
# the issue's table: personnel, check-ins, in village, waiting, assess, inside, total time
TABLE = {"A": (56, 392, 3, 79, 6, 24, 3876), "B": (10, 86, 2, 20, 5, 3, 627), "D": (38, 1652, 126, 1356, 20, 18, 30286),
         "E": (64, 1778, 298, 918, 48, 16, 43720), "F": (2, 149, 2, 136, 1, 1, 2357)}
# (villages, patients) of the table
SIZES = {"A": (21, 112), "B": (4, 30), "D": (13, 1520), "E": (15, 1280), "F": (1, 140), "G": (341, 19840)}

_simulated = {}


def _simulate(name):
    """the restatement's final state of a fixture's input, computed once"""
    if name not in _simulated:
        p, _ = R.read_input(name)
        _simulated[name] = (p,) + R.simulate(p)
    return _simulated[name]


@pytest.mark.parametrize("name", sorted(SHA256))
def test_fixtures_are_the_recorded_files(name):
    raw = open(os.path.join(R.GOLDEN, name), "rb").read()
    assert hashlib.sha256(raw).hexdigest() == SHA256[name]


@pytest.mark.parametrize("name", sorted(R.INPUTS))
def test_input_files_hold_the_table_s_settings(name):
    p, expected = R.read_input(name)
    assert p == R.params(*R.INPUTS[name])
    assert tuple(expected[:2]) == (SIZES[name][1], SIZES[name][0])
    if name == "G":
        assert expected[:8] == [19840, 341, 992, 46556, 9009, 10055, 417, 359]
        assert round(expected[8] * 19840) == 3019106


@pytest.mark.parametrize("name", STATES)
def test_restatement_reproduces_the_reference_state(name):
    p, villages, rec = _simulate(name)
    want = R.fixture_words(name)
    assert R.state_words(villages, rec) == want
    assert len(want) == 2 + 7 * want[0] + 5 * want[1]
    # and the totals are the input file's expected results
    t = R.totals(villages, rec)
    _, expected = R.read_input(name)
    assert [t[k] for k in R.TOTAL_KEYS[:8]] == expected[:8]
    assert abs(t["total_time"] / t["population"] - expected[8]) < 1e-4
    if name in TABLE:
        assert (t["personnel"], t["check_ins"], t["in_village"], t["waiting"], t["assess"], t["inside"],
                t["total_time"]) == TABLE[name]


def test_the_pinned_states_reach_what_the_table_says():
    """A: patients end away from home; D and E: lists longer than one chunk of 64"""
    for name, migrated, longest in (("A", 71, 0), ("D", 51, 300), ("E", 183, 341)):
        p, villages, rec = _simulate(name)
        home, first = {}, 0
        for v in villages:  # a village's own patients are numbered consecutively, in allocation order
            n = v["personnel"] * p["population_ratio"]
            home.update((pid, v["id"]) for pid in range(first, first + n))
            first += n
        away = sum(1 for v in villages for k in R.LISTS for pid in v[k] if home[pid] != v["id"])
        assert away == migrated
        assert max(len(v[k]) for v in villages for k in R.LISTS) >= longest


def test_the_order_of_the_merge_and_of_the_two_phases_is_pinned():
    """Taking the children's patients in arrival order, or walking the
    population ahead of them, gives another final state: the fixtures tell."""
    changed = {"arrival": [], "population_first": []}
    for name in ("A", "D", "E"):
        p, villages, rec = _simulate(name)
        want = R.state_words(villages, rec)
        if R.state_words(*R.simulate(p, merge="arrival")) != want:
            changed["arrival"].append(name)
        if R.state_words(*R.simulate(p, population_first=True)) != want:
            changed["population_first"].append(name)
    assert changed["arrival"] and changed["population_first"], changed


def test_my_rand_wraps_and_scales():
    # the first draw of seed 0: idum = MASK, k = 966, ...; the value is below 1 and a multiple of 2^-31 * 2^k
    s, d = R.my_rand(0)
    assert -2 ** 31 <= s < 2 ** 31 and 0.0 <= d < 1.0
    s2, d2 = R.my_rand(-123456789)  # a negative seed: C division truncates towards zero
    assert -2 ** 31 <= s2 < 2 ** 31 and 0.0 <= d2 <= 1.0
    # a patient's seed of village 1 with sim_seed 23 is the village seed, 1 * (IQ + 23)
    _, rec = R.build(R.params(*R.INPUTS["B"]))
    assert rec["seed"][0] == 0 and rec["seed"][2 ** 2 * 3] == 3 * (R.IQ + 7)


@pytest.mark.parametrize("name", sorted(R.INPUTS))
def test_bounds_equal_the_restatement(name):
    p = R.params(*R.INPUTS[name])
    want = R.counts(p)
    got = H.health_bounds(p)
    assert (got["villages"], got["patients"]) == SIZES[name]
    assert {k: got[k] for k in ("villages", "patients", "tasks", "scopes", "wait_nodes")} == \
        {k: want[k] for k in ("villages", "patients", "tasks", "scopes", "wait_nodes")}
    assert got["arena_bytes"] == R.arena_bytes(p)


def test_bounds_of_other_shapes():
    for values in ((4, 1, 5, 30, 2, 3, 3, 0.3, 0.8, 0.6), (2, 3, 4, 30, 2, 3, -77, 0.3, 0.8, 0.6),
                   (3, 4, 2, 0, 2, 6, 23, 0.4, 0.9, 0.4), (2, 70, 1, 3, 1, 1, 0, 0.0, 1.0, 1.0)):
        p = R.params(*values)
        want, got = R.counts(p), H.health_bounds(p)
        assert all(got[k] == want[k] for k in ("villages", "patients", "tasks", "scopes", "wait_nodes"))
        assert got["arena_bytes"] == R.arena_bytes(p)
    # sim_time = 0 creates nothing
    assert H.health_bounds(R.params(3, 4, 2, 0, 2, 6, 23, 0.4, 0.9, 0.4))["tasks"] == 0
    # the built tree has the counted villages and patients
    villages, rec = R.build(R.params(4, 1, 5, 30, 2, 3, 3, 0.3, 0.8, 0.6))
    assert (len(villages), len(rec["seed"])) == (4, 150)


GOOD = dict(level=3, cities=4, population_ratio=2, sim_time=40, assess_time=2, convalescence_time=6, seed=23,
            get_sick_p=0.4, convalescence_p=0.9, realloc_p=0.4)


@pytest.mark.parametrize("change,word", [
    ({"level": 0}, "level"), ({"level": -1}, "level"), ({"cities": 0}, "cities"), ({"population_ratio": 0}, "ratio"),
    ({"sim_time": -1}, "sim_time"), ({"assess_time": 0}, "assess_time"), ({"convalescence_time": 0}, "assess_time"),
    ({"get_sick_p": -0.1}, "probability 0"), ({"get_sick_p": 1.5}, "probability 0"),
    ({"get_sick_p": math.nan}, "probability 0"), ({"convalescence_p": 1.01}, "probability 1"),
    ({"convalescence_p": math.nan}, "probability 1"), ({"realloc_p": -1e-9}, "probability 2"),
    ({"realloc_p": math.inf}, "probability 2"),
    ({"level": 12, "cities": 2}, "LDS"),           # 2 * 2^11 = 4096 patients could reach the root in one round
    ({"level": 2, "cities": 1025}, "LDS"),         # 1025 * 2
    ({"level": 25, "cities": 1}, "32-bit"),        # deeper than the layout numbers
    ({"level": 6, "cities": 64}, "32-bit"),        # 64^5 villages at the bottom: their patients
    ({"population_ratio": 2 ** 29}, "32-bit"),     # patients
    ({"level": 4, "cities": 16, "sim_time": 2 ** 20}, "32-bit"),  # tasks: pool counts grow with sim_time
])
def test_argument_errors_are_einval_without_a_device(change, word):
    p = H._health_params(dict(GOOD, **change))
    r = H.HealthResult()
    assert H.lib().hclib_hip_health(C.byref(p), C.byref(r), None) == -2  # HCLIB_HIP_EINVAL
    assert word in H.lib().hclib_hip_last_error().decode()
    out = (C.c_uint64 * 6)()
    assert H.lib().hclib_hip_health_bounds(C.byref(p), out) == -2
    assert word in H.lib().hclib_hip_last_error().decode()


def test_null_pointers_are_einval():
    p = H._health_params(GOOD)
    r = H.HealthResult()
    out = (C.c_uint64 * 6)()
    assert H.lib().hclib_hip_health(None, C.byref(r), None) == -2
    assert "NULL" in H.lib().hclib_hip_last_error().decode()
    assert H.lib().hclib_hip_health(C.byref(p), None, None) == -2
    assert H.lib().hclib_hip_health_bounds(None, out) == -2
    assert H.lib().hclib_hip_health_bounds(C.byref(p), None) == -2
    st = H.HealthState()  # every array NULL
    assert H.lib().hclib_hip_health(C.byref(p), C.byref(r), C.byref(st)) == -2
    assert "state" in H.lib().hclib_hip_last_error().decode()


def test_limits_are_inclusive():
    # the largest merge that fits: 2048 ids
    assert H.health_bounds(dict(GOOD, level=11, cities=2, population_ratio=1, sim_time=1))["villages"] == 2 ** 11 - 1
    assert H.health_bounds(dict(GOOD, level=2, cities=1024))["villages"] == 1025
    assert H.health_bounds(dict(GOOD, level=12, cities=1, population_ratio=1))["villages"] == 12
    # probabilities of exactly 0 and 1 are valid
    assert H.health_bounds(dict(GOOD, get_sick_p=0.0, convalescence_p=1.0, realloc_p=1.0))["patients"] == 112


def test_read_input_and_the_python_wrapper():
    p, expected = H.health_read_input(os.path.join(R.GOLDEN, "A.input"))
    assert p == dict(GOOD) and expected["hosps_visited"] == 392 and expected["population"] == 112
    assert abs(expected["avg_stay"] - 3876 / 112) < 1e-5
    assert tuple(p) == H.HEALTH_PARAMS
    # the seed is the low 32 bits of the file's number
    assert H._health_params(dict(GOOD, seed=2 ** 32 + 5)).seed == 5
    assert H._health_params(dict(GOOD, seed=2 ** 31)).seed == -2 ** 31
    assert H._health_params(tuple(GOOD.values())).cities == 4
    with pytest.raises(ValueError):
        H.health_bounds({"level": 3})
    with pytest.raises(H.HclibError, match=r"\(-2\)"):
        H.health_bounds(dict(GOOD, cities=0))


def test_library_exports_health():
    for sym in ("hclib_hip_health", "hclib_hip_health_bounds", "hclib_hip_health_last_ticks"):
        assert hasattr(H.lib(), sym) and sym in H.EXPORTS_HIP
    assert C.sizeof(H.HealthParams) == 40 and C.sizeof(H.HealthResult) == 17 * 8


def test_valid_arguments_fail_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for sim_time in (40, 0):
        with pytest.raises(H.HclibError) as e:
            H.health(dict(GOOD, sim_time=sim_time))
        assert "(-1)" in str(e.value)  # HCLIB_HIP_ENODEV
