"""Plain-Python restatement of BOTS Health (test/performance-regression/
full-apps/bots/health/health.ref.c) and the counts of the device task graph of
hclib_amd/csrc/health.hip.

simulate(params) gives the reference's full final state (tests/
test_health_host.py pins it to states recorded from the compiled reference):

  my_rand                    :88-100, on 32-bit words that wrap; the value is
                             (float)(1.0 / IM) = 2^-31 times (float)idum
  allocate_village           :143-195, villages in allocation order: a village,
                             then its children i = cities .. 1, each with its
                             whole subtree; the child list runs 1 .. cities
  check_patients_inside      :280-297
  check_patients_assess_par  :299-345; what the reference appends to the
                             parent's realloc list goes to the village's outbox
  check_patients_waiting     :347-369
  check_patients_realloc     :371-386, smallest id first
  check_patients_population  :388-407
  put_in_hosp                :409-424
  sim_village_par            :426-461; the children's rounds come first here,
                             which any schedule is equivalent to: a child's
                             round touches the parent only through its outbox
  get_results                :197-276

A village is a dict: id, level, personnel, free, and the lists of patient ids
population, waiting, assess, inside, in order. The patients' records are four
lists indexed by patient id. Both invariants the device layout rests on are
asserted in every round: free = personnel - |assess| - |inside|, and a village
never holds more than its subtree's population.

counts(params) is the task graph of health.hip: per round a CALL per village, a
scope, a POST and its wait node per village with children; a scope is opened
with children + 1 tasks checked in."""
import os
import struct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "health")

IA, IM, IQ, IR, MASK = 16807, 2147483647, 127773, 2836, 123459876
PARAM_KEYS = ("level", "cities", "population_ratio", "sim_time", "assess_time", "convalescence_time", "seed",
              "get_sick_p", "convalescence_p", "realloc_p")
TOTAL_KEYS = ("population", "hospitals", "personnel", "check_ins", "in_village", "waiting", "assess", "inside",
              "total_time")
LISTS = ("population", "waiting", "assess", "inside")

# the inputs of the issue's table: name -> the ten settings
INPUTS = {
    "A": (3, 4, 2, 40, 2, 6, 23, 0.4, 0.9, 0.4),
    "B": (2, 3, 3, 25, 1, 3, 7, 0.5, 0.9, 0.5),
    "D": (3, 3, 40, 30, 2, 4, 11, 0.1, 0.7, 0.3),
    "E": (4, 2, 20, 60, 3, 5, 5, 0.05, 0.6, 0.5),
    "F": (1, 4, 70, 20, 2, 3, 9, 0.3, 0.5, 0.5),
    "G": (5, 4, 20, 365, 4, 9, 1, 0.01, 0.5, 0.2),
}


def params(*values):
    return dict(zip(PARAM_KEYS, values))


def _i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x & 0x80000000 else x


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def my_rand(seed):
    """(the next seed, the draw): :88-100. The draw is exact in a double: one
    int -> float conversion (struct rounds to nearest even as the cast does) and
    a scaling by 2^-31."""
    idum = _i32(seed ^ MASK)
    k = abs(idum) // IQ * (1 if idum >= 0 else -1)  # C division truncates
    idum = _i32(IA * (idum - k * IQ) - IR * k)
    idum = _i32(idum ^ MASK)
    if idum < 0:
        idum += IM
    return _i32(idum * IM), _f32(float(idum)) * 2.0 ** -31


def build(p):
    """(villages in allocation order, records): allocate_village from the root,
    vid 0. A village also gets `children` (indices, in list order 1 .. cities),
    `parent` and `subtree` (its subtree's population)."""
    villages, rec = [], {"seed": [], "time": [], "time_left": [], "hosps_visited": []}

    def alloc(level, vid, parent):
        personnel = 2 ** level
        seed = _i32(vid * (IQ + p["seed"]))
        v = {"id": vid, "level": level, "personnel": personnel, "free": personnel, "parent": parent, "children": [],
             "population": [], "waiting": [], "assess": [], "inside": [], "outbox": []}
        me = len(villages)
        villages.append(v)
        for _ in range(personnel * p["population_ratio"]):
            v["population"].append(len(rec["seed"]))
            rec["seed"].append(seed)
            seed, _ = my_rand(seed)
            for k in ("time", "time_left", "hosps_visited"):
                rec[k].append(0)
        v["subtree"] = len(v["population"])
        if level > 1:
            for i in range(p["cities"], 0, -1):
                child = alloc(level - 1, _i32(vid * p["cities"] + i), me)
                v["children"].insert(0, child)
                v["subtree"] += villages[child]["subtree"]
        return me

    alloc(p["level"], 0, None)
    return villages, rec


def _put_in_hosp(p, v, rec, pid):
    rec["hosps_visited"][pid] += 1
    if v["free"] > 0:
        v["free"] -= 1
        v["assess"].append(pid)
        rec["time_left"][pid] = p["assess_time"]
        rec["time"][pid] += p["assess_time"]
    else:
        v["waiting"].append(pid)


def _first_phase(p, v, rec, is_root, conv_p, realloc_p):
    """steps 2-4 of a round: inside, assess, waiting"""
    for pid in list(v["inside"]):
        rec["time_left"][pid] -= 1
        if rec["time_left"][pid] == 0:
            v["free"] += 1
            v["inside"].remove(pid)
            v["population"].append(pid)
    v["outbox"] = []
    for pid in list(v["assess"]):
        rec["time_left"][pid] -= 1
        if rec["time_left"][pid] != 0:
            continue
        rec["seed"][pid], draw = my_rand(rec["seed"][pid])
        v["assess"].remove(pid)
        if draw < conv_p:
            rec["seed"][pid], draw = my_rand(rec["seed"][pid])
            if draw > realloc_p or is_root:
                v["inside"].append(pid)
                rec["time_left"][pid] = p["convalescence_time"]
                rec["time"][pid] += p["convalescence_time"]
            else:
                v["free"] += 1
                v["outbox"].append(pid)
        else:
            v["free"] += 1
            v["population"].append(pid)
    for pid in list(v["waiting"]):
        if v["free"] > 0:
            v["free"] -= 1
            rec["time_left"][pid] = p["assess_time"]
            rec["time"][pid] += p["assess_time"]
            v["waiting"].remove(pid)
            v["assess"].append(pid)
        else:
            rec["time"][pid] += 1


def _population(p, v, rec, sick_p):
    for pid in list(v["population"]):
        rec["seed"][pid], draw = my_rand(rec["seed"][pid])
        if draw < sick_p:
            v["population"].remove(pid)
            _put_in_hosp(p, v, rec, pid)


def simulate(p, merge="id", population_first=False):
    """The final state after sim_time rounds: (villages, records). merge="arrival"
    and population_first are the two wrong orders the host test shows to matter:
    the outboxes taken in the children's order instead of by id, and the walk of
    the population ahead of the reallocations."""
    villages, rec = build(p)
    sick_p, conv_p, realloc_p = (_f32(p[k]) for k in ("get_sick_p", "convalescence_p", "realloc_p"))

    def sim(x):
        v = villages[x]
        for c in v["children"]:
            sim(c)
        _first_phase(p, v, rec, v["level"] == p["level"], conv_p, realloc_p)
        arrived = [pid for c in v["children"] for pid in villages[c]["outbox"]]
        if population_first:
            _population(p, v, rec, sick_p)
        for pid in (sorted(arrived) if merge == "id" else arrived):
            _put_in_hosp(p, v, rec, pid)
        if not population_first:
            _population(p, v, rec, sick_p)

    for _ in range(p["sim_time"]):
        sim(0)
        for v in villages:
            assert v["free"] == v["personnel"] - len(v["assess"]) - len(v["inside"])
            assert len(v["outbox"]) <= v["personnel"]
            assert sum(len(v[k]) for k in LISTS) <= v["subtree"]
    return villages, rec


def totals(villages, rec):
    """get_results' nine sums (sums of integers: the reference adds each time
    and each visit count as a float to a long, the same number below 2^24)"""
    t = dict.fromkeys(TOTAL_KEYS, 0)
    for v in villages:
        t["hospitals"] += 1
        t["personnel"] += v["personnel"]
        for name, key in zip(LISTS, ("in_village", "waiting", "assess", "inside")):
            t[key] += len(v[name])
            t["population"] += len(v[name])
            t["check_ins"] += sum(rec["hosps_visited"][pid] for pid in v[name])
            t["total_time"] += sum(rec["time"][pid] for pid in v[name])
    return t


def state_words(villages, rec):
    """The state as the flat int32 words of a fixture file and of
    hclib_hip_health_state_t: villages, patients, then per village id, level,
    free_personnel and the four lengths, then seed, time, time_left and
    hosps_visited per patient, then the lists' ids, village by village."""
    out = [len(villages), len(rec["seed"])]
    for v in villages:
        out += [v["id"], v["level"], v["free"]] + [len(v[k]) for k in LISTS]
    for k in ("seed", "time", "time_left", "hosps_visited"):
        out += rec[k]
    for v in villages:
        for k in LISTS:
            out += v[k]
    return out


def fixture_words(name):
    raw = open(os.path.join(GOLDEN, name + ".state"), "rb").read()
    return list(struct.unpack("<%di" % (len(raw) // 4), raw))


def read_input(name):
    """(params, the nine expected fields) of tests/golden/health/<name>.input"""
    f = open(os.path.join(GOLDEN, name + ".input")).read().split()
    assert len(f) == 19
    p = params(*[int(x) for x in f[:7]], *[float(x) for x in f[7:10]])
    return p, [int(x) for x in f[10:18]] + [float(f[18])]


def counts(p):
    """What one launch of health.hip creates, exactly."""
    level, c, t = p["level"], p["cities"], p["sim_time"]
    villages = sum(c ** k for k in range(level))
    inner = sum(c ** k for k in range(level - 1))
    patients = sum(c ** (level - l) * 2 ** l * p["population_ratio"] for l in range(1, level + 1))
    return {"villages": villages, "patients": patients, "tasks": t * (villages + inner), "scopes": t * inner,
            "wait_nodes": t * inner, "check_ins": t * inner * (c + 1)}


def arena_bytes(p):
    """The bytes of health.hip's arena: three 256-byte counter lines, two
    8-word lines per village, four record words per patient, and per village of
    level l with a subtree population P(l) the segment of 2 P(l) + 3 * 2^l ids."""
    level, c, r = p["level"], p["cities"], p["population_ratio"]
    cnt = counts(p)
    sub, ids = 0, 0
    for l in range(1, level + 1):
        sub = c * sub + 2 ** l * r
        ids += c ** (level - l) * (2 * sub + 3 * 2 ** l)
    return 3 * 256 + 4 * (16 * cnt["villages"] + 4 * cnt["patients"] + ids)
