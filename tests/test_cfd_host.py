"""CPU-side checks of Rodinia CFD (hclib_hip_cfd*): the numpy restatement
(tests/cfd_ref.py) writes, for every fixture, the three text files the compiled
reference wrote, byte for byte, and stays finite; the fixtures are the recorded
files and have the shapes their names promise; the library's reader equals the
restatement's on every array, bit for bit; hclib_hip_cfd_bounds equals an
enumeration in Python; every refusal is EINVAL, with its message, before a
device is looked for. No GPU."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import hclib_amd as H
from tests import cfd_ref as R

ENODEV, EINVAL = -1, -2  # HCLIB_HIP_ENODEV, HCLIB_HIP_EINVAL (include/hclib_hip.h)
KINDS = ("txt", "density", "momentum", "density_energy")
SHA256 = {
    "tiny": ("5779bc25c6589567e617d6317834985dbee90991fc8eaaf8072ebf9b51f30477",
             "eb719bb7e71aec126f35b3d42b6ecc53d4e7e67be76c7bf7ddb13a6d99a834b1",
             "4fabcea2c027e44f5a34b331f60099679da3e528d284af186a2c64078ad04182",
             "478b09f424342adaee08cfed7220f9ff9b7f572706c0acc9dbc4a865ef6fc6de"),
    "pad1": ("97c4d4a0c40e42d02b549800deddedd8e16e94c798342601a6b953f7c85dbb4d",
             "598e0f5094d17c6173838dba8a19052f7dc59de37859d7cd126dc1eee4af0f1f",
             "868eb6191fedcdba5847e448d6a3cf3478ab6e1273c515c22ab843bc3c634229",
             "9d39396f49dfc737e346f2931ccfdaa87de316005c0aa2276abf1ee7928a8db7"),
    "grid": ("2b6ee687dc6e63a9e84788014299b1b935ae0b04a0bb0cf2dfadcb43b9eeb2b6",
             "4035d7027f2d20a5d43c71d0e88d0b17eac9a45268321c15526163bd259e9cc7",
             "507cd7bee2269568ee841f2451270c198509682e06ecc803e1afc155d927bae4",
             "714c1dfffeb5ac03173d05e9283c648a225e4ccfe9e4417ab02aed6cf2aae1a0"),
    "hub": ("b5598c3350b40292bcfbff00f822d0e41e92969f20f1537b4cc2be20ffea8c7c",
            "7c0b1e987a5990e59583bf1597537f55c2190db36edf2473ff893499f9c29839",
            "ac6cb0b340d82e4d333dd179e5f4de8065ece74f10301f659c54e215ac850e29",
            "f3d0ba848b741ce4d48a4c726946a1e8eac68f07d05b8e0b9731ae68b69d1cc6"),
    "odd": ("313b7ccaf92be355c965f96e2401404e2944e80b4923c6fe81eac752d35bfe3f",
            "a1d1db954a13a7b7c07d40414ddf40d352092e49d591a523b8a155d564c3f386",
            "7177ba04269f143f3682d47bd90e004ed7272511924906156cf880f50d92aab0",
            "df59e3fbf9904d84f8d773a31e1dd77b8b28afac67b9f8611bc7269531021292"),
}


def _text(name, kind):
    with open(R.fixture_path(name, kind)) as f:
        return f.read()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixtures_are_the_recorded_files(name):
    got = tuple(hashlib.sha256(_text(name, k).encode()).hexdigest() for k in KINDS)
    assert got == SHA256[name]
    # and the input is what the generator writes
    assert R.mesh_text(R.MAKERS[name]()) == _text(name, "txt")


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_writes_the_reference_files_byte_for_byte(name):
    m = R.read_input(R.fixture_path(name))
    v = R.run(m)
    assert np.isfinite(v).all()
    text = R.dump(v, m["nel"], m["nelr"])
    for kind in KINDS[1:]:
        assert text[kind] == _text(name, kind), (name, kind)
    # the iteration has moved: four iterations print other numbers
    assert R.dump(R.run(m, 4), m["nel"], m["nelr"])["density"] != text["density"]


def test_two_then_three_iterations_are_five():
    m = R.read_input(R.fixture_path("grid"))
    assert np.array_equal(_bits(R.run(m, 3, R.run(m, 2))), _bits(R.run(m, 5)))


def test_fixture_shapes():
    t = R.read_input(R.fixture_path("tiny"))
    assert (t["nel"], t["nelr"]) == (5, 8) and (t["neighbours"][5:] == t["neighbours"][4]).all()
    raw = [int(row.split()[k]) for row in _text("tiny", "txt").splitlines()[1:] for k in (1, 5, 9, 13)]
    assert 0 in raw and -1 in raw and -3 in raw  # the wing; the far field written two ways
    assert (t["neighbours"] == -1).sum() == 1 and set(t["neighbours"][:, 2]) == {-2}
    p = R.read_input(R.fixture_path("pad1"))
    assert (p["nel"], p["nelr"]) == (9, 16)
    g = R.read_input(R.fixture_path("grid"))
    assert g["nel"] == g["nelr"] == 1000 and (g["neighbours"] == -1).any() and (g["neighbours"] == -2).any()
    h = R.read_input(R.fixture_path("hub"))
    nb = h["neighbours"]
    assert h["nelr"] // 8 >= 67 and (nb[:8][nb[:8] >= 0] < 8).all()  # block 0 names no other block
    assert all(((nb[8 * b:8 * b + 8] >= 0) & (nb[8 * b:8 * b + 8] < 8)).any() for b in range(1, h["nelr"] // 8))
    o = R.read_input(R.fixture_path("odd"))
    nb = o["neighbours"]
    assert (o["nel"], o["nelr"]) == (13, 16) and 2 in nb[2] and (nb[4] == 7).sum() == 2 and (nb[6] < 0).all()
    assert ((nb[:13] >= 13) & (nb[:13] < 16)).any()


@pytest.mark.parametrize("name", R.FIXTURES)
def test_reader_equals_the_restatement(name):
    got, want = H.cfd_read_input(R.fixture_path(name)), R.read_input(R.fixture_path(name))
    assert (got["nel"], got["nelr"]) == (want["nel"], want["nelr"])
    assert np.array_equal(_bits(got["areas"]), _bits(want["areas"]))
    assert np.array_equal(_bits(got["normals"]), _bits(want["normals"]))
    assert got["neighbours"].dtype == np.int32 and np.array_equal(got["neighbours"], want["neighbours"])


def test_reader_refuses(tmp_path):
    good = _text("tiny", "txt")
    cases = {"missing": None, "empty": "", "word": "five\n", "zero": "0\n", "negative": "-4\n",
             "truncated": good[:len(good) // 2], "cut_row": "\n".join(good.splitlines()[:-1]) + "\n",
             "letters": good.replace(good.split()[7], "abc", 1), "short_last": good.rstrip().rsplit(" ", 1)[0] + "\n"}
    words = {"missing": "cannot open", "empty": "no element count", "word": "no element count", "zero": "at least 1",
             "negative": "at least 1"}
    for key, text in cases.items():
        path = tmp_path / (key + ".txt")
        if text is not None:
            path.write_text(text)
        with pytest.raises(H.HclibError) as e:
            H.cfd_read_input(str(path))
        assert "(%d)" % EINVAL in str(e.value) and words.get(key, "truncated or not a number") in str(e.value), key
    assert H.lib().hclib_hip_cfd_read_input(R.fixture_path("tiny").encode(), None, None, None, None) == EINVAL
    # the second call's arrays are sized by the first: another count is refused
    counts = (C.c_int64 * 2)(4, 8)
    a = np.zeros(8 * 12)
    assert H.lib().hclib_hip_cfd_read_input(R.fixture_path("tiny").encode(), a.ctypes.data, a.ctypes.data, a.ctypes.data,
                                            counts) == EINVAL
    assert b"differs" in H.lib().hclib_hip_last_error()


def enumerate_bounds(mesh, iterations, block):
    """hclib_hip_cfd_bounds from the definitions: the tasks one by one"""
    nelr, nb = mesh["nelr"], mesh["neighbours"]
    block = block or 256
    nblocks = -(-nelr // block)
    reads = [set() for _ in range(nblocks)]
    for i in range(nelr):
        reads[i // block].add(i // block)
        for k in nb[i]:
            if k >= 0:
                reads[i // block].add(int(k) // block)
    hood = [set(r) for r in reads]
    for b, r in enumerate(reads):
        for o in r:
            hood[o].add(b)
    tasks = awaits = moved = 0
    waiters = {}
    for s in range(3 * iterations):
        for b in range(nblocks):
            tasks += 1
            if s:
                awaits += len(hood[b])
                for o in hood[b]:
                    waiters[(s - 1, o)] = waiters.get((s - 1, o), 0) + 1
            for i in range(b * block, min((b + 1) * block, nelr)):
                moved += 40 + 40 + 16 + 96 + 40 * int((nb[i] >= 0).sum()) + (8 + 48 if s % 3 == 0 else 48)
    up = lambda x: (x + 255) // 256 * 256  # noqa: E731
    arena = up(8 * nelr) + up(16 * nelr) + up(96 * nelr) + 3 * 5 * up(8 * nelr) + up(8 * nelr)
    return {"tasks": tasks, "awaits": awaits, "stages": 3 * iterations, "max_waiters": max(waiters.values(), default=0),
            "arena_bytes": arena, "bytes_moved": moved}


@pytest.mark.parametrize("name", R.FIXTURES)
def test_bounds_equal_the_enumeration(name):
    m = R.read_input(R.fixture_path(name))
    for block in (8, 24, 64, 256, 0, 1024):
        for iterations in (0, 1, 2, 5):
            assert H.cfd_bounds(m, iterations, block) == enumerate_bounds(m, iterations, block), (block, iterations)
    assert H.cfd_bounds(R.fixture_path(name), 5, 8) == H.cfd_bounds(m, 5, 8)


def test_hub_has_a_waiter_list_above_64():
    m = R.read_input(R.fixture_path("hub"))
    assert H.cfd_bounds(m, 5, 8)["max_waiters"] == m["nelr"] // 8 > 64


def test_every_refusal_is_einval_without_a_device():
    lib = H.lib()
    m = R.read_input(R.fixture_path("grid"))
    ar, nb, nr = m["areas"], m["neighbours"].copy(), m["normals"]
    out = np.zeros((m["nelr"], 5))
    out6 = (C.c_uint64 * 6)()
    res = H.CfdResult()

    def run(nel, iterations, block, form, areas=ar, nbs=nb, normals=nr, variables=out):
        p = [None if x is None else x.ctypes.data for x in (areas, nbs, normals, variables)]
        return lib.hclib_hip_cfd(nel, p[0], p[1], p[2], None, iterations, block, form, p[3], C.byref(res))

    def both(nel, iterations, block, word, nbs=nb):
        assert lib.hclib_hip_cfd_bounds(nel, nbs.ctypes.data, iterations, block, out6) == EINVAL
        assert word in lib.hclib_hip_last_error(), lib.hclib_hip_last_error()
        assert run(nel, iterations, block, 0, nbs=nbs) == EINVAL
        assert word in lib.hclib_hip_last_error(), lib.hclib_hip_last_error()

    for nel in (0, -1, -1000):
        both(nel, 5, 8, b"nel must be at least 1")
    both(2 ** 31 - 1, 5, 8, b"int indices")
    both(1000, -1, 8, b"iterations must not be negative")
    for block in (-8, 4, 12, 100, 1032, 2048):
        both(1000, 5, block, b"not a multiple of 8 in [8, 1024]")
    for form in (-1, 2, 7):
        assert run(1000, 5, 8, form) == EINVAL and b"unknown form" in lib.hclib_hip_last_error()
    # a neighbour index: nelr is outside, and so is one past the padding of a mesh of 997 (nelr 1000)
    bad = nb.copy()
    bad[17, 2] = 1000
    both(1000, 5, 8, b"names element 1000 of 1000", nbs=bad)
    both(997, 5, 8, b"names element 1000 of 1000", nbs=bad)
    bad[17, 2] = 999  # in [nel, nelr): a padded copy
    assert lib.hclib_hip_cfd_bounds(997, bad.ctypes.data, 5, 8, out6) == 0
    # the task count: 125 blocks, 3 stages an iteration
    assert lib.hclib_hip_cfd_bounds(1000, nb.ctypes.data, 178956, 8, out6) == 0 and out6[0] == 3 * 178956 * 125
    both(1000, 178957, 8, b"tasks")
    # NULL pointers
    for k in ("areas", "nbs", "normals", "variables"):
        assert run(1000, 5, 8, 0, **{k: None}) == EINVAL and b"NULL" in lib.hclib_hip_last_error()
    assert lib.hclib_hip_cfd_bounds(1000, None, 5, 8, out6) == EINVAL
    assert lib.hclib_hip_cfd_bounds(1000, nb.ctypes.data, 5, 8, None) == EINVAL
    # the binding's own checks
    with pytest.raises(ValueError):
        H.cfd(m, form="levels")
    with pytest.raises(ValueError):
        H.cfd({"nel": 1000, "areas": ar[:-8], "neighbours": nb, "normals": nr})
    with pytest.raises(ValueError):
        H.cfd(m, variables0=np.zeros(5))
    with pytest.raises(H.HclibError):
        H.cfd_bounds({"nel": 0, "areas": ar, "neighbours": nb, "normals": nr})


def test_argument_errors_come_before_the_device():
    """Valid arguments reach the device check; without a GPU that is ENODEV, never a fallback,
    also for iterations = 0, which launches nothing."""
    import torch

    if torch.cuda.is_available():
        return  # tests/test_cfd_gpu.py runs the solver
    for iterations in (0, 5):
        for form in ("dag", "phases"):
            with pytest.raises(H.HclibError) as e:
                H.cfd(R.fixture_path("tiny"), iterations, 8, form)
            assert "(%d)" % ENODEV in str(e.value)
