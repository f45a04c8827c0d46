"""Rodinia CFD (euler3d_cpu_double.ref.cpp) restated in numpy, operation for
operation in float64, with a seeded mesh generator and the fixtures of
tests/golden/cfd.

    python -m tests.cfd_ref tests/golden/cfd

writes the fixtures' input files <name>.txt. Their <name>.density, .momentum
and .density_energy are not made here: they are the files the compiled
reference wrote for that input (DESIGN.md §22 has the command), and
tests/test_cfd_host.py holds this restatement to them byte for byte. The files
of `grid` and `hub` are kept gzip-compressed (`python -m tests.cfd_ref
tests/golden/cfd pack`); fixture_path() hands out plain text either way, and
the tests pin the SHA-256 of the text, not of the archive.

The restatement. Every numpy operation on float64 arrays is one IEEE operation
per element, rounded on its own, and the reference built for x86-64 without
-march has no fused multiply-add, so writing the reference's expressions with
its parentheses gives its bits. A face takes one of three branches in the
reference (a neighbour, the wing, the far field, or none for an index below
-2); here all three are computed for every element and each is applied through
np.where under its mask, face after face in the reference's order, so an
element's accumulators see exactly the additions the reference makes (adding a
masked zero would not do: -0.0 + 0.0 is +0.0).
"""
import atexit
import gzip
import os
import shutil
import sys
import tempfile

import numpy as np

GAMMA = 1.4
NNB, NDIM, NVAR, RK = 4, 3, 5, 3
BLOCK_LENGTH = 8
FIXTURES = ("tiny", "pad1", "grid", "hub", "odd")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfd")


# --------------------------------------------------------------- the reader
def nelr_of(nel):
    return BLOCK_LENGTH * (nel // BLOCK_LENGTH + min(1, nel % BLOCK_LENGTH))


def read_input(path):
    """:417-455: the mesh as the reference holds it after reading."""
    tok = open(path).read().split()
    nel = int(tok[0])
    nelr = nelr_of(nel)
    areas = np.empty(nelr, dtype=np.float64)
    nbs = np.empty((nelr, NNB), dtype=np.int32)
    normals = np.empty((nelr, NNB, NDIM), dtype=np.float64)
    at = 1
    for i in range(nel):
        areas[i] = float(tok[at])
        at += 1
        for j in range(NNB):
            k = int(tok[at])
            if k < 0:
                k = -1
            nbs[i, j] = k - 1
            for d in range(NDIM):
                normals[i, j, d] = -float(tok[at + 1 + d])
            at += 1 + NDIM
    areas[nel:] = areas[nel - 1]
    nbs[nel:] = nbs[nel - 1]
    normals[nel:] = normals[nel - 1]
    return {"nel": nel, "nelr": nelr, "areas": areas, "neighbours": nbs, "normals": normals}


# ------------------------------------------------------------- the far field
def far_field():
    """:383-408. (variable[5], momentum_x[3], momentum_y[3], momentum_z[3], density_energy[3])"""
    f64 = np.float64
    angle = f64(3.1415926535897931 / 180.0) * f64(0.0)
    var = np.zeros(NVAR, dtype=np.float64)
    var[0] = 1.4
    p = f64(1.0)
    c = np.sqrt(f64(GAMMA) * p / var[0])
    speed = f64(1.2) * c
    vel = np.array([speed * np.cos(angle), speed * np.sin(angle), 0.0], dtype=np.float64)
    var[1:4] = var[0] * vel
    var[4] = var[0] * (f64(0.5) * (speed * speed)) + (p / f64(GAMMA - 1.0))
    fx, fy, fz, fe = _flux_contribution(var[1:4], var[4], p, vel)
    return var, np.array(fx), np.array(fy), np.array(fz), np.array(fe)


# ------------------------------------------------------- the element formulas
def _flux_contribution(mom, de, p, vel):
    """compute_flux_contribution :136-154; mom, vel: three arrays (or scalars) each"""
    fxx = vel[0] * mom[0] + p
    fxy = vel[0] * mom[1]
    fxz = vel[0] * mom[2]
    fyy = vel[1] * mom[1] + p
    fyz = vel[1] * mom[2]
    fzz = vel[2] * mom[2] + p
    de_p = de + p
    return (fxx, fxy, fxz), (fxy, fyy, fyz), (fxz, fyz, fzz), (vel[0] * de_p, vel[1] * de_p, vel[2] * de_p)


def _derive(v):
    """velocity, speed_sqd, pressure, speed of sound (:156-176) of states v[..., 5]"""
    d, e = v[..., 0], v[..., 4]
    mom = (v[..., 1], v[..., 2], v[..., 3])
    vel = (mom[0] / d, mom[1] / d, mom[2] / d)
    ssq = vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]
    p = (np.float64(GAMMA) - np.float64(1.0)) * (e - np.float64(0.5) * d * ssq)
    c = np.sqrt(np.float64(GAMMA) * p / d)
    return mom, vel, ssq, p, c


def step_factor(v, areas):
    """:186-200"""
    _, _, ssq, _, c = _derive(v)
    return np.float64(0.5) / (np.sqrt(areas) * (np.sqrt(ssq) + c))


def flux(mesh, v, ff):
    """compute_flux :225-343 for every element: [nelr, 5]"""
    nbs, normals = mesh["neighbours"], mesh["normals"]
    ffv, ffx, ffy, ffz, ffe = ff
    sc = np.float64(np.float32(0.2))
    half = np.float64(0.5)
    d_i, e_i = v[:, 0], v[:, 4]
    mom_i, vel_i, ssq_i, p_i, c_i = _derive(v)
    speed_i = np.sqrt(ssq_i)
    fcx_i, fcy_i, fcz_i, fce_i = _flux_contribution(mom_i, e_i, p_i, vel_i)
    n = v.shape[0]
    f_d, f_e = np.zeros(n), np.zeros(n)
    f_m = [np.zeros(n), np.zeros(n), np.zeros(n)]

    def add(acc, mask, term):
        return np.where(mask, acc + term, acc)

    with np.errstate(all="ignore"):
        for j in range(NNB):
            nb = nbs[:, j]
            nrm = (normals[:, j, 0], normals[:, j, 1], normals[:, j, 2])
            is_nb, is_wing, is_far = nb >= 0, nb == -1, nb == -2
            w = v[np.where(is_nb, nb, 0)]
            normal_len = np.sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2])
            d_n, e_n = w[:, 0], w[:, 4]
            mom_n, vel_n, ssq_n, p_n, c_n = _derive(w)
            fcx_n, fcy_n, fcz_n, fce_n = _flux_contribution(mom_n, e_n, p_n, vel_n)
            # a legitimate neighbour: artificial viscosity
            factor = -normal_len * sc * half * (speed_i + np.sqrt(ssq_n) + c_i + c_n)
            f_d = add(f_d, is_nb, factor * (d_i - d_n))
            f_e = add(f_e, is_nb, factor * (e_i - e_n))
            for k in range(3):
                f_m[k] = add(f_m[k], is_nb, factor * (mom_i[k] - mom_n[k]))
            # a wing boundary
            for k in range(3):
                f_m[k] = add(f_m[k], is_wing, nrm[k] * p_i)
            # cell-centered fluxes against the neighbour, or against the far field
            for k in range(3):
                factor = half * nrm[k]
                for mask, o_mom, o_e, o_x, o_y, o_z in ((is_nb, mom_n[k], fce_n[k], fcx_n[k], fcy_n[k], fcz_n[k]),
                                                        (is_far, ffv[1 + k], ffe[k], ffx[k], ffy[k], ffz[k])):
                    f_d = add(f_d, mask, factor * (o_mom + mom_i[k]))
                    f_e = add(f_e, mask, factor * (o_e + fce_i[k]))
                    f_m[0] = add(f_m[0], mask, factor * (o_x + fcx_i[k]))
                    f_m[1] = add(f_m[1], mask, factor * (o_y + fcy_i[k]))
                    f_m[2] = add(f_m[2], mask, factor * (o_z + fcz_i[k]))
    return np.stack([f_d, f_m[0], f_m[1], f_m[2], f_e], axis=1)


def time_step(j, old, sf, fl):
    """:356-362"""
    factor = sf / np.float64(RK + 1 - j)
    return old + factor[:, None] * fl


def run(mesh, iterations=5, variables0=None):
    """main's loop :470-482: variables [nelr, 5] after `iterations` iterations"""
    ff = far_field()
    nelr = mesh["nelr"]
    v = np.tile(ff[0], (nelr, 1)) if variables0 is None else np.array(variables0, dtype=np.float64).reshape(nelr, NVAR)
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            old = v.copy()
            sf = step_factor(v, mesh["areas"])
            for j in range(RK):
                v = time_step(j, old, sf, flux(mesh, v, ff))
    return v


def dump(v, nel, nelr):
    """dump() :84-111 with the stream's default format (%g): the texts of
    density, momentum and density_energy"""
    head = "%d %d\n" % (nel, nelr)
    den = head + "".join("%g\n" % v[i, 0] for i in range(nel))
    mom = head + "".join("%g %g %g \n" % (v[i, 1], v[i, 2], v[i, 3]) for i in range(nel))
    ene = head + "".join("%g\n" % v[i, 4] for i in range(nel))
    return {"density": den, "momentum": mom, "density_energy": ene}


# -------------------------------------------------------- the mesh generator
# A file mesh: nel rows (area, [(k, nx, ny, nz)] * 4) with the file's numbering:
# k > 0 is element k - 1, 0 the wing, k < 0 the far field.
_DIRS = ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0))


def generate(gx, gy, seed, p_wing=0.05, p_far=0.05, p_jump=0.05):
    """A gx x gy torus of elements (element x gy + y) with its four lattice
    neighbours; each face becomes the wing, the far field or a jump to a random
    element with the given probabilities (a jump is one-directional: the target
    does not name the element back). Normals: the lattice direction times
    U(0.5, 1.5) plus noise of 0.05; areas U(0.5, 2). Six decimals, so that the
    file's text is short and reads back exactly."""
    rng = np.random.RandomState(seed)
    nel = gx * gy
    rows = []
    for i in range(nel):
        x, y = divmod(i, gy)
        lattice = (((x + 1) % gx) * gy + y, ((x - 1) % gx) * gy + y, x * gy + (y + 1) % gy, x * gy + (y - 1) % gy)
        faces = []
        for j in range(NNB):
            u = rng.random_sample()
            if u < p_wing:
                k = 0
            elif u < p_wing + p_far:
                k = -1
            elif u < p_wing + p_far + p_jump:
                k = int(rng.randint(nel)) + 1
            else:
                k = lattice[j] + 1
            scale = rng.uniform(0.5, 1.5)
            nrm = [round(_DIRS[j][d] * scale + rng.uniform(-0.05, 0.05), 6) for d in range(NDIM)]
            faces.append([k] + nrm)
        rows.append([round(rng.uniform(0.5, 2.0), 6), faces])
    return rows


def mesh_text(rows):
    out = ["%d\n" % len(rows)]
    for area, faces in rows:
        out.append(repr(float(area)) + "".join("  %d %r %r %r" % (k, float(a), float(b), float(c)) for k, a, b, c in faces)
                   + "\n")
    return "".join(out)


def write_mesh(rows, path):
    with open(path, "w") as f:
        f.write(mesh_text(rows))


def mesh_of(rows, tmpdir, name="mesh.txt"):
    """the rows written to a file under tmpdir and read back: (path, mesh)"""
    path = os.path.join(str(tmpdir), name)
    write_mesh(rows, path)
    return path, read_input(path)


# --------------------------------------------------------------- the fixtures
def _tiny():
    # nel 5, nelr 8: three padded copies; a ring; a wing face on element 1; far-field faces written -1 and -3
    rows = generate(5, 1, 11, 0.0, 0.0, 0.0)
    for i, (_, faces) in enumerate(rows):
        faces[2][0] = -1 if i % 2 else -3
        faces[3][0] = 0 if i == 1 else (i + 2) % 5 + 1
    return rows


def _pad1():
    # nel 9, nelr 16: at block 8 the second block is one real element and seven copies
    return generate(3, 3, 12, 0.1, 0.1, 0.1)


def _grid():
    return generate(40, 25, 13)


def _hub():
    # 68 blocks of 8. Block 0's elements name only each other and boundaries; the first element of every other
    # block names an element of block 0 on its last face: N(0) is all 68 blocks, 67 of them only because they
    # name block 0
    rows = generate(68, 8, 14, 0.02, 0.02, 0.0)
    for i in range(8):
        faces = rows[i][1]
        faces[0][0], faces[1][0] = (i + 1) % 8 + 1, (i - 1) % 8 + 1
        faces[2][0], faces[3][0] = -1, 0 if i == 3 else -2
    for b in range(1, 68):
        rows[8 * b][1][3][0] = b % 8 + 1
    return rows


def _odd():
    # nel 13, nelr 16, a ring with chords: element 2 names itself; element 4 names element 7 on two faces; element
    # 6 has four boundary faces (wing, far field, far field, wing); element 9 names index 14, a padded copy of 12
    rows = generate(13, 1, 15, 0.0, 0.0, 0.0)
    for i in range(13):
        rows[i][1][2][0], rows[i][1][3][0] = (i + 3) % 13 + 1, (i - 3) % 13 + 1
    rows[2][1][2][0] = 3
    rows[4][1][2][0] = rows[4][1][3][0] = 8
    for j, k in enumerate((0, -1, -7, 0)):
        rows[6][1][j][0] = k
    rows[9][1][3][0] = 15
    return rows


MAKERS = {"tiny": _tiny, "pad1": _pad1, "grid": _grid, "hub": _hub, "odd": _odd}


PACKED = ("grid", "hub")  # kept gzip-compressed: 6,200 lines of numbers between them
_unpacked = None


def fixture_path(name, kind="txt"):
    """a path to tests/golden/cfd/<name>.<kind> as plain text: the file itself, or
    its .gz unpacked into a folder that lives as long as the process"""
    global _unpacked
    p = os.path.join(GOLDEN, name + "." + kind)
    if os.path.exists(p):
        return p
    if _unpacked is None:
        _unpacked = tempfile.mkdtemp(prefix="cfd_golden_")
        atexit.register(shutil.rmtree, _unpacked, True)
    out = os.path.join(_unpacked, name + "." + kind)
    if not os.path.exists(out):
        with gzip.open(p + ".gz", "rb") as z, open(out, "wb") as f:
            f.write(z.read())
    return out


def pack(path):
    """<path> -> <path>.gz, reproducibly (no name, no time in the header)"""
    with open(path, "rb") as f, open(path + ".gz", "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as z:
            z.write(f.read())
    os.remove(path)


if __name__ == "__main__":
    # the inputs; with "pack" as a second argument, instead compress what PACKED names (inputs and recorded outputs)
    for name in FIXTURES:
        if len(sys.argv) > 2 and sys.argv[2] == "pack":
            for kind in ("txt", "density", "momentum", "density_energy"):
                if name in PACKED and os.path.exists(os.path.join(sys.argv[1], name + "." + kind)):
                    pack(os.path.join(sys.argv[1], name + "." + kind))
        else:
            write_mesh(MAKERS[name](), os.path.join(sys.argv[1], name + ".txt"))
