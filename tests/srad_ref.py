"""Rodinia SRAD (test/performance-regression/full-apps/rodinia/srad/srad.ref.cpp)
restated in numpy, one IEEE operation per element and in the reference's types,
and the reader of the fixtures under tests/golden/srad/.

A fixture is data only: NAME.json (rows, cols, r1, r2, c1, c2, lambda, niter),
NAME.j0.bin (the image after `J = (float)exp(I)`, recorded from the compiled
reference run with niter = 0) and NAME.j.bin (the image the compiled reference
prints after niter iterations), both rows x cols little-endian float32 holding
the floats the reference passed to printf (a float promoted to double converts
back without loss). DESIGN.md §23 has the recipe.
"""
import json
import pathlib

import numpy as np

GOLDEN = pathlib.Path(__file__).parent / "golden" / "srad"
FIXTURES = ("a32x48_it3", "one16_it1", "pix16x32_it4", "tail48x16_it7", "n128_it20")

f32, f64 = np.float32, np.float64


def bits(a):
    """The bit patterns of a float32 array (or scalar), for exact comparison."""
    return np.ascontiguousarray(np.asarray(a, dtype=f32)).view(np.uint32)


def read_fixture(name):
    """{"rows", "cols", "roi": (r1, r2, c1, c2), "lam", "niter", "j0", "j"}."""
    p = json.loads((GOLDEN / f"{name}.json").read_text())
    shape = (p["rows"], p["cols"])
    fx = {"rows": p["rows"], "cols": p["cols"], "roi": (p["r1"], p["r2"], p["c1"], p["c2"]), "lam": p["lambda"],
          "niter": p["niter"]}
    for k in ("j0", "j"):
        fx[k] = np.fromfile(GOLDEN / f"{name}.{k}.bin", dtype="<f4").astype(f32).reshape(shape)
    return fx


def q0sqr_of(J, roi):
    """srad.ref.cpp:131-141: the serial section. The two float sums walk the
    region of interest row-major, one rounded add at a time."""
    r1, r2, c1, c2 = roi
    s, s2 = f32(0), f32(0)
    for tmp in J[r1:r2 + 1, c1:c2 + 1].ravel():
        s = f32(s + tmp)
        s2 = f32(s2 + f32(tmp * tmp))
    size_r = f32((r2 - r1 + 1) * (c2 - c1 + 1))
    with np.errstate(all="ignore"):
        mean = f32(s / size_r)
        var = f32(f32(s2 / size_r) - f32(mean * mean))
        return f32(var / f32(mean * mean))


def srad(j0, roi, lam, niter):
    """(J, q0sqr[niter]) after niter iterations from the image j0."""
    J = np.array(j0, dtype=f32)
    rows, cols = J.shape
    lam = f32(lam)
    iN = np.maximum(np.arange(rows) - 1, 0)
    iS = np.minimum(np.arange(rows) + 1, rows - 1)
    jW = np.maximum(np.arange(cols) - 1, 0)
    jE = np.minimum(np.arange(cols) + 1, cols - 1)
    q = np.zeros(niter, dtype=f32)
    with np.errstate(all="ignore"):
        for it in range(niter):
            q0 = q0sqr_of(J, roi)
            q[it] = q0
            # sweep 1 (:145-176)
            dN = J[iN, :] - J
            dS = J[iS, :] - J
            dW = J[:, jW] - J
            dE = J[:, jE] - J
            G2 = (((dN * dN + dS * dS) + dW * dW) + dE * dE) / (J * J)
            L = (((dN + dS) + dW) + dE) / J
            num = (f64(0.5) * G2.astype(f64) - f64(1.0 / 16.0) * (L * L).astype(f64)).astype(f32)
            den = (f64(1) + f64(.25) * L.astype(f64)).astype(f32)
            qsqr = num / (den * den)
            den = (qsqr - q0) / f32(q0 * f32(f32(1) + q0))
            c = (f64(1.0) / (f64(1.0) + den.astype(f64))).astype(f32)
            # `if (c < 0) c = 0; else if (c > 1) c = 1;`: a NaN and a -0.0 pass through
            c = np.where(c < 0, f32(0), np.where(c > 1, f32(1), c)).astype(f32)
            # sweep 2 (:182-207)
            D = ((c * dN + c[iS, :] * dS) + c * dW) + c[:, jE] * dE
            J = (J.astype(f64) + (f64(0.25) * f64(lam)) * D.astype(f64)).astype(f32)
    return J, q
