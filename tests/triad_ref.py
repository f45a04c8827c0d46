"""The forasync triad a[i] = b[i] + s * c[i] restated for the tests, with the
inputs that can tell a wrong kernel from a right one.

expected(b, c, s) is the reference's loop in numpy float32: the product is
rounded to float32, then the sum is (two operations, numpy contracts nothing
and flushes no subnormal). Results are compared as 32-bit patterns; where the
expected value is a NaN the result only has to be a NaN.

Input sets, all float32:
  uniform  rng.random in [0, 1), used with s = 3.0. A fused multiply-add gives
           other bits than the two rounded operations on about one element in
           seven, so contraction shows. For this set alone the result is also
           within 1 ulp of the float64 value (the two-rounded value itself
           reaches exactly 1 ulp of error here and no more). The other sets
           cancel, which makes that bound false for the reference too.
  bits     b and c are uniformly random 32-bit patterns: every sign, every
           binade, subnormals, NaNs and infinities. Random patterns never hit
           -0.0 or an infinity exactly (2^-32 and 2^-31 per element), so four
           elements are planted: b[5] = -0.0, c[6] = -0.0, b[9] = +inf,
           b[10] = -inf. check_coverage() asserts on the host that a draw holds
           a subnormal result, a subnormal product, a NaN result, an infinite
           result and a -0.0 input for the s it is used with.
  edges    edges_block(s): a short hand-written block (signed zeros, overflow
           of the add, inf - inf, exact cancellation b = -(s c) and one ulp off
           it, the smallest subnormal). With s = 0 and s = inf the same block
           holds 0 * inf: s = 0 against c = +-inf, s = inf against c = +-0.

Device side (TriadBench): `a` is a 16-byte aligned window of a larger int32
buffer filled with SENTINEL, a NaN pattern no arithmetic produces; GUARD
elements lie in front of the window and at least GUARD behind it. Before a
launch a[0, n) holds SENTINEL too. After it every element of a[0, n) has the
expected bits (and is not SENTINEL: an element never written is seen even
where a NaN is expected) and every word outside the window still holds
SENTINEL.
"""
import numpy as np

SENTINEL = 0x7FC0DEAD
GUARD = 4096  # elements; a multiple of 4, so the window stays 16-byte aligned
S_VALUES = (3.0, -0.3, 2.5e-20)
EDGE_S_VALUES = S_VALUES + (0.0, float("inf"))
FMAX = np.finfo(np.float32).max
TINY = np.finfo(np.float32).tiny          # smallest normal
DENORM_MIN = np.float32(2.0 ** -149)


def expected(b, c, s):
    """b + s * c as two float32 operations, each rounded."""
    assert b.dtype == np.float32 and c.dtype == np.float32
    with np.errstate(all="ignore"):
        p = np.float32(s) * c
        assert p.dtype == np.float32
        return b + p


def uniform_inputs(n, seed=2024):
    rng = np.random.default_rng(seed)
    return rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)


def bits_inputs(n, seed=4049):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 32, size=n, dtype=np.uint32).view(np.float32)
    c = rng.integers(0, 1 << 32, size=n, dtype=np.uint32).view(np.float32)
    if n > 10:
        b[5] = -0.0
        c[6] = -0.0
        b[9] = np.inf
        b[10] = -np.inf
    return b, c


def _subnormal(x):
    with np.errstate(all="ignore"):
        return (x != 0) & (np.abs(x) < TINY)  # False for NaN


def coverage(b, c, s):
    """How many elements of the case fall in each class the kernel has to get
    right beyond ordinary rounding."""
    with np.errstate(all="ignore"):
        p = np.float32(s) * c
        r = b + p
    return {
        "subnormal_result": int(_subnormal(r).sum()),
        "subnormal_product": int(_subnormal(p).sum()),
        "nan_result": int(np.isnan(r).sum()),
        "inf_result": int(np.isinf(r).sum()),
        "negative_zero_input": int(((b.view(np.uint32) == 0x80000000) | (c.view(np.uint32) == 0x80000000)).sum()),
    }


def check_coverage(b, c, s):
    cov = coverage(b, c, s)
    missing = [k for k, v in cov.items() if v == 0]
    assert not missing, f"the bits draw at s = {s} holds no {missing}: {cov}"
    return cov


def edges_block(s):
    """(b, c) of the hand-written cases for the scalar s; what each expects is
    left to expected()."""
    s32 = np.float32(s)
    pz, nz, inf = np.float32(0.0), np.float32(-0.0), np.float32(np.inf)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        cases = [
            # signed zeros: (+0) + (+0) = +0, (-0) + (-0) = -0, mixed = +0; the
            # product's zero takes the sign of s * c
            (pz, pz), (pz, nz), (nz, pz), (nz, nz),
            # a zero product under a non-zero b and the reverse
            (one, nz), (-one, pz), (pz, one), (nz, -one),
            # the largest finite value: the product overflows, or only the add does
            (pz, FMAX), (pz, -FMAX), (FMAX, FMAX), (-FMAX, -FMAX), (FMAX, -FMAX),
        ]
        half = np.float32(FMAX / 2)
        ch = np.float32(np.clip(half / s32, -FMAX, FMAX)) if s32 != 0 and np.isfinite(s32) else one
        cases += [(FMAX, ch), (-FMAX, -ch), (FMAX, np.float32(2) * ch)]  # s c = +-FMAX / 2, FMAX: the add overflows
        # infinities: inf + (-inf), inf + inf; with s = 0 the product is 0 * inf
        cases += [(inf, -inf), (-inf, inf), (inf, inf), (-inf, -inf), (one, inf), (one, -inf)]
        # cancellation: b = -(s c) exactly gives +0; one ulp either side gives
        # one ulp of the product, never the product's rounding error
        for cv in (np.float32(1.2345678), np.float32(-7.6543e10), np.float32(3.3e-30)):
            p = s32 * cv
            if np.isfinite(p) and p != 0:
                cases += [(-p, cv), (np.nextafter(-p, inf), cv), (np.nextafter(-p, -inf), cv)]
            else:
                cases += [(one, cv)] * 3
        # the smallest subnormal as b, as c, and against itself
        d = DENORM_MIN
        cases += [(d, pz), (-d, pz), (pz, d), (pz, -d), (d, d), (d, -d), (-d, d), (np.float32(TINY), -d),
                  (np.float32(-TINY), d)]
    b = np.array([x for x, _ in cases], dtype=np.float32)
    c = np.array([y for _, y in cases], dtype=np.float32)
    return b, c


def ulp_error_vs_float64(got, b, c, s):
    """|got - (b + s c in float64)| in float32 ulps of the float64 value
    (host, for the uniform set)."""
    ref = b.astype(np.float64) + np.float64(np.float32(s)) * c.astype(np.float64)
    _, e = np.frexp(ref)
    ulp = np.ldexp(1.0, np.maximum(e - 24, -149))
    return np.abs(got.astype(np.float64) - ref) / ulp


# ------------------------------------------------------------------ device
class TriadBench:
    """Inputs, expected values and the guarded output buffer on the device,
    generated once at the largest size and sliced from offset 0 (which keeps
    the 16-byte alignment). Nothing here is written after construction except
    the output buffer."""

    def __init__(self, torch, nmax, nmax_all_s=None):
        self.torch = torch
        self.nmax = nmax
        self.buf = torch.full((GUARD + nmax + GUARD + 4,), SENTINEL, dtype=torch.int32, device="cuda")
        assert self.a_ptr() % 16 == 0
        self.host = {"uniform": uniform_inputs(nmax), "bits": bits_inputs(nmax)}
        self.dev = {k: tuple(torch.from_numpy(x).cuda() for x in v) for k, v in self.host.items()}
        self.nmax_all_s = nmax if nmax_all_s is None else min(nmax, nmax_all_s)
        self._exp = {}
        self._dirty = nmax

    def a_ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def reset(self):
        self.buf.fill_(SENTINEL)
        self._dirty = 0

    def prefill(self, n):
        """SENTINEL over a[0, n) and over what the launch before wrote."""
        self.buf[GUARD:GUARD + max(n, self._dirty)].fill_(SENTINEL)
        self._dirty = n

    def inputs(self, kind):
        return self.dev[kind]

    def expected_bits(self, kind, s, n, cover=True):
        """int32 device tensor of the two-rounded result's bits, computed on the
        host once per (set, s) and shared."""
        key = (kind, float(s))
        if key not in self._exp:
            # the two (set, s) every kernel form runs are kept at full length,
            # the rest of the matrix at the length its two forms need
            m = self.nmax if key in (("uniform", 3.0), ("bits", S_VALUES[2])) else self.nmax_all_s
            assert n <= m, (key, n, m)
            b, c = self.host[kind]
            if kind == "bits" and cover:
                check_coverage(b[:m], c[:m], s)
            self._exp[key] = self.torch.from_numpy(expected(b[:m], c[:m], s).view(np.int32)).cuda()
        assert n <= self._exp[key].numel(), (key, n)
        return self._exp[key][:n]

    def launch(self, H, kind, s, n, b=None, c=None):
        """a[0, n) = SENTINEL, then the triad through the C ABI on torch's stream."""
        torch = self.torch
        self.prefill(n)
        if b is None:
            b, c = self.dev[kind]
        assert b.data_ptr() % 16 == 0 and c.data_ptr() % 16 == 0
        H.triad_f32(self.a_ptr(), b.data_ptr(), c.data_ptr(), s, n, torch.cuda.current_stream().cuda_stream)

    def mismatches(self, want_bits, n, visited=None):
        """Indices (a few) where a[0, n) is wrong and where the guard changed.
        want_bits: int32 tensor of n expected patterns; visited: optional bool
        tensor, False where the launch must leave SENTINEL."""
        torch = self.torch
        got = self.buf[GUARD:GUARD + n]
        gf, wf = got.view(torch.float32), want_bits.view(torch.float32)
        ok = ((got == want_bits) | (torch.isnan(gf) & torch.isnan(wf))) & (got != SENTINEL)
        if visited is not None:
            ok = torch.where(visited, ok, got == SENTINEL)
        front = self.buf[:GUARD] == SENTINEL
        back = self.buf[GUARD + n:] == SENTINEL
        if bool(ok.all() & front.all() & back.all()):
            return None
        bad = torch.nonzero(~ok).flatten()
        out = {"wrong": int(bad.numel()), "guard_front": int((~front).sum()), "guard_back": int((~back).sum())}
        out["first"] = [(int(i), hex(int(got[i]) & 0xFFFFFFFF), hex(int(want_bits[i]) & 0xFFFFFFFF))
                        for i in bad[:8].tolist()]
        gb = torch.nonzero(~back).flatten()
        out["guard_back_first"] = [n + int(i) for i in gb[:4].tolist()]
        return out

    def within_one_ulp_of_float64(self, n):
        """The uniform set at s = 3.0: every result within 1 ulp (of float32, at
        the float64 value) of b + 3 c in float64, which is exact there."""
        torch = self.torch
        b, c = self.dev["uniform"]
        ref = b[:n].double() + 3.0 * c[:n].double()
        _, e = torch.frexp(ref)
        ulp = torch.ldexp(torch.ones_like(ref), (e - 24).clamp(min=-149))
        got = self.buf[GUARD:GUARD + n].view(torch.float32).double()
        return bool(((got - ref).abs() <= ulp).all())
