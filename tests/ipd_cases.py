"""Hard inputs for the IPD landmark normalisation, and its answer in exact rational arithmetic -- test helper (no GPU).

The operation (FeatureExtractor.py:30-66 and the f32 cast of its callers), per face raw f32[468,3]:

    out[3 L + c] = f32( (f64(raw[L, c]) - f64(raw[1, c])) / ipd ),   ipd = sqrt(fma(dz, dz, fma(dy, dy, dx dx))),  d = raw[33] - raw[263],
    ipd replaced by 1e-6 when it is 0.

REFERENCE.  ref_ipd() and ref_element() restate it with fractions.Fraction: the subtraction rounded once to f64, one rounding per link
of the fma chain, a correctly rounded square root through math.isqrt, the == 0 -> 1e-6 branch, the quotient rounded once to f64 and then
once to f32 (subnormals, overflow to inf and the sign of zero included).  It shares no code with the kernels, the C oracle or numpy.  It
is slow, so reference() applies it to every engineered element, every face's ipd and a fixed sample of SAMPLE ordinary elements;
tests/test_ipd_exact_host.py shows that the C oracle agrees on all of those, and the rest of each face is the C oracle's.

HARD ELEMENTS.  An f64 quotient, reciprocal or square root that is one f64 ulp off changes the f32 result only where the quotient lies
within about one f64 ulp of an f32 rounding boundary (2^-28 of random elements).  _engineer() builds such elements: for the face's ipd it
draws an f32 midpoint m (odd 25-bit significand), sets n = RN53(m ipd) + k ulp, k in {-1, 0, 1}, and keeps the case when n = v - r
exactly with v = f32(n) and r = v - n both float32 (r is a few bits at the far end of n: 3 tries in 16 succeed) and n / ipd lies within
2 f64 ulps of m.  v becomes the landmark's coordinate and r landmark 1's.

DENSE FAMILIES (family(name), 465 faces each unless noted): face k engineers all three coordinates of landmark ENG[k], ENG = every
landmark but 1, 33 and 263, so every engineerable column -- every lane, load iteration and coordinate phase of every copy of the
prologue -- is hit in every family.  Other landmarks are ordinary U(0,1) values (times the family's scale).
  A  lm33 - lm263 = (dx, 0, 0) with dx a 24-bit value: ipd exact, m ipd exact, so k = 0 is an EXACT tie (to even); k = +-1 next to it
  B  ipd a general 3-D distance: inexact square root; on two faces of three lm263 is redrawn until the fma chain's ipd differs from
     three separately rounded squares added left to right; carries double-rounding cases
  C  lm33 == lm263 on a non-zero face: the divisor is 1e-6
  D  scale, by k % 5: pixel scale (x 1920) / x 1e-3 / lm33 and lm263 ADJACENT float32 values in x and y (z too on odd faces): quotients
     of ~1e7 / ipd of ~2^-130 from subnormal lm33, lm263: ordinary landmarks overflow to +-inf, a third of them (x 2^-30) stay finite,
     and on every other such face the engineered m is the overflow threshold 2^128 - 2^103 or a midpoint just below it / ipd of ~2^39 and landmarks of
     ~2^-90: subnormal float32 quotients, m an odd multiple of 2^-150.  + 4 faces of subnormal float32 LANDMARKS (x 2^-130: 18-bit
     multiples of 2^-149 cannot be engineered, they are ordinary faces checked whole by the rational reference): 469 faces
  E  9 faces, zeros and signs, checked whole by the rational reference (nothing engineered): all-zero (2), all landmarks equal (2),
     -0.0 landmarks over a +0.0 landmark 1 (all / a mask) and a mask over a -0.0 landmark 1: results -0.0 where v is -0.0 and landmark
     1 is +0.0, valid 0; one landmark of 2^-149 on an otherwise zero face (one subnormal result, valid 1); ipd 4 with landmarks of
     -2^-149 (the quotient rounds to -0.0) and 3 2^-149

PROBE FAMILIES, for reading x out of a fused kernel (465 faces each).  Every landmark equals landmark 1, so its features are exactly 0,
except the engineered landmark and the two that carry the IPD, 33 and 263 (landmark 33 cannot equal landmark 1: landmark 1 holds the
engineered r, which depends on the ipd).  Engineered |x| log-uniform in [1/8, 1), both signs; on every third face the two float32
neighbours of m also straddle a bf16 rounding tie (low 16 bits 0x7fff | 0x8000 | 0x8001), so that the bf16 mode can see one ulp.
  P   lm33, lm263 ordinary: a general ipd
  PF  lm33 ~ 256, lm263 within 2^-10 of it: landmark 33's features are ~1e5, beyond f16 -- the split-f16 modes RESCUE every face
readout_net(shift) is the network that hands x to the pose: +-1 and power-of-two weights, zero biases, zero weight on the columns of
landmarks 1, 33 and 263; E0 sums coordinate c of all engineered landmarks (one non-zero term per face) into a +- pair of units, the
ReLU funnel carries the six values, E4 recombines them: pose[:, c] = tanh(2^-shift x_c) 2^shift, every sum of one non-zero term.
shift = 0 is the live-Tanh read-out.  shift = 60 puts the Tanh argument below 2^-60, where tanhf(z) == z in any sane math library
(z^3 / 3 is 2^-120 of z), so pose[:, c] == x_c EXACTLY: the device's tanhf and the C library's differ by up to 2 ulps elsewhere, and only
this form can be compared bit for bit with the C oracle's chain.  The split-f16 and bf16 modes cannot carry 2^-60 (f16 pieces), they
read through shift = 0.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from nlml_hpe_amd import synth

NOSE, EYE_L, EYE_R = 1, 33, 263
ENG = np.array([L for L in range(468) if L not in (NOSE, EYE_L, EYE_R)])        # 465 landmarks, 1,395 columns
ENG_COLS = (3 * ENG[:, None] + np.arange(3)[None, :]).reshape(-1)
N_FACES = len(ENG)
SAMPLE = 20000
_STREAM = 60          # Philox stream ids 60.. of synth.rng belong to this file
DENSE = ("A", "B", "C", "D", "E")
PROBES = ("P", "PF")
F16_OVER = 65520.0    # f32 values from here on convert to an infinite f16: the split-f16 modes rescue the face
INF = math.inf


# ---- the exact reference ------------------------------------------------------------------------------------------------------------
def _two(e: int) -> Fraction:
    return Fraction(1 << e) if e >= 0 else Fraction(1, 1 << -e)


def rn(a: Fraction, p: int, emin: int, emax: int):
    """a >= 0 rounded to nearest, ties to even, in the binary format of p significant bits whose quantum is at least 2^emin and whose
    finite values are below 2^(emax + 1) -> Fraction, or INF."""
    if a == 0:
        return a
    n, d = a.numerator, a.denominator
    e = n.bit_length() - d.bit_length()
    if not (n >= (d << e) if e >= 0 else (n << -e) >= d):
        e -= 1                                            # e = floor(log2 a)
    q = max(e - p + 1, emin)
    num, den = (n << -q, d) if q < 0 else (n, d << q)
    fl, rem = divmod(num, den)
    if 2 * rem > den or (2 * rem == den and (fl & 1)):
        fl += 1
    res = Fraction(fl) * _two(q)
    return INF if res >= _two(emax + 1) else res


def rn64(a: Fraction) -> Fraction:
    """Signed, f64."""
    r = rn(abs(a), 53, -1074, 1023)
    assert r != INF
    return -r if a < 0 else r


def sqrt64(s: Fraction) -> Fraction:
    """The correctly rounded f64 square root of an f64 value s >= 0."""
    if s == 0:
        return s
    m, den = s.numerator, s.denominator
    assert den & (den - 1) == 0
    e = -(den.bit_length() - 1)
    if e & 1:
        m, e = m << 1, e - 1
    k = max(0, (130 - m.bit_length()) // 2)             # the root has >= 64 bits: r + 1/2 below is never a tie of 53 bits
    m, e = m << (2 * k), e - 2 * k
    r = math.isqrt(m)
    return rn64(Fraction(2 * r + (0 if r * r == m else 1), 2) * _two(e // 2))


ONE_MICRO = Fraction(1e-6)      # the f64 value of the literal


def ref_radicand(l33, l263, fused_chain: bool = True) -> Fraction:
    """l33, l263: three f32 values each -> the f64 sum of squares.  fused_chain False: three separately rounded squares added left to
    right (a WRONG variant)."""
    dx, dy, dz = (rn64(Fraction(float(a)) - Fraction(float(b))) for a, b in zip(l33, l263))
    if fused_chain:
        return rn64(dz * dz + rn64(dy * dy + rn64(dx * dx)))
    return rn64(rn64(rn64(dx * dx) + rn64(dy * dy)) + rn64(dz * dz))


def ref_ipd(l33, l263, fused_chain: bool = True) -> Fraction:
    d = sqrt64(ref_radicand(l33, l263, fused_chain))
    return ONE_MICRO if d == 0 else d


def ref_quotient(v: float, r: float):
    """(negative?, |n| as Fraction): n = f64(v) - f64(r) rounded once to f64, with IEEE's sign of zero."""
    d = Fraction(v) - Fraction(r)
    if d == 0:
        return (v == 0 and math.copysign(1.0, v) < 0 and math.copysign(1.0, r) > 0), d
    return d < 0, rn(abs(d), 53, -1074, 1023)


def ref_element(v: float, r: float, ipd: Fraction, direct: bool = False) -> float:
    """The f32 result as a Python float (signed zero, +-inf).  direct: ONE rounding of the exact quotient to f32 (a WRONG variant)."""
    neg, n = ref_quotient(v, r)
    q = n / ipd
    if not direct:
        q = rn(q, 53, -1074, 1023)
    o = rn(q, 24, -149, 127) if q != INF else INF
    o = INF if o == INF else float(o)
    return -o if neg else o


def f32_bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- engineered elements --------------------------------------------------------------------------------------------------------------
def _ulp53(x: float) -> Fraction:
    return _two(math.frexp(x)[1] - 53) if abs(x) >= 2.0 ** -1022 else _two(-1074)


def _m_normal(g, lo_exp: int, hi_exp: int, bf16_tie: bool = False) -> float:
    """An f32 midpoint of magnitude in [2^lo_exp, 2^hi_exp), log-uniform, with either sign."""
    u = lo_exp + (hi_exp - lo_exp) * g.random()
    e = math.floor(u)
    M = min(int(2.0 ** (u - e) * 2 ** 23), 2 ** 24 - 1)
    if bf16_tie:
        M = (M & ~0xFFFF) | (0x7FFF if g.random() < 0.5 else 0x8000)
    m = math.ldexp(float(2 * M + 1), e - 24)
    return -m if g.random() < 0.5 else m


def _engineer(g, ipd: float, ks, draw_m, tries: int = 20000):
    """-> (v f32, r f32, m, k): (f64(v) - f64(r)) / ipd within 2 f64 ulps of the f32 midpoint m, v - r exact.  k is drawn first and
    kept: an exact product m ipd (k = 0 in family A) is accepted far more often than its neighbours."""
    ipd_q = Fraction(ipd)
    k = int(ks[g.integers(len(ks))])
    for t in range(tries):
        if t == tries // 2:
            k = 0                 # an ipd of a few bits (adjacent eyes: 1.5 2^-24) leaves no n = m ipd +- ulp that is v - r: exact ties only
        m = draw_m(g)
        n = m * ipd                                       # RN53 of the exact product
        if k:
            n = math.nextafter(n, math.copysign(INF, n) * k)
        with np.errstate(over="ignore"):
            v = np.float32(n)
        if not np.isfinite(v) or v == 0:
            continue
        r = float(v) - n
        if r == 0 or float(np.float32(r)) != r or float(v) - r != n or Fraction(float(v)) - Fraction(r) != Fraction(n):
            continue
        if abs(Fraction(n) / ipd_q - Fraction(m)) > 2 * _ulp53(m):
            continue
        return v, np.float32(r), m, k
    raise RuntimeError(f"no engineered element in {tries} tries for ipd {ipd!r}")


def _fill(fam, g, faces, ks, draw_m_of):
    """Engineer landmark ENG[k % 465] of every face k in `faces` (lm33, lm263 and the ordinary landmarks are already in place)."""
    raw = fam["raw"]
    for k in faces:
        L = int(ENG[k % N_FACES])
        ipd = float(ref_ipd(raw[k, EYE_L], raw[k, EYE_R]))
        for c in range(3):
            v, r, m, kk = _engineer(g, ipd, ks, draw_m_of(k, ipd))
            raw[k, L, c], raw[k, NOSE, c] = v, r
            fam["eng_face"].append(k); fam["eng_col"].append(3 * L + c); fam["eng_m"].append(m); fam["eng_k"].append(kk)


def _m_for_scale(scale: float):
    """Midpoints that make n = m ipd a coordinate of about `scale`: quotients of the family's own magnitude."""
    def of(k, ipd):
        e = math.floor(math.log2(scale / ipd))
        return lambda g: _m_normal(g, e - 2, e + 1)
    return of


def _distinct_eyes(g, raw, k, scale, want_chain_visible):
    for _ in range(2000):
        raw[k, EYE_R] = synth._uniform_f32(g, (3,), 0.0, 1.0) * np.float32(scale)
        if want_chain_visible:       # a coordinate difference of more than 26 bits: its square is inexact, so the chain's order shows
            raw[k, EYE_R] *= (2.0 ** -g.integers(4, 12, size=3)).astype(np.float32)
        a = ref_ipd(raw[k, EYE_L], raw[k, EYE_R])
        if a != ONE_MICRO and (not want_chain_visible or a != ref_ipd(raw[k, EYE_L], raw[k, EYE_R], fused_chain=False)):
            return
    raise RuntimeError("no such pair of eyes")


def _new(B, g, scale=1.0):
    raw = synth._uniform_f32(g, (B, 468, 3), 0.0, 1.0) * np.float32(scale)
    return {"raw": raw, "eng_face": [], "eng_col": [], "eng_m": [], "eng_k": [], "whole": []}


def _build(name: str) -> dict:
    g = synth.rng(17, _STREAM + (DENSE + PROBES).index(name))
    every = range(N_FACES)
    if name == "A":
        fam = _new(N_FACES, g)
        raw = fam["raw"]
        raw[:, EYE_L] = raw[:, EYE_R]
        raw[:, EYE_R, 0] = synth._uniform_f32(g, (N_FACES,), 0.5, 0.75)
        raw[:, EYE_L, 0] = synth._uniform_f32(g, (N_FACES,), 0.75, 1.0)
        _fill(fam, g, every, (-1, 0, 0, 1), _m_for_scale(0.5))       # half exact ties
    elif name == "B":
        fam = _new(N_FACES, g)
        for k in every:
            _distinct_eyes(g, fam["raw"], k, 1.0, want_chain_visible=k % 3 != 2)
        _fill(fam, g, every, (-1, 0, 1), _m_for_scale(0.5))
    elif name == "C":
        fam = _new(N_FACES, g)
        fam["raw"][:, EYE_R] = fam["raw"][:, EYE_L]
        _fill(fam, g, every, (-1, 0, 1), _m_for_scale(0.5))
    elif name == "D":
        fam = _new(N_FACES + 4, g)
        raw = fam["raw"]
        kind = np.arange(N_FACES + 4) % 5
        kind[N_FACES:] = 5
        fam["kind"] = kind
        raw[kind == 0] *= np.float32(1920.0)
        raw[kind == 1] *= np.float32(1e-3)
        for k in np.flatnonzero(kind == 2):                           # adjacent float32 values
            raw[k, EYE_L] = raw[k, EYE_R]
            for c in range(3 if k & 1 else 2):
                raw[k, EYE_L, c] = np.nextafter(raw[k, EYE_R, c], np.float32(2.0))
        for k in np.flatnonzero(kind == 3):                           # ipd ~ 2^-130: quotients overflow
            raw[k, EYE_R] = 0.0
            raw[k, EYE_L] = (synth._uniform_f32(g, (3,), 0.25, 1.0) * np.float32(2.0 ** -128)) * np.float32(0.25)
            raw[k, 2::3] *= np.float32(2.0 ** -30)                   # a third of the landmarks stay finite (263, among them, is zero)
        for k in np.flatnonzero(kind == 4):                           # ipd ~ 2^39, landmarks ~ 2^-90: subnormal quotients
            eyes = raw[k, [EYE_L, EYE_R]] * np.float32(2.0 ** 40)
            raw[k] *= np.float32(2.0 ** -90)
            raw[k, [EYE_L, EYE_R]] = eyes
        raw[kind == 5] *= np.float32(2.0 ** -130)                     # subnormal landmarks

        def draw(k, ipd):
            if kind[k] == 0:
                return _m_for_scale(960.0)(k, ipd)
            if kind[k] == 1:
                return _m_for_scale(5e-4)(k, ipd)
            if kind[k] == 3 and (k // 5) & 1:
                # the overflow threshold 2^128 - 2^103 itself on one draw in four, else one of the 1,024 midpoints below it
                return lambda g: math.copysign(math.ldexp(float(2 ** 25 - 1 - 2 * (0 if g.random() < 0.25 else int(g.integers(1, 1024)))), 103),
                                               g.random() - 0.5)
            if kind[k] == 3:
                return _m_for_scale(2.0 ** -31)(k, ipd)
            if kind[k] == 4:
                return lambda g: math.copysign(math.ldexp(float(2 * int(g.integers(2 ** 14, 2 ** 22)) + 1), -150), g.random() - 0.5)
            return _m_for_scale(0.5)(k, ipd)
        _fill(fam, g, every, (-1, 0, 1), draw)
        fam["whole"] = list(range(N_FACES, N_FACES + 4))
    elif name == "E":
        fam = _new(9, g)
        raw = fam["raw"]
        raw[0:2] = 0.0
        raw[2] = np.array([0.25, 0.5, 0.75], np.float32)
        raw[3] = np.float32(0.1)
        raw[4] = -0.0
        raw[4, NOSE] = 0.0
        raw[5] = np.where(g.random((468, 3)) < 0.5, np.float32(-0.0), np.float32(0.0))
        raw[5, NOSE] = 0.0
        raw[6] = np.where(g.random((468, 3)) < 0.5, np.float32(-0.0), np.float32(0.0))
        raw[6, NOSE] = -0.0
        raw[7] = 0.0
        raw[7, 200, 1] = np.float32(2.0 ** -149)
        raw[8] = 0.0
        raw[8, EYE_L, 0] = 4.0
        raw[8, 100, 2] = np.float32(-2.0 ** -149)
        raw[8, 467, 2] = np.float32(3 * 2.0 ** -149)
        fam["whole"] = list(range(9))
    elif name in PROBES:
        fam = _new(N_FACES, g)
        raw = fam["raw"]
        if name == "PF":
            raw[:, EYE_L] += np.float32(256.0)
            raw[:, EYE_R] = raw[:, EYE_L] + raw[:, EYE_R] * np.float32(2.0 ** -10)
        _fill(fam, g, every, (-1, 0, 1), lambda k, ipd: (lambda g: _m_normal(g, -3, 0, bf16_tie=k % 3 == 0)))
        keep = np.ones(468, bool)
        for k in every:
            keep[:] = True
            keep[[EYE_L, EYE_R, int(ENG[k])]] = False
            raw[k, keep] = raw[k, NOSE]
    else:
        raise KeyError(name)
    for key in ("eng_face", "eng_col", "eng_k"):
        fam[key] = np.array(fam[key], np.int64)
    fam["eng_m"] = np.array(fam["eng_m"], np.float64)
    fam["name"] = name
    return fam


_families: dict = {}


def family(name: str) -> dict:
    """dict(name, raw f32[B,468,3], eng_face, eng_col int[n], eng_m f64[n] (the midpoint), eng_k int[n], whole = faces the rational
    reference answers on every element, ipd f64[B] (rational), eng_want f32[n] (rational)[, kind int[B] (family D)])."""
    if name not in _families:
        fam = _build(name)
        raw = fam["raw"]
        ipd_q = [ref_ipd(f[EYE_L], f[EYE_R]) for f in raw]
        fam["ipd"] = np.array([float(q) for q in ipd_q])
        flat = raw.reshape(len(raw), -1)
        with np.errstate(over="ignore"):
            fam["eng_want"] = np.array([ref_element(float(flat[f, c]), float(flat[f, 3 + c % 3]), ipd_q[f])
                                        for f, c in zip(fam["eng_face"], fam["eng_col"])], np.float64).astype(np.float32)
        fam["ipd_q"] = ipd_q
        _families[name] = fam
    return _families[name]


def rational_rows(fam: dict, faces) -> np.ndarray:
    """f32[len(faces), 1404]: whole faces by the rational reference."""
    flat = fam["raw"].reshape(len(fam["raw"]), -1)
    out = np.empty((len(faces), 1404), np.float32)
    with np.errstate(over="ignore"):
        for i, f in enumerate(faces):
            out[i] = np.array([ref_element(float(flat[f, c]), float(flat[f, 3 + c % 3]), fam["ipd_q"][f]) for c in range(1404)], np.float64)
    return out


def sample(fam: dict, n: int):
    """A fixed sample of n ordinary elements of the family -> (face int[n], col int[n], want f32[n] by the rational reference)."""
    key = ("sample", n)
    if key not in fam:
        g = synth.rng(23, _STREAM + 20 + (DENSE + PROBES).index(fam["name"]))
        B = len(fam["raw"])
        face, col = g.integers(0, B, size=n), g.integers(0, 1404, size=n)
        flat = fam["raw"].reshape(B, -1)
        with np.errstate(over="ignore"):
            want = np.array([ref_element(float(flat[f, c]), float(flat[f, 3 + c % 3]), fam["ipd_q"][f]) for f, c in zip(face, col)],
                            np.float64).astype(np.float32)
        fam[key] = (face, col, want)
    return fam[key]


def sample_share(name: str) -> int:
    """SAMPLE ordinary elements over the seven families, in equal parts."""
    return SAMPLE // len(DENSE + PROBES) + 1


def reference(name: str):
    """-> (features f32[B,1404], valid bool[B]): the C oracle's rows with the rational reference's values written over every
    engineered element, every sampled element and every `whole` face (tests/test_ipd_exact_host.py: the two agree there)."""
    fam = family(name)
    key = "reference"
    if key not in fam:
        from oracle import c_oracle as CO
        out = CO.normalize_ipd(fam["raw"], True).copy()
        out[fam["eng_face"], fam["eng_col"]] = fam["eng_want"]
        f, c, w = sample(fam, sample_share(name))
        out[f, c] = w
        if len(fam["whole"]):
            out[fam["whole"]] = rational_rows(fam, fam["whole"])
        fam[key] = (out, ((f32_bits(out) & 0x7FFFFFFF) != 0).any(axis=1))
    return fam[key]


def nudged(features: np.ndarray, fam: dict) -> np.ndarray:
    """The features with every engineered element moved one float32 ulp, across the midpoint it was engineered against."""
    out = features.copy()
    x = out[fam["eng_face"], fam["eng_col"]]
    with np.errstate(over="ignore"):
        toward = np.where(np.abs(fam["eng_m"]) > np.abs(x.astype(np.float64)), np.sign(x) * np.float32(np.inf), np.float32(0.0)).astype(np.float32)
    with np.errstate(over="ignore"):                      # the largest finite float32 next to the overflow threshold moves to inf
        out[fam["eng_face"], fam["eng_col"]] = np.nextafter(x, toward)
    return out


# ---- the read-out network -------------------------------------------------------------------------------------------------------------
HEAD_NAMES = ("yaw", "pitch", "roll")
READOUT_EXACT_SHIFT = 60


def readout_net(shift: int = 0):
    """-> (encoder state dict, {head: state dict}) with pose[:, c] = 2^shift tanh(2^-shift x_c) on the probe families (module docstring)."""
    import exact_nets as XN
    widths = (1404,) + XN.ENCODER_OUT
    enc = {}
    for i in range(6):
        enc[f"encoder.{2 * i}.weight"] = np.zeros((widths[i + 1], widths[i]), np.float32)
        enc[f"encoder.{2 * i}.bias"] = np.zeros(widths[i + 1], np.float32)
    for c in range(3):
        enc["encoder.0.weight"][2 * c, 3 * ENG + c] = 1.0
        enc["encoder.0.weight"][2 * c + 1, 3 * ENG + c] = -1.0
        enc["encoder.8.weight"][c, 2 * c], enc["encoder.8.weight"][c, 2 * c + 1] = 2.0 ** -shift, -(2.0 ** -shift)
        enc["encoder.10.weight"][3 * c, c] = 2.0 ** shift
    for i in (2, 4, 6):
        enc[f"encoder.{i}.weight"][np.arange(6), np.arange(6)] = 1.0
    heads = {}
    for n in HEAD_NAMES:
        sd = {}
        for i, (n_out, n_in) in enumerate(XN.HEAD_SHAPES):
            sd[f"model.{2 * i}.weight"] = np.zeros((n_out, n_in), np.float32)
            sd[f"model.{2 * i}.bias"] = np.zeros(n_out, np.float32)
        sd["model.0.weight"][0, 0], sd["model.0.weight"][1, 0] = 1.0, -1.0
        for i in (2, 4, 6):
            sd[f"model.{i}.weight"][[0, 1], [0, 1]] = 1.0
        sd["model.8.weight"][0, 0], sd["model.8.weight"][0, 1] = 1.0, -1.0
        heads[n] = sd
    return enc, heads
