"""Test helper: the yardstick of tests/test_cr_reference_host.py and tests/test_td_fvec_exact_gpu.py -- the f-vector entry
f = float32(a cos(b w + c) + d) and its derivative df = float32(((-a) b) sin(b w + c)) (TD_Tester.py:25-28,37,82) with a CORRECTLY
ROUNDED cos / sin from multi-precision arithmetic, and the inputs at which a device build of csrc/cr_cos.h can go wrong:

  cr_cos, cr_sin            the correctly rounded f64 value: mpmath at 320 bits rounded once (exactly: the mantissa and exponent go
                            through Python's correctly rounded int / int); without mpmath, the 70-digit decimal series that
                            tests/test_abi_and_host.py and tests/test_td_gradient_host.py use (decimal_cos, decimal_sin)
  f_entry, df_entry         numpy f64 operations in the reference's order, each rounded on its own, one cast to float32
  slow_path_cos / _sin      the header's fast-path predicate restated with math.cos / math.sin: True where the header must take the
                            double-double path; `ulps` moves the library value, the header's premise being a library within 2 ulp
  tie_inputs_cos / _sin     arguments whose EXACT a cos(t) + d (or ((-a) b) sin(t)) lies within ~2^-49 |a| of the midpoint of two
                            neighbouring float32s: the float then depends on the last bits of the cos
  near_tie_inputs           the same for a shipped row (a, b, c, d): w such that fl(fl(b w) + c) is next to such an argument
  hard_arguments            ~100,000 arguments of the bare cos / sin with |t| <= 2^20

Nothing here looks at the code under test."""
from __future__ import annotations

import math
from decimal import Decimal, localcontext

import numpy as np

try:
    import mpmath
except ImportError:                                          # the decimal series below then serves (a few times slower)
    mpmath = None

MP_BITS = 320
PI_100 = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899862803482534211706798")
DEC_PREC = 70


# ---------------------------------------------------------------------------------------------------------------------------------
# 70-digit decimal series (the reduction by pi/2 and the two Taylor series), as the two host tests have always carried them
def _decimal_trig(xf: float, sin: bool, eps_exp: int) -> Decimal:
    with localcontext() as ctx:
        ctx.prec = DEC_PREC
        X = Decimal(xf)
        k = (X / (PI_100 / 2)).to_integral_value()
        r = X - k * (PI_100 / 2)

        def series(start):
            t = Decimal(1) if start == 0 else r
            s, n = t, start
            while abs(t) > Decimal(10) ** -eps_exp:
                n += 2
                t = -t * r * r / (n * (n - 1))
                s += t
            return s
        if sin:
            return [series(1), series(0), -series(1), -series(0)][int(k) % 4]
        return [series(0), -series(1), -series(0), series(1)][int(k) % 4]


def decimal_cos(xf: float) -> Decimal:
    """cos(xf) to ~65 digits (finite xf)."""
    return _decimal_trig(float(xf), False, 65)


def decimal_sin(xf: float) -> Decimal:
    """sin(xf) to ~65 digits (finite xf)."""
    return _decimal_trig(float(xf), True, 80)


def _round_decimal(v: Decimal) -> float:
    return float(v)                                          # Python converts a Decimal through its exact digits: correctly rounded


def _round_mpf(v) -> float:
    """An mpmath number -> the nearest f64 (ties to even), subnormals included: Python's int -> float and int / int are both
    correctly rounded, so no assumption about mpmath's own float conversion is made."""
    sign, man, exp, _ = v._mpf_
    if man == 0:
        return 0.0
    man = int(man)
    r = float(man << exp) if exp >= 0 else man / (1 << -exp)
    return -r if sign else r


def _cr(t, sin: bool, backend: str | None):
    t = np.asarray(t, np.float64)
    out = np.empty(t.shape, np.float64)
    flat, o = t.ravel(), out.reshape(-1)
    backend = backend or ("mpmath" if mpmath is not None else "decimal")
    if backend == "mpmath":
        fn = mpmath.sin if sin else mpmath.cos
        with mpmath.workprec(MP_BITS):
            for i, v in enumerate(flat):
                v = float(v)
                if not math.isfinite(v):
                    o[i] = math.nan
                elif v == 0.0:
                    o[i] = v if sin else 1.0                 # sin keeps the sign of zero
                else:
                    o[i] = _round_mpf(fn(mpmath.mpf(v)))
    elif backend == "decimal":
        for i, v in enumerate(flat):
            v = float(v)
            if not math.isfinite(v):
                o[i] = math.nan
            elif v == 0.0:
                o[i] = v if sin else 1.0
            elif sin and abs(v) < 1e-30:
                o[i] = v                                     # sin v = v (1 - v^2/6 ...): rounds to v far below 2^-27; (the series' fixed
            else:                                            # absolute cut-off would not resolve a subnormal)
                o[i] = _round_decimal(_decimal_trig(v, sin, 80))
    else:
        raise ValueError(backend)
    return out if out.ndim else float(out)


def cr_cos(t, backend: str | None = None):
    """The correctly rounded f64 cos of every element of t (NaN for NaN / Inf)."""
    return _cr(t, False, backend)


def cr_sin(t, backend: str | None = None):
    return _cr(t, True, backend)


# ---------------------------------------------------------------------------------------------------------------------------------
def _libm(t, sin: bool):
    fn = math.sin if sin else math.cos
    t = np.asarray(t, np.float64)
    return np.fromiter((fn(v) if math.isfinite(v) else math.nan for v in t.ravel()), np.float64, t.size).reshape(t.shape)


def argument(b, w, c):
    """fl(fl(b w) + c): the argument as numpy forms it, the product and the sum rounded separately."""
    bw = np.asarray(b, np.float64) * np.asarray(w, np.float64)
    return bw + np.asarray(c, np.float64)


def f_from_cos(a, cosv, d):
    """float32(fl(fl(a cosv) + d)) for a given cos value."""
    ac = np.asarray(a, np.float64) * np.asarray(cosv, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(ac + np.asarray(d, np.float64)).astype(np.float32)


def df_from_sin(a, b, sinv):
    nab = (-np.asarray(a, np.float64)) * np.asarray(b, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(nab * np.asarray(sinv, np.float64)).astype(np.float32)


def f_entry(a, b, w, c, d):
    """float32(a cos(b w + c) + d), TD_Tester.py:25-28,37, with the cos correctly rounded."""
    return f_from_cos(a, cr_cos(argument(b, w, c)), d)


def df_entry(a, b, w, c):
    """float32(((-a) b) sin(b w + c)), TD_Tester.py:82, with the sin correctly rounded."""
    return df_from_sin(a, b, cr_sin(argument(b, w, c)))


def f_entry_libm(a, b, w, c, d):
    """The same entries with the host libm's cos / sin: what the reference and the oracles compute."""
    return f_from_cos(a, _libm(argument(b, w, c), False), d)


def df_entry_libm(a, b, w, c):
    return df_from_sin(a, b, _libm(argument(b, w, c), True))


def _moved(v, ulps: int):
    for _ in range(abs(ulps)):
        v = np.nextafter(v, np.inf if ulps > 0 else -np.inf)
    return v


def _predicate(scale, v):
    delta = (np.abs(scale) + np.abs(v)) * 2.0 ** -46
    return (v - delta).astype(np.float32) != (v + delta).astype(np.float32)


def slow_path_cos(a, t, d, ulps: int = 0):
    """True where cr_f32_a_cos_d must take the double-double path: (float)(v - delta) != (float)(v + delta), v = a cos(t) + d from the
    library cos (moved by `ulps` units in its last place), delta = (|a| + |v|) 2^-46."""
    a = np.asarray(a, np.float64)
    v = a * _moved(_libm(t, False), ulps) + np.asarray(d, np.float64)
    return _predicate(a, v)


def slow_path_sin(a, b, t, ulps: int = 0):
    nab = (-np.asarray(a, np.float64)) * np.asarray(b, np.float64)
    v = nab * _moved(_libm(t, True), ulps)
    return _predicate(nab, v)


# ---------------------------------------------------------------------------------------------------------------------------------
def _f32_midpoints(lo, hi, n, rng):
    """n midpoints (f64, exact) between a random float32 in [lo, hi] and its successor, and that float32."""
    f = rng.uniform(lo, hi, n).astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf))
    return (f.astype(np.float64) + up.astype(np.float64)) * 0.5, f


def _collect(n, draw, keep):
    """n inputs from draw(count) -> tuple of arrays, keeping the rows keep(*arrays) accepts: a draw that cannot give a tie is drawn
    again here, so that no test leaves an input out."""
    got, have = None, 0
    for _ in range(200):
        cand = draw(2 * n)
        ok = keep(*cand)
        cand = tuple(c[ok] for c in cand)
        got = cand if got is None else tuple(np.concatenate([g, c]) for g, c in zip(got, cand))
        have = len(got[0])
        if have >= n:
            return tuple(g[:n] for g in got)
    raise RuntimeError(f"only {have} of {n} tie inputs found")


def _fails_at_all_shifts(pred, *args):
    return pred(*args, ulps=0) & pred(*args, ulps=2) & pred(*args, ulps=-2)


def tie_inputs_cos(a: float, d: float, n: int, seed: int, kmax: int = 3):
    """(t f64[n], m f64[n]): a cos(t) + d is next to m, the midpoint of two neighbouring float32s in [d - |a|, d + |a|];
    t = +-acos((m - d) / a) + 2 pi k, |k| <= kmax, rounded to f64.  For the row (a, 1, 0, d), b w + c = w = t exactly."""
    rng = np.random.default_rng(seed)
    a, d = float(a), float(d)

    def draw(count):
        m, _ = _f32_midpoints(d - abs(a), d + abs(a), count, rng)
        q = (m - d) / a
        sign = rng.choice([-1.0, 1.0], count)
        k = rng.integers(-kmax, kmax + 1, count)
        with np.errstate(invalid="ignore"):
            t = sign * np.arccos(q) + 2.0 * np.pi * k
        return t, m

    def keep(t, m):
        with np.errstate(invalid="ignore"):
            inside = np.abs((m - d) / a) < 1.0
        t = np.where(inside, t, 1.0)
        return inside & _fails_at_all_shifts(slow_path_cos, np.full(len(t), a), t, np.full(len(t), d))
    return _collect(n, draw, keep)


def tie_inputs_sin(a: float, b: float, n: int, seed: int, kmax: int = 3):
    """(t f64[n], m f64[n]): ((-a) b) sin(t) is next to m, the midpoint of two neighbouring float32s in [-|a b|, |a b|];
    t = asin(m / nab) or its reflection pi - t, + 2 pi k, |k| <= kmax."""
    rng = np.random.default_rng(seed)
    nab = (-float(a)) * float(b)

    def draw(count):
        m, _ = _f32_midpoints(-abs(nab), abs(nab), count, rng)
        with np.errstate(invalid="ignore"):
            t = np.arcsin(m / nab)
        t = np.where(rng.integers(0, 2, count) == 1, np.pi - t, t)
        return t + 2.0 * np.pi * rng.integers(-kmax, kmax + 1, count), m

    def keep(t, m):
        inside = np.abs(m / nab) < 1.0
        t = np.where(inside, t, 1.0)
        return inside & _fails_at_all_shifts(slow_path_sin, np.full(len(t), float(a)), np.full(len(t), float(b)), t)
    return _collect(n, draw, keep)


def _best_w(b, c, t):
    """w next to (t - c) / b whose re-formed argument fl(fl(b w) + c) is closest to t (a few neighbours of the rounded quotient
    are tried: the quotient's own rounding moves the argument by up to a few of its ulps, more than a tie forgives)."""
    w0 = (t - c) / b
    best, err = w0, np.abs(argument(b, w0, c) - t)
    up, dn = w0, w0
    for _ in range(4):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        for cand in (up, dn):
            e = np.abs(argument(b, cand, c) - t)
            better = e < err
            best, err = np.where(better, cand, best), np.where(better, e, err)
    return best


def near_tie_inputs(row, n: int, seed: int, sin: bool = False, wmax: float = 3.0):
    """(w f64[n], m f64[n]) for a shipped row (a, b, c, d): the f entry (or, sin=True, the df entry) at w is next to the float32
    midpoint m.  w = (t - c) / b rounded, |w| <= wmax (the optimiser's domain); the argument the entry sees is fl(fl(b w) + c)."""
    a, b, c, d = (float(v) for v in row)
    rng = np.random.default_rng(seed)
    kmax = int(abs(b) * wmax / (2.0 * np.pi)) + 1

    def draw(count):
        if sin:
            t, m = tie_inputs_sin(a, b, count, int(rng.integers(1 << 30)), kmax)
        else:
            t, m = tie_inputs_cos(a, d, count, int(rng.integers(1 << 30)), kmax)
        return _best_w(b, c, t), m

    def keep(w, m):
        arg = argument(b, w, c)
        full = lambda v: np.full(len(w), v)
        if sin:
            fails = _fails_at_all_shifts(slow_path_sin, full(a), full(b), arg)
        else:
            fails = _fails_at_all_shifts(slow_path_cos, full(a), arg, full(d))
        return fails & (np.abs(w) <= wmax)
    return _collect(n, draw, keep)


# ---------------------------------------------------------------------------------------------------------------------------------
K_MAX = 667_543                                              # the largest k with k pi/2 <= 2^20


def nearest_k_half_pi(k) -> np.ndarray:
    """The doubles nearest k pi/2."""
    with localcontext() as ctx:
        ctx.prec = DEC_PREC
        return np.array([float(Decimal(int(v)) * PI_100 / 2) for v in np.asarray(k).ravel()], np.float64)


def hard_arguments(seed: int = 0) -> np.ndarray:
    """~100,000 arguments with |t| <= 2^20 for the bare cos / sin: uniform +-12; next to k pi/2, |k| <= 8, at offsets 2^-60..2^-2;
    log-uniform 2^-30..2^20 with both signs; the doubles nearest k pi/2 up to the reduction's limit; zeros, subnormals, +-2^20."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-12.0, 12.0, 30_000)]
    base = nearest_k_half_pi(np.arange(-8, 9))
    e = np.arange(2, 61)
    off = (2.0 ** -e)[None, :, None] * rng.uniform(1.0, 2.0, (17, len(e), 20)) * rng.choice([-1.0, 1.0], (17, len(e), 20))
    parts.append((base[:, None, None] + off).ravel())
    parts.append(2.0 ** rng.uniform(-30.0, 20.0, 30_000) * rng.choice([-1.0, 1.0], 30_000))
    k = np.concatenate([rng.integers(1, K_MAX + 1, 19_000), [1, 2, 3, 4, K_MAX - 1, K_MAX]])
    parts.append(nearest_k_half_pi(k) * rng.choice([-1.0, 1.0], len(k)))
    tiny = np.finfo(np.float64).tiny
    parts.append(np.array([0.0, -0.0, 5e-324, -5e-324, tiny / 2, -tiny / 2, tiny, -tiny, 2.0 ** 20, -2.0 ** 20,
                           np.nextafter(2.0 ** 20, 0.0), -np.nextafter(2.0 ** 20, 0.0)]))
    t = np.concatenate(parts)
    assert (np.abs(t) <= 2.0 ** 20).all()
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# the tie / near-tie sets the GPU tests feed to the device (and the host test checks from the reference alone)
N_TIE = 2005                                                 # 125 workgroups of 16 evaluations (501 of 4 gradients) and a partial one


def shipped_rows(art) -> np.ndarray:
    """f64[3 axes, 3 rows, 4]: the cosine rows (a, b, c, d) of yaw, pitch and roll."""
    return np.stack([art["optimized_yaw"][:3], art["optimized_pitch"][:3], art["optimized_roll"][:3]]).astype(np.float64)


def tie_cases_cos(art):
    """[(name, axis, row j, (a, b, c, d), w f64[N_TIE], m)]: exact ties for (a, 1, 0, d) with (a, d) of shipped rows -- the two with
    the largest |a| and |d| among them -- and (1, 0); near-ties for every shipped row with its own (b, c).  The (axis, j) a case is
    read out at covers the three axes and, on yaw, the three rows."""
    rows = shipped_rows(art)
    out = []
    for n, (axis, j, a, d) in enumerate([(0, 0, 1.0, 0.0), (0, 1, rows[0, 2, 0], rows[0, 2, 3]), (1, 2, rows[1, 2, 0], rows[1, 2, 3]),
                                         (2, 0, rows[2, 1, 0], rows[2, 1, 3]), (0, 2, rows[0, 0, 0], rows[0, 0, 3])]):
        t, m = tie_inputs_cos(a, d, N_TIE, seed=100 + n)
        out.append((f"tie-a{a:.3g}-d{d:.3g}", axis, j, (float(a), 1.0, 0.0, float(d)), t, m))
    for axis in range(3):
        for j in range(3):
            w, m = near_tie_inputs(rows[axis, j], N_TIE, seed=200 + 3 * axis + j)
            out.append((f"near-{'ypr'[axis]}{j}", axis, j, tuple(float(v) for v in rows[axis, j]), w, m))
    return out


def tie_cases_sin(art):
    """[(name, (a, b, c, d), w, m)] for the df read-out (rank 1, yaw row 0): exact ties of ((-a) b) sin(t) for a few (a, b) and
    near-ties of the nine shipped rows."""
    rows = shipped_rows(art)
    out = []
    for n, (a, b) in enumerate([(-1.0, 1.0), (rows[1, 2, 0], 1.0), (rows[2, 2, 0], rows[2, 2, 1])]):
        row = (float(a), float(b), 0.0, 0.0)
        if b == 1.0:
            t, m = tie_inputs_sin(a, b, N_TIE, seed=300 + n)                # b w + c = w = t exactly
        else:
            t, m = near_tie_inputs(row, N_TIE, seed=300 + n, sin=True)
        out.append((f"tie-a{a:.3g}-b{b:.3g}", row, t, m))
    for axis in range(3):
        for j in range(3):
            w, m = near_tie_inputs(rows[axis, j], N_TIE, seed=400 + 3 * axis + j, sin=True)
            out.append((f"near-{'ypr'[axis]}{j}", tuple(float(v) for v in rows[axis, j]), w, m))
    return out
