"""Test helper for the cosine fit (K8, nlml_hpe_amd/csrc/cosine_fit_ref.h / cosine_fit.hip): the oracle, scipy's real Powell with a
recorder, the columns the tests fit, and the chain's tensor.  No test here.

THE ORACLE shares no code with the header: ``objective_py`` is the objective in Python floats (IEEE f64, one rounding per operation,
no fused multiply-add) with the cos from multi-precision arithmetic rounded once (tests/cr_reference.cr_cos) and the square as
e * e, in the order the issue states:

    wr_i = w_i * 0.017453292519943295;  t_i = b wr_i + c;  m_i = a cos(t_i) + d;  e_i = y_i - m_i;  q_i = e_i e_i;
    s = ((0 + q_0) + q_1) + ...;  value = s / 2

``scipy_powell`` runs scipy.optimize.minimize(method='Powell') itself over a given objective and records every visited point.

The library wrappers (host_objective, host_fit) only marshal arrays for the *_host entry points.
"""
from __future__ import annotations

import functools
import os

import numpy as np

import cr_reference as CR
from nlml_hpe_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAW = np.arange(-50, 51, 10)        # configs/config_TD_main.yaml
PITCH = np.arange(-40, 41, 10)
ROLL = np.arange(-30, 31, 10)
BINS = {"yaw": YAW, "pitch": PITCH, "roll": ROLL}
AXES = ("yaw", "pitch", "roll")
OUTPUTS = ("x", "fun", "nfev", "nit", "status")
DEG2RAD = 0.017453292519943295
PW_CONVERGED, PW_MAXFEV, PW_MAXITER, PW_NAN = 1, 2, 3, 4     # powell.h; scipy's res.status + 1
MAXFEV = 4000                                                 # scipy's 1000 n for n = 4 parameters
NAN_NFEV = 1 + 3 * 4                                          # powell.h: the start, then three bracket points along each direction
CHEAPEST = ("yaw1", "roll2", "pitch1")                       # the three shipped columns with the fewest evaluations


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    """Bit for bit, except that any NaN equals any NaN (two libraries' NaNs may differ in sign and payload)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float64:
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0.0, a)), bits(np.where(nb, 0.0, b))))
    return bool(np.array_equal(a, b))


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def objective_py(p, y, w_deg):
    a, b, c, d = (float(v) for v in p)
    t = [b * (float(w) * DEG2RAD) + c for w in w_deg]
    cosv = np.atleast_1d(CR.cr_cos(np.array(t, np.float64)))
    s = 0.0
    for yi, ci in zip(y, cosv):
        e = float(yi) - (a * float(ci) + d)
        s = s + e * e
    return s / 2.0


def scipy_powell(fun, x0, **options):
    """scipy's own minimize(method='Powell') over fun -> (res, visited f64[nfev,4], values f64[nfev])."""
    from scipy.optimize import minimize

    visited, values = [], []

    def recording(p):
        v = fun(p)
        visited.append(np.array(p, np.float64))
        values.append(v)
        return v
    res = minimize(recording, np.array(x0, np.float64), method="Powell", options=options or None)
    return res, np.array(visited).reshape(-1, 4), np.array(values, np.float64)


def scipy_outputs(res):
    return {"x": np.array(res.x, np.float64), "fun": np.float64(res.fun), "nfev": np.int32(res.nfev), "nit": np.int32(res.nit),
            "status": np.int32(res.status + 1)}


# ---- the library's host forms -----------------------------------------------------------------------------------------------------
def host_objective(y, w_deg, params):
    y, w = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(w_deg, np.float64)
    P = np.ascontiguousarray(params, np.float64).reshape(-1, 4)
    out = np.full(P.shape[0], 7.0)
    rc = _lib.lib().nlml_cosine_fit_objective_host(y.ctypes.data, w.ctypes.data, y.shape[0], P.ctypes.data, P.shape[0], out.ctypes.data)
    assert rc == 0, _lib.lib().nlml_last_error()
    return out


def pack(cols, ld=None):
    """[(y [n], w [n])] -> y f64[C,ld], w f64[C,ld] (the padding holds NaN: a kernel that read it would show), n i32[C]."""
    n = np.array([len(c[0]) for c in cols], np.int32)
    ld = int(ld if ld is not None else max(n.max(initial=1), 1))
    Y, W = np.full((len(cols), ld), np.nan), np.full((len(cols), ld), np.nan)
    for f, (y, w) in enumerate(cols):
        Y[f, :len(y)], W[f, :len(w)] = y, w
    return Y, W, n


def host_fit(cols, x0, ld=None, xtol=1e-4, ftol=1e-4):
    """nlml_cosine_fit_host on [(y, w)] -> dict of OUTPUTS."""
    Y, W, n = pack(cols, ld)
    X0 = np.ascontiguousarray(x0, np.float64).reshape(len(cols), 4)
    out = {"x": np.full((len(cols), 4), 7.0), "fun": np.full(len(cols), 7.0), "nfev": np.full(len(cols), -7, np.int32),
           "nit": np.full(len(cols), -7, np.int32), "status": np.full(len(cols), -7, np.int32)}
    rc = _lib.lib().nlml_cosine_fit_host(Y.ctypes.data, W.ctypes.data, Y.shape[1], n.ctypes.data, len(cols), X0.ctypes.data, xtol, ftol,
                                         *[out[k].ctypes.data for k in OUTPUTS])
    assert rc == 0, _lib.lib().nlml_last_error()
    return out


# ---- columns ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shipped():
    """The shipped artefacts: (factors {axis: f32[bins,3]}, optimized {axis: f64[3,4]})."""
    fm = np.load(os.path.join(REPO, "outputs", "features", "Factor_Matrices.npz"))
    td = np.load(os.path.join(REPO, "outputs", "features", "Trained_data.npz"))
    return {a: fm[f"U_{a}"] for a in AXES}, {a: td[f"optimized_{a}"] for a in AXES}


def shipped_pairs():
    U, _ = shipped()
    return [(U[a], BINS[a]) for a in AXES]


def shipped_columns():
    """name -> (y f64[n], w f64[n]) for the nine columns, yaw0 .. roll2: the order of a Train launch."""
    U, _ = shipped()
    return {f"{a}{j}": (U[a][:, j].astype(np.float64), BINS[a].astype(np.float64)) for a in AXES for j in range(3)}


@functools.lru_cache(maxsize=None)
def shipped_guess():
    """f64[9,4]: the package's own Fourier start of the nine columns (tests compare it with the reference's recorded one)."""
    from nlml_hpe_amd import TD_Trainer
    return np.concatenate(TD_Trainer.estimate_init_Fourier_Trans(*shipped_pairs()))


def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "fx13_cosine_fit.npz"))


def random_column(n, seed, noise=0.02):
    """A noisy cosine on n uniform bins -> (y f64[n] of f32 values, w f64[n])."""
    rng = np.random.default_rng(seed)
    w = np.linspace(-50.0, 50.0, n) if n > 1 else np.array([10.0])
    a, b, c, d = rng.uniform(0.2, 0.6), rng.uniform(0.6, 1.6), rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3)
    y = a * np.cos(b * np.radians(w) + c) + d + noise * rng.normal(size=n)
    return y.astype(np.float32).astype(np.float64), w


def random_start(seed):
    rng = np.random.default_rng(seed)
    return np.array([rng.uniform(0.1, 0.8), rng.uniform(0.5, 2.0), rng.uniform(-1.0, 1.0), rng.uniform(-0.5, 0.5)])


def random_params(count, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-1, 1, count), rng.uniform(-3, 3, count), rng.uniform(-3, 3, count), rng.uniform(-1, 1, count)], axis=1)


def edge_columns():
    """name -> ((y, w), x0): the columns that take the machine off its happy path."""
    y, w = shipped_columns()["yaw1"]
    g = shipped_guess()
    ynan, yinf, winf = y.copy(), y.copy(), w.copy()
    ynan[3] = np.nan
    yinf[5] = np.inf
    winf[7] = np.inf
    out = {
        # a NaN sample or an infinite angle (cos(Inf) = NaN): the objective is NaN everywhere, status 4 after NAN_NFEV evaluations
        "nan": ((ynan, w), g[1]),
        "inf_angle": ((y, winf), g[1]),
        # an infinite SAMPLE makes the objective the constant +Inf, not NaN: scipy (and the machine) walk on to maxfev
        "inf": ((yinf, w), g[1]),
        "constant": ((np.full(9, 0.25), PITCH.astype(np.float64)), np.array([0.1, 1.0, 0.0, 0.0])),
        "maxfev": (shipped_columns()["yaw2"], g[2]),
        "one_row": (random_column(1, 5), np.array([0.3, 1.0, 0.1, 0.0])),
        "rows64": (random_column(64, 6), random_start(6)),
    }
    return out


def batch(count, seed=0):
    """count distinct small fits of mixed row counts -> ([(y, w)], x0 f64[count,4])."""
    cols = [random_column(3 + (i * 5 + seed) % 9, 1000 * seed + i) for i in range(count)]
    return cols, np.stack([random_start(1000 * seed + i) for i in range(count)])


# ---- the chain's tensor ------------------------------------------------------------------------------------------------------------
CHAIN_I = 8
CHAIN_CONFIG = {
    "tensor_decom_ranks": {"R_identity": 5, "R_yaw": 3, "R_pitch": 3, "R_roll": 3, "R_features": 1404},
    "yaw_bins": {"min_bin": -50, "max_bin": 51, "interval": 10},
    "pitch_bins": {"min_bin": -40, "max_bin": 41, "interval": 10},
    "roll_bins": {"min_bin": -30, "max_bin": 31, "interval": 10},
}
CHAIN_CELLS = 16


def chain_base():
    """f32[8,468,3]: eight synthetic identities (tucker_cases.base_landmarks: a mean face plus identity modes)."""
    import tucker_cases as TC
    return TC.base_landmarks(CHAIN_I, 468, seed=13)


def chain_tensor_host():
    """The chain's tensor f32[8,11,9,7,1404] from the host form of K6 (the device's bits, tests/test_rotation_gpu.py)."""
    from nlml_hpe_amd import IntrinsicRotation as IR
    base = np.ascontiguousarray(chain_base(), np.float32)
    t = [np.ascontiguousarray(IR.rotation_matrices(ax, v), np.float64) for ax, v in (("y", YAW), ("x", PITCH), ("z", ROLL))]
    shape = (CHAIN_I, len(YAW), len(PITCH), len(ROLL), 1404)
    out = np.zeros(shape, np.float32)
    zero = [int(np.where(v == 0)[0][0]) for v in (YAW, PITCH, ROLL)]
    rc = _lib.lib().nlml_compose_rotation_tensor_host(base.ctypes.data, shape[0], t[0].ctypes.data, shape[1], t[1].ctypes.data, shape[2],
                                                      t[2].ctypes.data, shape[3], _lib.ROT_INTRINSIC, *zero, out.ctypes.data, None)
    assert rc == 0, _lib.lib().nlml_last_error()
    return out


def chain_cells():
    """i64[16,4]: (identity, yaw bin, pitch bin, roll bin) of the grid cells the chain test estimates, and their poses in degrees."""
    rng = np.random.default_rng(17)
    idx = np.stack([rng.integers(0, s, CHAIN_CELLS) for s in (CHAIN_I, len(YAW), len(PITCH), len(ROLL))], axis=1)
    deg = np.stack([YAW[idx[:, 1]], PITCH[idx[:, 2]], ROLL[idx[:, 3]]], axis=1).astype(np.float64)
    return idx, deg
