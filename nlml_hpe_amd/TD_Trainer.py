"""The cosine fit of the three pose factors (the reference's TD_Trainer.py), on the device.

The reference's ``Train`` fits every column of U_yaw, U_pitch and U_roll by  a cos(b radians(w) + c) + d  over the angle bins w:
a Fourier initial guess per column, then scipy's Powell over (a, b, c, d) on an interpreted least-squares objective.  Here the
guess stays on the host (nine tiny FFTs) and all the minimisations go to the GPU as ONE launch of K8 (ops.cosine_fit,
csrc/cosine_fit.hip): one wave per column, the whole Powell run inside the kernel.  The reference's function names are kept so
that a caller of the reference's module finds them here.

The objective is the reference's in its own f64 operation order, with np.cos and the scalar ``** 2`` -- neither correctly rounded
in glibc -- replaced by their correctly rounded values (csrc/cosine_fit_ref.h).  The end points therefore agree with a run of the
reference to the distance between two hosts' runs of the reference itself (a few 1e-8), not bit for bit.

``backend="host"`` runs the same header on the CPU (nlml_cosine_fit_host): the same bits as the device, no GPU involved.

The reference's Taylor-series guess (TD_Trainer.py:164-229) is computed and discarded there; it is not part of this module.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def func(w_i, a_j, b_j, c_j, d_j):
    """The model a cos(b w + c) + d at the angle w_i in radians (TD_Trainer.py:25-34)."""
    return a_j * np.cos(b_j * w_i + c_j) + d_j


def objective(params, U_j, w):
    """1/2 sum_i (U_j[i] - func(radians(w[i]), *params))^2 through the library's host objective (csrc/cosine_fit_ref.h): the value
    the fits minimise.  U_j the column, w its bins in degrees."""
    y = np.ascontiguousarray(U_j, dtype=np.float64)
    wd = np.ascontiguousarray(w, dtype=np.float64)
    p = np.ascontiguousarray(params, dtype=np.float64).reshape(1, 4)
    if y.ndim != 1 or wd.shape != y.shape:
        raise ValueError(f"U_j and w: expected two vectors of one length, got {y.shape}, {wd.shape}")
    out = np.empty(1, np.float64)
    _lib.check(_lib.lib().nlml_cosine_fit_objective_host(y.ctypes.data, wd.ctypes.data, y.shape[0], p.ctypes.data, 1, out.ctypes.data),
               "nlml_cosine_fit_objective_host")
    return float(out[0])


def est_params_by_Uniform_Fourier(U, w):
    """The start (a, b, c, d) of every column of U [n, cols] on the uniform bins w (degrees): the strongest non-constant bin of the
    column's discrete Fourier transform gives the angular frequency b, its phase c and twice its modulus over n the amplitude a; d
    is the column's mean (TD_Trainer.py:125-148).  The transform is scipy.fft's on the column IN THE DTYPE IT ARRIVES IN (the
    shipped factors are f32 and scipy keeps single precision; numpy's fft would upcast and give other bits)."""
    from scipy.fft import fft

    U = np.asarray(U)
    step = np.radians(w)
    step = step[1] - step[0]
    n = U.shape[0]
    freqs = np.fft.fftfreq(n, d=step)
    guess = np.zeros((U.shape[1], 4))
    for j in range(U.shape[1]):
        column = U[:, j]
        spectrum = fft(column)
        k = int(np.argmax(np.abs(spectrum[1:]))) + 1
        guess[j] = [2 * np.abs(spectrum[k]) / n, 2 * np.pi * np.abs(freqs[k]), np.angle(spectrum[k]), np.mean(column)]
    return guess


def estimate_init_Fourier_Trans(yaw_params, pitch_params, roll_params):
    """(guess_yaw, guess_pitch, guess_roll) for the three (U, w) pairs (TD_Trainer.py:150-159)."""
    return tuple(est_params_by_Uniform_Fourier(U, w) for U, w in (yaw_params, pitch_params, roll_params))


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _pack(problems):
    """[(U [n,cols], w [n], guess [cols,4])] -> y f64[C,ld], w_deg f64[C,ld], n i32[C], x0 f64[C,4]: one row per column."""
    cols = [(np.asarray(U[:, j], dtype=np.float64), np.asarray(w, dtype=np.float64), g[j]) for U, w, g in problems for j in range(U.shape[1])]
    for yv, wv, _ in cols:
        if yv.shape != wv.shape:
            raise ValueError(f"a factor with {yv.shape[0]} rows next to {wv.shape[0]} bins")
        if not 1 <= yv.shape[0] <= _lib.COSINE_FIT_ROWS_MAX:
            raise ValueError(f"a factor with {yv.shape[0]} rows: the fit takes 1..{_lib.COSINE_FIT_ROWS_MAX}")
    ld = max((c[0].shape[0] for c in cols), default=1)
    y = np.zeros((len(cols), ld))
    wd = np.zeros((len(cols), ld))
    for f, (yv, wv, _) in enumerate(cols):
        y[f, :yv.shape[0]] = yv                      # f32 -> f64: exact
        wd[f, :wv.shape[0]] = wv
    n = np.array([c[0].shape[0] for c in cols], np.int32)
    x0 = np.array([c[2] for c in cols], np.float64).reshape(len(cols), 4)
    return y, wd, n, x0


def fit_columns(problems, backend="device", xtol=1e-4, ftol=1e-4, device=None):
    """All columns of [(U, w, guess)] as one batch -> dict(x f64[C,4], fun, nfev, nit, status) of numpy arrays, columns in order.
    backend "device": one launch of K8 on the GPU; "host": nlml_cosine_fit_host."""
    if backend not in ("device", "host"):
        raise ValueError(f"backend: expected 'device' or 'host', got {backend!r}")
    y, wd, n, x0 = _pack(problems)
    Cn, ld = y.shape
    if backend == "device":
        import torch

        from . import ops
        dev = torch.device(device) if device is not None else torch.device("cuda")
        res = ops.cosine_fit(torch.from_numpy(y).to(dev), torch.from_numpy(wd).to(dev), torch.from_numpy(n), torch.from_numpy(x0).to(dev),
                             xtol=xtol, ftol=ftol)
        return {k: v.cpu().numpy() for k, v in res.items()}
    out = {"x": np.zeros((Cn, 4)), "fun": np.zeros(Cn), "nfev": np.zeros(Cn, np.int32), "nit": np.zeros(Cn, np.int32),
           "status": np.zeros(Cn, np.int32)}
    _lib.check(_lib.lib().nlml_cosine_fit_host(y.ctypes.data, wd.ctypes.data, ld, n.ctypes.data, Cn, x0.ctypes.data, float(xtol), float(ftol),
                                               *[out[k].ctypes.data for k in ("x", "fun", "nfev", "nit", "status")]),
               "nlml_cosine_fit_host")
    return out


def optimize_for_matrix_using_grads(U_matrix, w_vector, initial_guesses, backend="device"):
    """The fitted (a, b, c, d) of every column of U_matrix, f64[cols,4] (TD_Trainer.py:70-93; despite the name the reference's
    Powell uses no gradient, and neither does this)."""
    U = _host(U_matrix)
    return fit_columns([(U, _host(w_vector), np.asarray(initial_guesses, np.float64))], backend=backend)["x"]


def Train(yaw_params, pitch_params, roll_params, backend="device", return_info=False):
    """(optimized_yaw, optimized_pitch, optimized_roll), each f64[cols,4], for the three (U, w) pairs: U [bins, cols] a pose factor
    (numpy or torch, any float dtype), w its bins in degrees (TD_Trainer.py:232-351).  All columns are fitted in one launch.
    return_info: also the dict of fit_columns (fun, nfev, nit, status per column, yaw's columns first)."""
    pairs = [(_host(U), _host(w)) for U, w in (yaw_params, pitch_params, roll_params)]
    guesses = estimate_init_Fourier_Trans(*pairs)
    res = fit_columns([(U, w, g) for (U, w), g in zip(pairs, guesses)], backend=backend)
    cuts = np.cumsum([U.shape[1] for U, _ in pairs])[:-1]
    out = tuple(np.split(res["x"], cuts))
    return out + (res,) if return_info else out
