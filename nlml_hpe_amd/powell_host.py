"""Host-side driver of the Powell state machine (nlml_hpe_amd/csrc/powell.h) -- no GPU involved.

``minimize_powell(fun, x0)`` steps the same machine the device kernel runs, calling a Python
objective at each suspend point.  It exists so the restated control flow can be compared with
scipy.optimize.minimize(method='Powell') on the CPU (tests/test_powell_sm.py); the product path for
TD inference is the device kernel (ops.tucker_powell).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import _lib

STATUS = {0: "running", 1: "converged", 2: "maxfev", 3: "maxiter", 4: "nan"}


def minimize_powell(fun, x0, xtol: float = 1e-4, ftol: float = 1e-4, record: list | None = None,
                    rank_aware: bool = False):
    """x0 f64[8]: the 8-parameter machine of the shipped artefacts (nlml_powell_init/step/result); any other length n = 3 + R,
    R = 1..16 -- or rank_aware=True at 8 too: the rank-aware machine the device runs for that identity rank (the _n forms; scipy's
    limits follow n)."""
    L = _lib.lib()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    n = x0.shape[0] if x0.ndim == 1 else 0
    if not 3 + _lib.TUCKER_RANK_MIN <= n <= 3 + _lib.TUCKER_RANK_MAX:
        raise ValueError(f"the state machine takes 3 + R parameters for an identity rank R in [{_lib.TUCKER_RANK_MIN}, "
                         f"{_lib.TUCKER_RANK_MAX}], got shape {x0.shape}")
    if n == 8 and not rank_aware:
        state = C.create_string_buffer(L.nlml_powell_state_bytes())
        _lib.check(L.nlml_powell_init(state, x0.ctypes.data_as(C.c_void_p), xtol, ftol), "nlml_powell_init")
        step, result = L.nlml_powell_step, L.nlml_powell_result
    else:
        state = C.create_string_buffer(L.nlml_powell_state_bytes_n(n))
        _lib.check(L.nlml_powell_init_n(state, n, x0.ctypes.data_as(C.c_void_p), xtol, ftol), "nlml_powell_init_n")
        step, result = L.nlml_powell_step_n, L.nlml_powell_result_n
    xe = np.empty(n, dtype=np.float64)
    f = 0.0
    while step(state, C.c_double(f), xe.ctypes.data_as(C.c_void_p)) == 1:
        if record is not None:
            record.append(xe.copy())
        f = float(fun(xe.copy()))
    x = np.empty(n)
    fval, nfev, nit, status = C.c_double(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(result(state, x.ctypes.data_as(C.c_void_p), C.byref(fval), C.byref(nfev), C.byref(nit),
                                    C.byref(status)), "nlml_powell_result")
    return SimpleNamespace(x=x, fun=fval.value, nfev=nfev.value, nit=nit.value, status=status.value,
                           message=STATUS.get(status.value, "?"))
