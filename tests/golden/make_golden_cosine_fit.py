#!/usr/bin/env python3
"""Generate tests/golden/fx13_cosine_fit.npz by running the reference's own TD_Trainer.

Run ONCE in the build container (needs the reference checkout and the built library; the GPU box has neither the reference nor a need
to run this):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cosine_fit.py

What is imported from the reference and called (file:line of the callee):
  FX13   TD_Trainer.py:150  estimate_init_Fourier_Trans   the Fourier start of the nine columns of the shipped factor matrices
         TD_Trainer.py:232  Train                         the nine fits; the scipy result objects Train's minimize calls return
                                                          (res.nfev, res.nit, res.status, res.fun) are recorded by wrapping the
                                                          `minimize` name the module calls
  FX13b  TD_Trainer.py:232  Train                         on the f32 factors that this package's numpy-backend decomposition gives for
                                                          the chain tensor of tests/cosine_fit_cases.py (8 synthetic identities)
Nothing of the reference's source is written to the fixture: it holds the numbers the reference returned and the library versions.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("NLML_REFERENCE", "/root/reference")
OUT = os.environ.get("NLML_GOLDEN_OUT", HERE)
# The reference first on sys.path; the repo root (which holds files named like the reference's modules) must not shadow it.
sys.path[:] = [p for p in sys.path if os.path.abspath(p or os.getcwd()) != REPO]
sys.path.insert(0, REF)
sys.path.insert(1, REPO)
sys.path.insert(2, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")

for _n in ("cv2", "mediapipe", "utils", "tensorly"):
    sys.modules.setdefault(_n, types.ModuleType(_n))


def _ref(name: str):
    """Import a module of the reference and make sure it IS the reference's file (not a same-named file of this repo)."""
    import importlib
    mod = importlib.import_module(name)
    path = os.path.abspath(getattr(mod, "__file__", "") or "")
    if not path.startswith(REF + os.sep):
        raise ImportError(f"{name} resolved to {path}, not to the reference under {REF}")
    return mod


def _train_recorded(TD_Trainer, pairs):
    """The reference's Train on three (U, w) pairs -> (optimized [3], the scipy results of its minimize calls in call order)."""
    results = []
    scipy_minimize = TD_Trainer.minimize

    def recording_minimize(*a, **k):
        res = scipy_minimize(*a, **k)
        results.append(res)
        return res

    TD_Trainer.minimize = recording_minimize
    try:
        with np.errstate(all="ignore"):
            optimized = TD_Trainer.Train(*pairs)
    finally:
        TD_Trainer.minimize = scipy_minimize
    return optimized, results


def fx13_cosine_fit():
    import scipy

    import cosine_fit_cases as CC
    from nlml_hpe_amd import tucker_decompose as TD
    TD_Trainer = _ref("TD_Trainer")

    fm = np.load(os.path.join(REF, "outputs/features/Factor_Matrices.npz"))
    pairs = [(fm[f"U_{a}"], CC.BINS[a]) for a in CC.AXES]
    guess = TD_Trainer.estimate_init_Fourier_Trans(*pairs)
    optimized, results = _train_recorded(TD_Trainer, pairs)
    assert len(results) == 9
    out = {"numpy_version": np.array(np.__version__), "scipy_version": np.array(scipy.__version__)}
    for a, g, o in zip(CC.AXES, guess, optimized):
        out[f"guess_{a}"] = np.asarray(g, np.float64)
        out[f"optimized_{a}"] = np.asarray(o, np.float64)
    out["nfev"] = np.array([r.nfev for r in results], np.int32)
    out["nit"] = np.array([r.nit for r in results], np.int32)
    out["status"] = np.array([r.status for r in results], np.int32)          # scipy's own codes: 0 converged, 1 maxfev, 2 maxiter, 3 NaN
    out["fun"] = np.array([float(r.fun) for r in results], np.float64)
    print("FX13 nfev", out["nfev"], "status", out["status"])

    # FX13b: the chain tensor, the numpy-backend decomposition, the f32 factors as the npz holds them, the reference's Train
    X = CC.chain_tensor_host()
    r = CC.CHAIN_CONFIG["tensor_decom_ranks"]
    rank = [r["R_identity"], r["R_yaw"], r["R_pitch"], r["R_roll"], r["R_features"]]
    _, factors = TD.tucker(X, rank, backend="numpy")
    f32 = [np.asarray(u, np.float32) for u in factors]
    pairs_b = [(f32[1 + k], CC.BINS[a]) for k, a in enumerate(CC.AXES)]
    optimized_b, results_b = _train_recorded(TD_Trainer, pairs_b)
    for k, (a, o) in enumerate(zip(CC.AXES, optimized_b)):
        out[f"b_optimized_{a}"] = np.asarray(o, np.float64)
        out[f"b_U_{a}"] = f32[1 + k]
    out["b_nfev"] = np.array([r_.nfev for r_ in results_b], np.int32)
    out["b_status"] = np.array([r_.status for r_ in results_b], np.int32)
    print("FX13b nfev", out["b_nfev"], "status", out["b_status"])
    np.savez_compressed(os.path.join(OUT, "fx13_cosine_fit.npz"), **out)


if __name__ == "__main__":
    fx13_cosine_fit()
