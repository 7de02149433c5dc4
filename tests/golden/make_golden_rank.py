#!/usr/bin/env python3
"""Generate tests/golden/fx10_td_identity_rank.npz by running the reference's own Python at identity ranks other than 5.

Run ONCE in the build container (needs /root/reference; the GPU box has neither the reference nor a need to run this):

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rank.py

What is imported from /root/reference and called (file:line of the callee):
  FX10 TD_Tester.py:31   objective           32 parameter sets per rank (and the same einsum for x_hat of the first 8)
       TD_Tester.py:60   compute_gradient    the first 8 parameter sets per rank
       TD_Tester.py:162  Test (scipy Powell) four clean grid faces per rank; the scipy result object Test builds (res.x, res.fun,
                                             res.nfev) is recorded by wrapping the `minimize` name Test calls
for the ranks of tests/rank_fixture.py: R = 1 and 3 (W[:R], the slicing TD_Inference.py:54-55 names) and R = 8 (W plus three
synthetic identity slices from a fixed seed; the fixture stores the seed and a checksum of the slices, not the slices).
Nothing of the reference's source is written to the fixture: it holds seeds and the numbers the reference returned.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.environ.get("NLML_GOLDEN_OUT", HERE)      # where the fixture is written (the regeneration test uses a temp dir)
# The reference first on sys.path; the repo root (which holds files named like the reference's modules) must not shadow it.
sys.path[:] = [p for p in sys.path if os.path.abspath(p or os.getcwd()) != REPO]
sys.path.insert(0, REF)
sys.path.insert(1, REPO)
sys.path.insert(2, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")

for _n in ("cv2", "mediapipe", "utils", "tensorly"):
    sys.modules.setdefault(_n, types.ModuleType(_n))

import torch  # noqa: E402

import rank_fixture as RF  # noqa: E402


def _ref(name: str):
    """Import a module of the reference and make sure it IS the reference's file (not a same-named file of this repo)."""
    import importlib
    mod = importlib.import_module(name)
    path = os.path.abspath(getattr(mod, "__file__", "") or "")
    if not path.startswith(REF + os.sep):
        raise ImportError(f"{name} resolved to {path}, not to the reference under {REF}")
    return mod


def fx10_td_identity_rank(ranks=RF.RANKS):
    TD_Tester = _ref("TD_Tester")
    import scipy
    td = np.load(os.path.join(REF, "outputs/features/Trained_data.npz"))
    fm = np.load(os.path.join(REF, "outputs/features/Factor_Matrices.npz"))
    art = {"W": td["W"], "U_id": fm["U_id"], "U_yaw": fm["U_yaw"], "U_pitch": fm["U_pitch"], "U_roll": fm["U_roll"],
           "optimized_yaw": td["optimized_yaw"], "optimized_pitch": td["optimized_pitch"], "optimized_roll": td["optimized_roll"]}
    Py, Pp, Pr = RF.cos_rows(art)

    results = []
    scipy_minimize = TD_Tester.minimize

    def recording_minimize(*a, **k):
        res = scipy_minimize(*a, **k)
        results.append(res)
        return res

    TD_Tester.minimize = recording_minimize
    out = {"seed": np.array(RF.SEED), "ranks": np.array(ranks), "picks": np.array(RF.PICKS),
           "scipy_version": np.array(scipy.__version__)}
    try:
        for R in ranks:
            W = RF.rank_W(art["W"], R)
            if R > 5:
                out[f"r{R}_slices_sha256"] = np.array(RF.slices_checksum(W[5:]))
            P = RF.params(R)
            X = RF.noisy_faces(art, R, RF.N_PARAMS)
            err = np.empty(RF.N_PARAMS)
            xh = np.empty((RF.N_XHAT, 1404))
            grad = np.empty((RF.N_GRAD, 3 + R))
            for i in range(RF.N_PARAMS):
                err[i] = TD_Tester.objective(P[i], W, torch.from_numpy(X[i]), Py, Pp, Pr)
                if i < RF.N_XHAT:
                    f_y = np.array([TD_Tester.func(P[i][0], p) for p in Py]).flatten().astype(np.float32)
                    f_p = np.array([TD_Tester.func(P[i][1], p) for p in Pp]).flatten().astype(np.float32)
                    f_r = np.array([TD_Tester.func(P[i][2], p) for p in Pr]).flatten().astype(np.float32)
                    xh[i] = np.einsum('ijklm,i,j,k,l->m', W, P[i][3:], f_y, f_p, f_r)      # TD_Tester.py:46
                if i < RF.N_GRAD:
                    grad[i] = TD_Tester.compute_gradient(P[i], W, torch.from_numpy(X[i]), Py, Pp, Pr)
            faces = RF.grid_faces(art, R)
            deg, res_x, res_fun, nfev = [], [], [], []
            for x in faces:
                del results[:]
                y, p, r, _ = TD_Tester.Test(W, torch.from_numpy(x), R, Py, Pp, Pr, None, None, None, None)
                res = results[-1]
                deg.append((y, p, r)); res_x.append(np.array(res.x, np.float64)); res_fun.append(float(res.fun)); nfev.append(int(res.nfev))
                print(f"FX10 R={R}", (y, p, r), "nfev", nfev[-1], "fun", res_fun[-1])
            out.update({f"r{R}_err": err, f"r{R}_x_hat": xh, f"r{R}_grad": grad, f"r{R}_deg": np.array(deg),
                        f"r{R}_res_x": np.stack(res_x), f"r{R}_res_fun": np.array(res_fun), f"r{R}_nfev": np.array(nfev)})
            print(f"FX10 R={R} err range", err.min(), err.max())
    finally:
        TD_Tester.minimize = scipy_minimize
    np.savez_compressed(os.path.join(OUT, "fx10_td_identity_rank.npz"), **out)


if __name__ == "__main__":
    fx10_td_identity_rank()
