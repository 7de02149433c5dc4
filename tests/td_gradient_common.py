"""Test helper of tests/test_td_gradient_host.py and tests/test_td_gradient_gpu.py: K3g's host restatement through ctypes, and the
inputs both files check it on (FX9 = the FX4 inputs at rank 5, FX10 at ranks 1, 3 and 8, synthetic draws against oracle.tucker)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import rank_fixture as RF
from nlml_hpe_amd import _lib, synth

F = 1404
N_DRAWS = 200                      # oracle draws per rank
DRAW_RANKS = (1, 5, 16)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def gradient_host(Wm, X, P, cp, x_index=None, ldx=None, want_v=False):
    """nlml_tucker_gradient_host -> (err f64[N], grad f64[N,3+R][, v f32[N,1404]])."""
    Wm = np.ascontiguousarray(Wm, np.float32).reshape(-1, F)
    R = Wm.shape[0] // 27
    X = np.ascontiguousarray(X, np.float32)
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3 + R)
    cp = np.ascontiguousarray(cp, np.float64)
    xi = None if x_index is None else np.ascontiguousarray(x_index, np.int32)
    N = len(P)
    err, grad = np.full(N, np.nan), np.full((N, 3 + R), np.nan)
    v = np.full((N, F), np.nan, np.float32) if want_v else None
    rc = _lib.lib().nlml_tucker_gradient_host(_p(Wm), _p(X), ldx or X.shape[-1], _p(xi), _p(P), _p(cp), N, _p(err), _p(grad), R, _p(v))
    _lib.check(rc, "nlml_tucker_gradient_host")
    return (err, grad, v) if want_v else (err, grad)


def cos_block(art):
    return np.stack(RF.cos_rows(art))


def fx9_inputs(art, golden_dir):
    """(W f32[5,3,3,3,1404], params, x, reference gradient, reference objective) of FX9 / FX4."""
    f = np.load(os.path.join(golden_dir, "fx4_td_objective.npz"))
    g = np.load(os.path.join(golden_dir, "fx9_td_gradient.npz"))["grad"]
    n = len(g)
    return np.asarray(art["W"], np.float32), f["params"][:n], f["x"][:n], g, f["err"][:n]


def fx10_inputs(art, golden_dir, R):
    fx = np.load(os.path.join(golden_dir, "fx10_td_identity_rank.npz"))
    W = RF.rank_W(art["W"], R)
    P, X = RF.params(R)[:RF.N_GRAD], RF.noisy_faces(art, R, RF.N_PARAMS)[:RF.N_GRAD]
    return W, P, X, fx[f"r{R}_grad"], fx[f"r{R}_err"][:RF.N_GRAD]


def draws(art, R, n=N_DRAWS):
    """(W, params, faces) of the oracle comparison: synth.tucker_params draws on synth.tucker_grid_faces rows of the rank-R model."""
    W = RF.rank_W(art["W"], R)
    a = dict(art)
    a["W"], a["U_id"] = W, RF.rank_U_id(art["U_id"], R)
    P = synth.tucker_params(n, R, seed=40 + R)
    X = synth.tucker_grid_faces(a, synth.tucker_grid_indices(n, seed=40 + R), seed=40 + R)
    return W, P, X
