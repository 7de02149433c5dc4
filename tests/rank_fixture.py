"""Test helper: the W tensors, faces and parameter sets of FX10 (tests/golden/fx10_td_identity_rank.npz) for an identity rank R.

  R <= 5   W[:R] and U_id[:, :R] -- the slicing the reference itself names (TD_Inference.py:54-55);
  R  > 5   W plus R - 5 synthetic identity slices: N(0, 1) from a fixed Philox stream, scaled element by element to the mean
           magnitude of W's own five slices, rounded to f32; the identity coordinates of a face get R - 5 more entries of the
           U_id columns' typical size.  The fixture stores the seed and a checksum of the slices, not the slices.
Everything here is deterministic data preparation; the numbers a test compares against come from the reference (FX10) or from
oracle.tucker.
"""
from __future__ import annotations

import hashlib

import numpy as np

from nlml_hpe_amd import synth

SEED = 1010                       # Philox key of everything synthetic in FX10
RANKS = (1, 3, 8)                 # the fixture's ranks
PICKS = ((100, 7, 2, 4), (0, 5, 4, 3), (700, 0, 8, 6), (1500, 10, 0, 0))   # FX5's (id, yaw-bin, pitch-bin, roll-bin)
N_PARAMS, N_XHAT, N_GRAD = 32, 8, 8


def extra_slices(W: np.ndarray, count: int, seed: int = SEED) -> np.ndarray:
    """f32[count,3,3,3,1404] synthetic identity slices at W's per-element magnitude."""
    W = np.asarray(W, np.float32)
    scale = np.abs(W.astype(np.float64)).mean(axis=0)
    z = synth.rng(seed, 501).standard_normal((count,) + W.shape[1:])
    return (z * scale).astype(np.float32)


def slices_checksum(S: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(S, np.float32).tobytes()).hexdigest()


def rank_W(W: np.ndarray, R: int, seed: int = SEED) -> np.ndarray:
    """W f32[5,3,3,3,1404] -> f32[R,3,3,3,1404]."""
    W = np.asarray(W, np.float32)
    if R <= W.shape[0]:
        return np.ascontiguousarray(W[:R])
    return np.ascontiguousarray(np.concatenate([W, extra_slices(W, R - W.shape[0], seed)], axis=0))


def rank_U_id(U_id: np.ndarray, R: int, seed: int = SEED) -> np.ndarray:
    """U_id f64/f32[n,5] -> [n,R]: the first R columns, or R - 5 more columns of the existing columns' mean spread."""
    U = np.asarray(U_id)
    if R <= U.shape[1]:
        return np.ascontiguousarray(U[:, :R])
    sd = float(np.asarray(U, np.float64).std(axis=0).mean())
    extra = (sd * synth.rng(seed, 502).standard_normal((U.shape[0], R - U.shape[1]))).astype(U.dtype)
    return np.ascontiguousarray(np.concatenate([U, extra], axis=1))


def grid_faces(art: dict, R: int, picks=PICKS, seed: int = SEED) -> np.ndarray:
    """Clean grid faces f32[len(picks),1404] of the rank-R model: W_R x1 U_id_R[i] x2 U_yaw[j] x3 U_pitch[k] x4 U_roll[l]."""
    from oracle import tucker as OT
    W, U = rank_W(art["W"], R, seed), rank_U_id(art["U_id"], R, seed)
    return np.stack([OT.grid_reconstruction(W, U[i], art["U_yaw"][j], art["U_pitch"][k], art["U_roll"][l]) for i, j, k, l in picks])


def noisy_faces(art: dict, R: int, n: int, seed: int = SEED) -> np.ndarray:
    """n grid faces of the rank-R model plus N(0, 1e-3) noise (the form of FX4's inputs) -> f32[n,1404]."""
    from oracle import tucker as OT
    W, U = rank_W(art["W"], R, seed), rank_U_id(art["U_id"], R, seed)
    idx = synth.tucker_grid_indices(n, seed=seed + R)
    X = np.stack([OT.grid_reconstruction(W, U[i], art["U_yaw"][j], art["U_pitch"][k], art["U_roll"][l]) for i, j, k, l in idx])
    return (X.astype(np.float64) + 1e-3 * synth.rng(seed + R, 77).standard_normal(X.shape)).astype(np.float32)


def params(R: int, n: int = N_PARAMS, seed: int = SEED) -> np.ndarray:
    """f64[n,3+R] parameter sets; row 0 is the optimiser's starting point (TD_Tester.py:166)."""
    P = synth.tucker_params(n, R, seed=seed + R)
    P[0] = 0.0
    return P


def cos_rows(art: dict):
    return art["optimized_yaw"][0:3, :], art["optimized_pitch"][0:3, :], art["optimized_roll"][0:3, :]
