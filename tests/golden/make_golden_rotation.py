#!/usr/bin/env python3
"""Generate tests/golden/fx12_rotation_tensor.npz by running the reference's own tensor composition and landmark rotation.

Run ONCE in the build container (needs /root/reference; the GPU box has neither the reference nor a need to run this):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rotation.py

What is imported from /root/reference and called (file:line of the callee):
  FX12 CreateTensor.py:52                  Compose_Tensor(..., use_rotation_features=1)   once, 2 identities x 3 x 3 x 3 bins; the loop
                                                                                         order, the intrinsic rotation (:104-110) and the
                                                                                         (0,0,0) copy (:97-98) are the reference's own
       helpers/IntrinsicRotation.py:108    apply_rotations                               both rotation types, POSES below, on identity 1
                                                                                         and on the 64-row sign table
       helpers/IntrinsicRotation.py:90     rotation_matrix                               every bin of the reference's full grid
                                                                                         (11 + 9 + 7 values) on all three axes
Compose_Tensor reads its base landmarks from image files through FaceMesh (:72-77).  Neither exists here, so the reference's
module is handed two stand-ins for the duration of the call: glob.glob returns the path it was asked for, and
FeatureExtractor.get_feature_vector returns the fixture's base landmarks of the identity named in that path.  cv2, mediapipe and
tensorly are stubs (mediapipe's FaceMesh is constructed and never used; tensorly.tensor returns its argument).

base f32[2,468,3] from Generator G (nlml_hpe_amd/synth.py rng), seed 12:
  identity 0   U(-2, 2), landmark 1 moved to the origin (the form the IPD normalisation leaves)
  identity 1   U(0, 640) pixel-scale coordinates; a handful of coordinates set to -0.0 and +0.0, landmark 300 all -0.0
signs f32[64,3]: every combination of {0.0, -0.0, 1.25, -0.75}^3.
Nothing non-finite, and nothing of the reference's source, is written to the fixture: it holds the inputs and the numbers the
reference returned.  The per-cell time of the reference's loop on this CPU is printed, not stored.
"""
from __future__ import annotations

import itertools
import os
import sys
import time
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
sys.dont_write_bytecode = True

for _n in ("cv2", "mediapipe", "tensorly"):
    sys.modules.setdefault(_n, types.ModuleType(_n))
sys.modules["mediapipe"].solutions = types.SimpleNamespace(face_mesh=types.SimpleNamespace(FaceMesh=lambda **kw: None))
sys.modules["tensorly"].tensor = lambda t: t

import torch  # noqa: E402,F401

from nlml_hpe_amd import synth  # noqa: E402

SEED = 12
YAW, PITCH, ROLL = np.arange(-50, 51, 50), np.arange(-40, 41, 40), np.arange(-30, 31, 30)     # the fixture's 3 x 3 x 3 bins
FULL_YAW, FULL_PITCH, FULL_ROLL = np.arange(-50, 51, 10), np.arange(-40, 41, 10), np.arange(-30, 31, 10)   # the reference's grid
# (yaw, pitch, roll) in degrees: multiples of 90, poses with three, two and one zero angle, ordinary ones
POSES = [(0, 0, 0), (90, 0, 0), (0, -90, 180), (270, 90, -90), (0, 0, 17), (0, -23.5, 40), (31, 12, -7), (-48.25, 37.5, 29.125)]
SIGN_VALUES = (0.0, -0.0, 1.25, -0.75)


def _ref(name: str):
    """Import a module of the reference and make sure it IS the reference's file (not a same-named file of this repo)."""
    import importlib
    mod = importlib.import_module(name)
    path = os.path.abspath(getattr(mod, "__file__", "") or "")
    if not path.startswith(REF + os.sep):
        raise ImportError(f"{name} resolved to {path}, not to the reference under {REF}")
    return mod


def inputs():
    """(base f32[2,468,3], signs f32[64,3]); the recipe in the module docstring."""
    base = np.zeros((2, 468, 3), np.float32)
    u = synth.rng(SEED, 0).random((468, 3)) * 4.0 - 2.0
    base[0] = (u - u[1]).astype(np.float32)
    base[1] = (synth.rng(SEED, 1).random((468, 3)) * 640.0).astype(np.float32)
    for i, c, v in ((5, 0, -0.0), (5, 2, 0.0), (17, 1, -0.0), (99, 0, 0.0), (99, 1, -0.0), (200, 2, -0.0), (467, 0, -0.0)):
        base[1, i, c] = v
    base[1, 300] = -0.0
    signs = np.array(list(itertools.product(SIGN_VALUES, repeat=3)), np.float32)
    return base, signs


def fx12_rotation_tensor():
    CT = _ref("CreateTensor")
    IR = _ref("helpers.IntrinsicRotation")
    base, signs = inputs()
    identities = ["0", "1"]

    def fake_glob(pattern):                       # CreateTensor.py:75: glob.glob(base_img_path + ".*")[0]
        return [pattern[:-2]]

    def fake_features(face_mesh, path, normalize=True):      # CreateTensor.py:76: the base landmarks of the identity in the path
        name = os.path.basename(path)
        assert name.startswith("ID") and name.endswith("_(0_0_0)"), path
        return base[identities.index(name[2:-len("_(0_0_0)")])].reshape(-1).copy()

    shape = (len(identities), len(YAW), len(PITCH), len(ROLL), 1404)
    real_glob, real_fe = CT.glob, CT.FE.get_feature_vector
    CT.glob = types.SimpleNamespace(glob=fake_glob)
    CT.FE.get_feature_vector = fake_features
    try:
        t0 = time.perf_counter()
        tensor, flag = CT.Compose_Tensor("images", shape, YAW, PITCH, ROLL, identities, 1)
        dt = time.perf_counter() - t0
    finally:
        CT.glob, CT.FE.get_feature_vector = real_glob, real_fe
    tensor = tensor.numpy()
    assert flag is False and tensor.shape == shape and tensor.dtype == np.float32
    cells = int(np.prod(shape[:4]))
    print(f"reference Compose_Tensor: {cells} cells in {dt * 1e3:.2f} ms = {dt * 1e3 / cells:.3f} ms per cell on this CPU")

    types_ = ("intrinsic", "extrinsic")
    apply64 = np.zeros((2, len(POSES), 468, 3), np.float64)
    signs64 = np.zeros((2, len(POSES), 64, 3), np.float64)
    for k, rt in enumerate(types_):
        for j, pose in enumerate(POSES):
            apply64[k, j] = IR.apply_rotations(base[1], list(pose), rt)
            signs64[k, j] = IR.apply_rotations(signs, list(pose), rt)
    mats = {}
    for ax in ("x", "y", "z"):
        for nm, vals in (("yaw", FULL_YAW), ("pitch", FULL_PITCH), ("roll", FULL_ROLL)):
            mats[f"rot_{ax}_{nm}_bits"] = np.stack([IR.rotation_matrix(ax, a) for a in vals]).astype(np.float64).view(np.uint64)
    assert np.isfinite(tensor).all() and np.isfinite(apply64).all() and np.isfinite(signs64).all() and np.isfinite(base).all()
    path = os.path.join(OUT, "fx12_rotation_tensor.npz")
    np.savez_compressed(path, base_bits=base.view(np.uint32), signs_bits=signs.view(np.uint32), yaw=YAW, pitch=PITCH, roll=ROLL,
                        full_yaw=FULL_YAW, full_pitch=FULL_PITCH, full_roll=FULL_ROLL, tensor_bits=tensor.view(np.uint32),
                        poses=np.array(POSES, np.float64), apply_f64_bits=apply64.view(np.uint64), signs_f64_bits=signs64.view(np.uint64),
                        **mats)
    print("FX12 written:", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    fx12_rotation_tensor()
