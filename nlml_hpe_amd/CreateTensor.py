"""Host-side mirror of the reference's CreateTensor module on the HIP kernel (K6, csrc/rotate_landmarks.hip).

Same names and argument meaning as /root/reference/CreateTensor.py:
  discretize_interval(a, b, n)                                                            :26-48
  Compose_Tensor(..., tensor_shape, yaw_discretized, pitch_discretized, roll_discretized,
                 identities, use_rotation_features)                                       :52-119  -> (tensor, False)
The first argument differs: the reference reads every identity's pose-(0,0,0) image through FaceMesh (:72-77); here the caller hands
the landmarks themselves, base_landmarks f32[I,468,3] -- the pre-extracted-landmark mode of the other entry points.  With
use_rotation_features=1 (the default source of the training tensor, TD_main.py:58) the tensor is then pure arithmetic: every
identity's landmarks rotated to every (yaw, pitch, roll) bin, intrinsic order (:104), the all-zero bin copied (:97-98).
"""
from __future__ import annotations

import numpy as np
import torch

from . import IntrinsicRotation as IR
from . import ops


def discretize_interval(a, b, n):
    """n equally spaced points of [a, b] and their spacing (:26-48)."""
    if n <= 0:
        raise ValueError("Number of points must be positive.")
    if a >= b:
        raise ValueError("Start of interval must be less than end of interval.")
    spacing = (b - a) / (n - 1)
    return [a + i * spacing for i in range(n)], spacing


def _zero_bin(values, name: str) -> int:
    """Index of the bin whose VALUE is 0 (the reference compares values, :97), -1 if there is none."""
    hits = [i for i, v in enumerate(values) if v == 0]
    if len(hits) > 1:
        raise ValueError(f"{name}_discretized holds the value 0 {len(hits)} times: the copy rule takes one zero bin per axis")
    return hits[0] if hits else -1


def Compose_Tensor(base_landmarks, tensor_shape, yaw_discretized, pitch_discretized, roll_discretized, identities=None,
                   use_rotation_features=1):
    """-> (composition tensor f32[I,ny,np,nr,1404] on the device, False), the reference's bits (:96-119)."""
    if use_rotation_features != 1:
        raise NotImplementedError(
            "use_rotation_features=0 reads every pose's image through FaceMesh and falls back to the torch-f32 per-point rotation "
            "apply_rotation_to_points (CreateTensor.py:80-94), whose operation order is not pinned; only use_rotation_features=1 "
            "(rotation of the base landmarks) runs here")
    base = IR._landmarks(base_landmarks, 3)
    yaw, pitch, roll = list(yaw_discretized), list(pitch_discretized), list(roll_discretized)
    shape = (base.shape[0], len(yaw), len(pitch), len(roll), ops.F_REF)
    if tuple(int(s) for s in tensor_shape) != shape:
        raise ValueError(f"tensor_shape {tuple(tensor_shape)} disagrees with the inputs: {shape[0]} identities and "
                         f"{shape[1]} x {shape[2]} x {shape[3]} bins of 1404 features give {shape}")
    if identities is not None and len(identities) != shape[0]:
        raise ValueError(f"{len(identities)} identities but base_landmarks holds {shape[0]}")
    zero = (_zero_bin(yaw, "yaw"), _zero_bin(pitch, "pitch"), _zero_bin(roll, "roll"))
    base = base.to(IR._dev())
    dev = base.device
    tables = [torch.from_numpy(IR.rotation_matrices(axis, vals)).to(dev) for axis, vals in (("y", yaw), ("x", pitch), ("z", roll))]
    return ops.compose_rotation_tensor(base, *tables, order="intrinsic", zero_index=zero), False
