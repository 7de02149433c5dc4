"""Host-side mirror of the reference's helpers/IntrinsicRotation module on the HIP kernel (K6, csrc/rotate_landmarks.hip).

Same names and argument meaning as /root/reference/helpers/IntrinsicRotation.py for the numpy path:
  rotation_matrix(axis, angle)                                   :90-105   -> f64[3,3] on the host
  apply_rotations(landmarks, angles, rotation_type='extrinsic')  :108-120  -> f64[468,3] on the device
plus the batched form this build adds: apply_rotations_batch (one pose per face).
The trigonometry stays on the host, in numpy and in the reference's expressions, so the matrices are the reference's bit for bit
(the -0.0 that -np.sin(0) puts into Rx and Rz included); the kernel only multiplies.  The torch-f32, per-point path of the reference
(apply_rotation_to_points, :75-86) is not offered: its operation order is not pinned.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops

_AXES = ("x", "y", "z")


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def rotation_matrix(axis, angle):
    """f64[3,3] for `angle` degrees about 'x', 'y' or 'z' (IntrinsicRotation.py:90-105)."""
    if axis not in _AXES:
        raise ValueError("Axis must be 'x', 'y', or 'z'")
    angle_rad = np.radians(angle)
    c, s = np.cos(angle_rad), np.sin(angle_rad)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def rotation_matrices(axis, angles) -> np.ndarray:
    """rotation_matrix for every angle of a sequence -> f64[n,3,3]: one scalar call per angle, the reference's own evaluation."""
    return np.array([rotation_matrix(axis, a) for a in angles], dtype=np.float64).reshape(-1, 3, 3)


def _axis_matrices_vectorised(axis, angles) -> np.ndarray:
    """rotation_matrix over an array of angles (degrees, f64[n]) -> f64[n,3,3] without a Python loop."""
    rad = np.radians(np.asarray(angles, dtype=np.float64))
    c, s = np.cos(rad), np.sin(rad)
    M = np.zeros(rad.shape + (3, 3), np.float64)
    a, b = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]     # the plane of the rotation: M[a][a] = c, M[a][b] = -s, M[b][a] = s
    k = 3 - a - b
    M[..., k, k] = 1.0
    M[..., a, a] = c
    M[..., b, b] = c
    M[..., a, b] = -s
    M[..., b, a] = s
    return M


def pose_matrices(angles_deg, rotation_type="extrinsic") -> np.ndarray:
    """angles_deg [B,3] as (yaw, pitch, roll) -> f64[B,3,3,3]: each face's three matrices in APPLICATION order (:113-118) --
    intrinsic Rx(pitch), Ry(yaw), Rz(roll); extrinsic Rz(roll)^T, Ry(yaw)^T, Rx(pitch)^T."""
    order = _lib.rot_order_from_name(rotation_type)
    ang = np.asarray(angles_deg, dtype=np.float64).reshape(-1, 3)
    rx, ry, rz = _axis_matrices_vectorised("x", ang[:, 1]), _axis_matrices_vectorised("y", ang[:, 0]), _axis_matrices_vectorised("z", ang[:, 2])
    if order == _lib.ROT_INTRINSIC:
        return np.ascontiguousarray(np.stack([rx, ry, rz], axis=1))
    t = (0, 2, 1)
    return np.ascontiguousarray(np.stack([rz.transpose(t), ry.transpose(t), rx.transpose(t)], axis=1))


def _landmarks(landmarks, dims: int) -> torch.Tensor:
    """Landmarks given as a numpy array or a tensor on any device -> the checked f32 tensor of `dims` dimensions, not yet moved."""
    if isinstance(landmarks, torch.Tensor):
        t = landmarks.detach()
        if t.dtype != torch.float32:
            raise TypeError(f"landmarks: expected float32 (the reference's FaceMesh features), got {t.dtype}")
    else:
        a = np.asarray(landmarks)
        if a.dtype != np.float32:
            raise TypeError(f"landmarks: expected float32 (the reference's FaceMesh features), got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != dims or tuple(t.shape[-2:]) != (468, 3):
        raise ValueError(f"landmarks: expected {'[468,3]' if dims == 2 else '[B,468,3]'}, got {tuple(t.shape)}")
    return t


def apply_rotations(landmarks, angles, rotation_type="extrinsic"):
    """One [468,3] float32 block at the pose angles = (yaw, pitch, roll) in degrees -> f64[468,3] on the device, the reference's bits
    (:108-120).  The matrices come from rotation_matrix itself, one scalar call each."""
    order = _lib.rot_order_from_name(rotation_type)
    lm = _landmarks(landmarks, 2).to(_dev())
    rot_x = rotation_matrix("x", angles[1])
    rot_y = rotation_matrix("y", angles[0])
    rot_z = rotation_matrix("z", angles[2])
    stages = [rot_x, rot_y, rot_z] if order == _lib.ROT_INTRINSIC else [rot_z.T, rot_y.T, rot_x.T]
    rot = torch.from_numpy(np.ascontiguousarray(np.stack(stages), dtype=np.float64).reshape(1, 3, 3, 3)).to(lm.device)
    return ops.rotate_landmarks(lm.unsqueeze(0), rot, return_f64=True, return_f32=False)[0]


def apply_rotations_batch(landmarks, angles_deg, rotation_type="extrinsic", dtype=torch.float64):
    """landmarks f32[B,468,3], angles_deg [B,3] as (yaw, pitch, roll) -> [B,468,3] on the device: apply_rotations per face, as
    dtype float64 (the reference's return value) or float32 (one rounding of it, as CreateTensor.py:110 stores it)."""
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"dtype: expected torch.float32 or torch.float64, got {dtype}")
    lm = _landmarks(landmarks, 3)
    ang = np.asarray(angles_deg.detach().cpu().numpy() if isinstance(angles_deg, torch.Tensor) else angles_deg, dtype=np.float64)
    if ang.shape != (lm.shape[0], 3):
        raise ValueError(f"angles_deg: expected [{lm.shape[0]},3], got {ang.shape}")
    rot = pose_matrices(ang, rotation_type)
    lm = lm.to(_dev())
    rot = torch.from_numpy(rot).to(lm.device)
    f64 = dtype == torch.float64
    return ops.rotate_landmarks(lm, rot, return_f64=f64, return_f32=not f64)
