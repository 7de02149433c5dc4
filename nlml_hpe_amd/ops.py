"""torch-facing operators over the C ABI (include/nlml_hpe.h).

Each function takes CUDA(HIP) tensors, checks shapes/dtypes on the host (a wrong shape must
never reach a hand-written kernel), and launches on torch's CURRENT stream.  The same entry
points are registered as ``torch.ops.nlml_hpe.*`` custom ops.  No CPU path:
a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

F_REF = 1404
LATENT = 9


def _stream_ptr(device=None) -> int:
    """torch's current HIP stream OF `device` (default: the current device)."""
    return torch.cuda.current_stream(device).cuda_stream


def _need_cuda(t: torch.Tensor, name: str, dtype) -> None:
    if not t.is_cuda:
        raise _lib.NlmlError(f"{name}: expected a GPU tensor (there is no CPU fallback), got device {t.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


class _on_device_of:
    """Every operand on ONE GPU, and the launch on THAT GPU: a HIP launch goes to the calling thread's current device, so a
    model living on cuda:1 called while cuda:0 is current would run on GPU 0 against GPU 1's memory, on a foreign stream.
    `with _on_device_of(x, blob, ...) as stream:` checks that all tensors share a device, makes it current for the launch and
    yields that device's current stream handle; outputs must be allocated on `x.device` by the caller."""

    def __init__(self, *named):
        ts = [(n, t) for n, t in named if t is not None]
        self.device = ts[0][1].device
        for n, t in ts[1:]:
            if t.device != self.device:
                raise _lib.NlmlError(f"{n} is on {t.device} but {ts[0][0]} is on {self.device}: all operands must share one GPU")
        self.guard = torch.cuda.device(self.device)

    def __enter__(self) -> int:
        self.guard.__enter__()
        return _stream_ptr(self.device)

    def __exit__(self, *exc):
        return self.guard.__exit__(*exc)


def _raw_rows(raw: torch.Tensor) -> torch.Tensor:
    if raw.dim() != 3 or raw.shape[1:] != (468, 3):
        raise ValueError(f"raw: expected [B,468,3], got {tuple(raw.shape)}")
    return raw.contiguous()


def normalize_ipd(raw: torch.Tensor, normalize: bool = True, return_valid: bool = False):
    """raw f32[B,468,3] -> features f32[B,1404] (FeatureExtractor.py:30-66,101), bit-exact."""
    _need_cuda(raw, "raw", torch.float32)
    raw = _raw_rows(raw)
    B = raw.shape[0]
    out = torch.empty((B, F_REF), dtype=torch.float32, device=raw.device)
    valid = torch.empty((B,), dtype=torch.uint8, device=raw.device) if return_valid else None
    with _on_device_of(("raw", raw)) as stream:
        _lib.check(_lib.lib().nlml_normalize_ipd(raw.data_ptr(), B, int(bool(normalize)), out.data_ptr(),
                                                 valid.data_ptr() if valid is not None else None, stream),
                   "nlml_normalize_ipd")
    return (out, valid.bool()) if return_valid else out


def normalize_centroid(raw: torch.Tensor, return_valid: bool = False, return_stats: bool = False):
    """raw f32[B,468,3] -> features f32[B,1404] normalised by centroid and RMS radius (FeatureExtractor.py:17-28,101), bit-exact
    [, valid bool[B]: the raw row is not the all-zero "no face" sentinel (whose features are all zero)]
    [, stats f64[B,4]: centroid x, y, z and the scale]."""
    _need_cuda(raw, "raw", torch.float32)
    raw = _raw_rows(raw)
    B = raw.shape[0]
    out = torch.empty((B, F_REF), dtype=torch.float32, device=raw.device)
    valid = torch.empty((B,), dtype=torch.uint8, device=raw.device) if return_valid else None
    stats = torch.empty((B, 4), dtype=torch.float64, device=raw.device) if return_stats else None
    with _on_device_of(("raw", raw)) as stream:
        _lib.check(_lib.lib().nlml_normalize_centroid(raw.data_ptr(), B, out.data_ptr(),
                                                      valid.data_ptr() if valid is not None else None,
                                                      stats.data_ptr() if stats is not None else None, stream),
                   "nlml_normalize_centroid")
    res = [out]
    if return_valid:
        res.append(valid.bool())
    if return_stats:
        res.append(stats)
    return res[0] if len(res) == 1 else tuple(res)


def _rot_table(t: torch.Tensor, name: str) -> torch.Tensor:
    _need_cuda(t, name, torch.float64)
    if t.dim() != 3 or t.shape[1:] != (3, 3):
        raise ValueError(f"{name}: expected [n,3,3], got {tuple(t.shape)}")
    return t.contiguous()


def compose_rotation_tensor(base: torch.Tensor, rot_yaw: torch.Tensor, rot_pitch: torch.Tensor, rot_roll: torch.Tensor,
                            order="intrinsic", zero_index=None, return_f64: bool = False):
    """The rotation training tensor (CreateTensor.py:96-114): base f32[I,468,3], one f64[n,3,3] matrix table per axis ->
    f32[I,ny,np,nr,1404] (+ f64 of the same shape), the reference's bits.  order: "intrinsic" (stages pitch, yaw, roll) or "extrinsic"
    (stages roll, yaw, pitch; pass the transposed matrices).  zero_index: (yaw, pitch, roll) indices of the bins whose value is 0 --
    that cell is the base copied bit for bit -- or -1 / None where there is none."""
    _need_cuda(base, "base", torch.float32)
    if base.dim() != 3 or base.shape[1:] != (468, 3):
        raise ValueError(f"base: expected [I,468,3], got {tuple(base.shape)}")
    base = base.contiguous()
    rot_yaw, rot_pitch, rot_roll = _rot_table(rot_yaw, "rot_yaw"), _rot_table(rot_pitch, "rot_pitch"), _rot_table(rot_roll, "rot_roll")
    order = _lib.rot_order_from_name(order)
    zero = [-1, -1, -1] if zero_index is None else [int(z) for z in zero_index]
    I, ny, np_, nr = base.shape[0], rot_yaw.shape[0], rot_pitch.shape[0], rot_roll.shape[0]
    if len(zero) != 3 or any(not -1 <= z < n for z, n in zip(zero, (ny, np_, nr))):
        raise ValueError(f"zero_index: expected (yaw, pitch, roll) indices in -1..n-1 for {ny} x {np_} x {nr} bins, got {zero_index!r}")
    out = torch.empty((I, ny, np_, nr, F_REF), dtype=torch.float32, device=base.device)
    out64 = torch.empty((I, ny, np_, nr, F_REF), dtype=torch.float64, device=base.device) if return_f64 else None
    with _on_device_of(("base", base), ("rot_yaw", rot_yaw), ("rot_pitch", rot_pitch), ("rot_roll", rot_roll)) as stream:
        _lib.check(_lib.lib().nlml_compose_rotation_tensor(
            base.data_ptr(), I, rot_yaw.data_ptr(), ny, rot_pitch.data_ptr(), np_, rot_roll.data_ptr(), nr, order, *zero, out.data_ptr(),
            out64.data_ptr() if return_f64 else None, stream), "nlml_compose_rotation_tensor")
    return (out, out64) if return_f64 else out


def rotate_landmarks(lm: torch.Tensor, rot: torch.Tensor, return_f64: bool = False, return_f32: bool = True):
    """apply_rotations (IntrinsicRotation.py:108-120) with one pose per face: lm f32[B,468,3], rot f64[B,3,3,3] (each face's three
    matrices in application order) -> f32[B,468,3] (one rounding of the f64 result) and / or the f64[B,468,3] itself, the reference's
    bits."""
    _need_cuda(lm, "lm", torch.float32)
    _need_cuda(rot, "rot", torch.float64)
    lm = _raw_rows(lm)
    B = lm.shape[0]
    if tuple(rot.shape) != (B, 3, 3, 3):
        raise ValueError(f"rot: expected [{B},3,3,3], got {tuple(rot.shape)}")
    if not (return_f32 or return_f64):
        raise ValueError("rotate_landmarks: at least one of return_f32, return_f64")
    rot = rot.contiguous()
    out = torch.empty((B, 468, 3), dtype=torch.float32, device=lm.device) if return_f32 else None
    out64 = torch.empty((B, 468, 3), dtype=torch.float64, device=lm.device) if return_f64 else None
    with _on_device_of(("lm", lm), ("rot", rot)) as stream:
        _lib.check(_lib.lib().nlml_rotate_landmarks(lm.data_ptr(), rot.data_ptr(), out.data_ptr() if return_f32 else None,
                                                    out64.data_ptr() if return_f64 else None, B, stream), "nlml_rotate_landmarks")
    if return_f32 and return_f64:
        return out, out64
    return out if return_f32 else out64


# ---- the K2 forward (encoder + heads): one private forward behind the five public wrappers ---------------------------------------
_k2_ws: dict = {}


def _k2_workspace(form: str, B: int, F: int, device, floor_faces: int = 0, need_bytes: int = 0) -> torch.Tensor:
    """Scratch of the K2 call forms that need one (its contents never matter).  Buffers are cached per form, device and stream and
    NEVER released or replaced: a captured hipGraph keeps replaying into the pointer it was captured with, so growing means
    adding a larger buffer next to the old one.  floor_faces: a new buffer holds at least that many faces of the reference width."""
    size_of = _lib.lib().nlml_encoder_heads_small_workspace_bytes if form == "small" else _lib.lib().nlml_encoder_heads_workspace_bytes
    need = max(16, need_bytes or size_of(B, F))        # need_bytes: the caller knows what this call takes (the "ws" form's quad part)
    # one pool per (device, stream): launches on different streams may overlap and must not share scratch
    pool = _k2_ws.setdefault((form, str(device), _stream_ptr(device)), [])
    for ws in pool:
        if ws.numel() >= need:
            return ws
    ws = torch.empty((max(need, size_of(floor_faces, F_REF)),), dtype=torch.uint8, device=device)
    pool.append(ws)
    return ws


def _small_workspace(B: int, F: int, device) -> torch.Tensor:
    """The layer-per-launch path's scratch; the first buffer is sized for the largest batch that path takes at the reference width
    (46 MB)."""
    return _k2_workspace("small", B, F, device, floor_faces=_lib.lib().nlml_k2_small_batch_max(_lib.MODE_F16X2S))


def _k2_quad_part(rows: tuple, blob: torch.Tensor, device) -> int:
    """Bytes of workspace with which nlml_*_ws sends a part of this batch through the four-tile strict-fast kernel
    (csrc/encoder_heads_f16x2_w8.hip) on `device`, 0 if it would not.  The library's own rule (nlml_k2_quad_part); rows: the
    (pointer, row stride, B, F) it takes."""
    n, need = C.c_int64(0), C.c_size_t(0)
    with torch.cuda.device(device):
        rc = _lib.lib().nlml_k2_quad_part(*rows, blob.numel(), C.byref(n), C.byref(need))
    return int(need.value) if rc == 0 and n.value > 0 else 0


def _k2_forward(form: str, x, raw, blob: torch.Tensor, F: int, normalize, return_latent: bool, return_valid: bool, workspace=None):
    """x f32[B,F] (raw None) or raw f32[B,468,3] (x None) -> out f32[B,3][, latent f32[B,9]][, valid bool[B]] through the C entry
    point of the call form: "" (the fused kernel -- or, where _k2_quad_part says so, the _ws entry point with the pooled workspace),
    "small", "streamed" or "quad" (all through a workspace, pooled unless given)."""
    if raw is None:
        _need_cuda(x, "x", torch.float32)
        _need_cuda(blob, "blob", torch.uint8)
        if x.dim() != 2 or x.shape[1] != F:
            raise ValueError(f"x: expected [B,{F}], got {tuple(x.shape)}")
        if x.stride(1) != 1:
            x = x.contiguous()
        src, name, symbol = x, "x", "nlml_encoder_heads_fwd"
        B = x.shape[0]
        head = rows = (x.data_ptr(), x.stride(0) if B > 1 else F, B, F)
    else:
        _need_cuda(raw, "raw", torch.float32)
        _need_cuda(blob, "blob", torch.uint8)
        src, name, symbol = _raw_rows(raw), "raw", "nlml_landmarks_to_pose"
        B = src.shape[0]
        head, rows = (src.data_ptr(), B, int(bool(normalize))), (src.data_ptr(), F, B, F)
    dev = src.device
    tail = ()
    quad_bytes = 0 if form else _k2_quad_part(rows, blob, dev)
    if quad_bytes:
        form = "ws"        # the dispatcher splits the batch: whole rounds through the four-tile kernel, the rest through the fused one
    if form:
        symbol += "_" + form
        if workspace is None:
            workspace = _small_workspace(B, F, dev) if form == "small" else _k2_workspace(form, B, F, dev, need_bytes=quad_bytes)
        tail = (workspace.data_ptr(), workspace.numel())
    out = torch.empty((B, 3), dtype=torch.float32, device=dev)
    latent = torch.empty((B, LATENT), dtype=torch.float32, device=dev) if return_latent else None
    valid = torch.empty((B,), dtype=torch.uint8, device=dev) if return_valid else None
    with _on_device_of((name, src), ("blob", blob), ("workspace", workspace)) as stream:
        _lib.check(getattr(_lib.lib(), symbol)(
            *head, blob.data_ptr(), blob.numel(), out.data_ptr(),
            latent.data_ptr() if latent is not None else None,
            valid.data_ptr() if valid is not None else None, *tail, stream), symbol)
    res = [out]
    if return_latent:
        res.append(latent)
    if return_valid:
        res.append(valid.bool())
    return res[0] if len(res) == 1 else tuple(res)


def encoder_heads_fwd(x: torch.Tensor, blob: torch.Tensor, F: int, return_latent: bool = False,
                      return_valid: bool = False):
    """x f32[B,F] -> radians f32[B,3] (CombinedAnglePredictionModel.forward, Model_Builder.py:115-126)."""
    return _k2_forward("", x, None, blob, F, None, return_latent, return_valid)


def encoder_heads_fwd_debug(x: torch.Tensor, blob: torch.Tensor, F: int, want_stamps: bool = False):
    """Diagnostic build: (out [B,3], latent [B,9], pre_tanh [B,64][, stamps i64[ceil(B/64),4,16]]); include/nlml_hpe.h."""
    _need_cuda(x, "x", torch.float32)
    _need_cuda(blob, "blob", torch.uint8)
    if x.dim() != 2 or x.shape[1] != F:
        raise ValueError(f"x: expected [B,{F}], got {tuple(x.shape)}")
    x = x.contiguous()
    B = x.shape[0]
    out = torch.empty((B, 3), dtype=torch.float32, device=x.device)
    latent = torch.empty((B, LATENT), dtype=torch.float32, device=x.device)
    pre = torch.empty((B, 64), dtype=torch.float32, device=x.device)
    stamps = torch.zeros(((B + 63) // 64, 4, 16), dtype=torch.int64, device=x.device) if want_stamps else None
    with _on_device_of(("x", x), ("blob", blob)) as stream:
        _lib.check(_lib.lib().nlml_encoder_heads_fwd_debug(x.data_ptr(), F, B, F, blob.data_ptr(), blob.numel(),
                                                           out.data_ptr(), latent.data_ptr(), pre.data_ptr(),
                                                           stamps.data_ptr() if want_stamps else None, stream),
                   "nlml_encoder_heads_fwd_debug")
    return (out, latent, pre, stamps) if want_stamps else (out, latent, pre)


def landmarks_to_pose(raw: torch.Tensor, blob: torch.Tensor, normalize: bool = True, return_latent: bool = False,
                      return_valid: bool = False):
    """Fused K1+K2: raw f32[B,468,3] -> radians f32[B,3]; normalised features never reach HBM."""
    return _k2_forward("", None, raw, blob, F_REF, normalize, return_latent, return_valid)


def encoder_heads_fwd_small(x: torch.Tensor, blob: torch.Tensor, F: int, return_latent: bool = False,
                            return_valid: bool = False, workspace: torch.Tensor | None = None):
    """encoder_heads_fwd for small batches (split-f16 blob only): one launch per big layer (five launches; seven with a strict blob: its
    tail is two launches and the f32 re-evaluation launch follows) spread over the whole chip, bit-identical results."""
    return _k2_forward("small", x, None, blob, F, None, return_latent, return_valid, workspace)


def landmarks_to_pose_small(raw: torch.Tensor, blob: torch.Tensor, normalize: bool = True, return_latent: bool = False,
                            return_valid: bool = False, workspace: torch.Tensor | None = None):
    """landmarks_to_pose for small batches (split-f16 blob only): one launch per big layer (five launches; seven with a strict blob) spread
    over the whole chip, bit-identical results."""
    return _k2_forward("small", None, raw, blob, F_REF, normalize, return_latent, return_valid, workspace)


def landmarks_to_pose_streamed(raw: torch.Tensor, blob: torch.Tensor, normalize: bool = True, return_latent: bool = False,
                               return_valid: bool = False, workspace: torch.Tensor | None = None):
    """landmarks_to_pose (strict-fast blob only) as trunk launch + streamed tail launch + the f32 re-evaluation launch
    (nlml_landmarks_to_pose_streamed): bit-identical to the fused kernel, measured 1.4-2.2 % faster at 65,536 faces; nothing calls it by default
    (DESIGN.md section 3).  The hand-over buffer (1 KB per face) is cached per device and stream like the layer-per-launch path's scratch."""
    return _k2_forward("streamed", None, raw, blob, F_REF, normalize, return_latent, return_valid, workspace)


def landmarks_to_pose_quad(raw: torch.Tensor, blob: torch.Tensor, normalize: bool = True, return_latent: bool = False,
                           return_valid: bool = False, workspace: torch.Tensor | None = None):
    """landmarks_to_pose (strict-fast blob only) through the four-tile kernel whatever the batch size (nlml_landmarks_to_pose_quad: a
    workgroup runs layers 0-2 over four tiles, then the streamed tail once; + the f32 re-evaluation launch): bit-identical to the fused
    kernel.  landmarks_to_pose itself takes this path for whole rounds of 256 faces per compute unit.  The
    hand-over buffer (1 KB per face) is cached per device and stream like the streamed path's."""
    return _k2_forward("quad", None, raw, blob, F_REF, normalize, return_latent, return_valid, workspace)


def encoder_heads_fwd_quad(x: torch.Tensor, blob: torch.Tensor, F: int, return_latent: bool = False,
                           return_valid: bool = False, workspace: torch.Tensor | None = None):
    """encoder_heads_fwd (strict-fast blob only, rows 16-byte aligned) through the four-tile kernel whatever the batch size
    (nlml_encoder_heads_fwd_quad); see landmarks_to_pose_quad."""
    return _k2_forward("quad", x, None, blob, F, None, return_latent, return_valid, workspace)


# ---- the TD path (K3 objective, K3g gradient, device Powell): one operand preamble behind the three public wrappers ----------------
def _td_operands(Wm, x, cos_params, params=None, x_index=None, x0=None):
    """The operand checks of the TD wrappers -> (Wm, x, cos_params, params, x_index, x0, r_id, N), every tensor contiguous.  With params
    (objective, gradient): N = its rows, evaluation n on row n of x, or on row x_index[n].  Without (Powell): one minimisation per row
    of x, N of them, started at x0[n] if x0 is given."""
    _need_cuda(Wm, "Wm", torch.float32)
    _need_cuda(x, "x", torch.float32)
    if params is not None:
        _need_cuda(params, "params", torch.float64)
    _need_cuda(cos_params, "cos_params", torch.float64)
    if Wm.dim() != 2 or Wm.shape[1] != F_REF:
        raise ValueError(f"Wm: expected [27*R,1404], got {tuple(Wm.shape)}")
    r_id = _lib.tucker_rank_of_rows(Wm.shape[0])
    if x.dim() != 2 or x.shape[1] != F_REF:
        raise ValueError(f"x: expected [{'N' if params is None else 'M'},1404], got {tuple(x.shape)}")
    if params is not None and (params.dim() != 2 or params.shape[1] != 3 + r_id):
        raise ValueError(f"params: expected [N,{3 + r_id}] for Wm of identity rank {r_id}, got {tuple(params.shape)}")
    if tuple(cos_params.shape) != (3, 3, 4):
        raise ValueError(f"cos_params: expected [3,3,4], got {tuple(cos_params.shape)}")
    Wm, x, cos_params = Wm.contiguous(), x.contiguous(), cos_params.contiguous()
    if params is None:
        N = x.shape[0]
        if x0 is not None:
            _need_cuda(x0, "x0", torch.float64)
            if tuple(x0.shape) != (N, 3 + r_id):
                raise ValueError(f"x0: expected [{N},{3 + r_id}], got {tuple(x0.shape)}")
            x0 = x0.contiguous()
        return Wm, x, cos_params, None, None, x0, r_id, N
    params = params.contiguous()
    N = params.shape[0]
    if x_index is not None:
        _need_cuda(x_index, "x_index", torch.int32)
        if x_index.shape != (N,):
            raise ValueError("x_index: expected [N]")
        x_index = x_index.contiguous()
        if N and (int(x_index.min()) < 0 or int(x_index.max()) >= x.shape[0]):
            raise IndexError("x_index out of range")
    elif x.shape[0] != N:
        raise ValueError(f"x has {x.shape[0]} rows but params has {N} (pass x_index to share rows)")
    return Wm, x, cos_params, params, x_index, None, r_id, N


def tucker_objective(Wm: torch.Tensor, x: torch.Tensor, params: torch.Tensor, cos_params: torch.Tensor,
                     x_index: torch.Tensor | None = None, return_xhat: bool = False, order="reference"):
    """Batched objective (TD_Tester.py:31-58): Wm f32[27R,1404], x f32[M,1404], params f64[N,3+R],
    cos_params f64[3,3,4] -> err f64[N] (+ x_hat f64[N,1404]); R = the identity rank, 1..16 (5 for the shipped artefacts).  order: "reference" (the default and the parity mode: np.einsum's
    operation order and numpy's pairwise sum -- the reference's bits) or "fast" (opt-in: a GEMM on the f64 matrix cores, <= 1e-12
    relative, ~5x the evaluations/s)."""
    order = _lib.td_order_from_name(order)
    Wm, x, cos_params, params, x_index, _, r_id, N = _td_operands(Wm, x, cos_params, params, x_index)
    err = torch.empty((N,), dtype=torch.float64, device=x.device)
    xh = torch.empty((N, F_REF), dtype=torch.float64, device=x.device) if return_xhat else None
    with _on_device_of(("x", x), ("Wm", Wm), ("params", params), ("cos_params", cos_params), ("x_index", x_index)) as stream:
        _lib.check(_lib.lib().nlml_tucker_objective_r(
            Wm.data_ptr(), x.data_ptr(), F_REF, x_index.data_ptr() if x_index is not None else None,
            params.data_ptr(), cos_params.data_ptr(), N, err.data_ptr(),
            xh.data_ptr() if xh is not None else None, r_id, order, stream), "nlml_tucker_objective_r")
    return (err, xh) if return_xhat else err


def tucker_gradient(Wm: torch.Tensor, x: torch.Tensor, params: torch.Tensor, cos_params: torch.Tensor,
                    x_index: torch.Tensor | None = None, return_err: bool = True):
    """K3g: objective value and analytic gradient (TD_Tester.py:60-102, the reference's ``jac=``) in one native call, in the reference's
    own operation order: Wm f32[27R,1404], x f32[M,1404], params f64[N,3+R], cos_params f64[3,3,4] -> (err f64[N], grad f64[N,3+R]),
    or grad alone with return_err=False.  err carries the bits of tucker_objective(order="reference"); every gradient component the
    reference's own (csrc/tucker_grad_ref.h has the order).  R = 1..16."""
    Wm, x, cos_params, params, x_index, _, r_id, N = _td_operands(Wm, x, cos_params, params, x_index)
    err = torch.empty((N,), dtype=torch.float64, device=x.device) if return_err else None
    grad = torch.empty((N, 3 + r_id), dtype=torch.float64, device=x.device)
    ws_bytes = _lib.lib().nlml_tucker_gradient_workspace_bytes(N, r_id)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=x.device)
    with _on_device_of(("x", x), ("Wm", Wm), ("params", params), ("cos_params", cos_params), ("x_index", x_index)) as stream:
        _lib.check(_lib.lib().nlml_tucker_gradient_r(
            Wm.data_ptr(), x.data_ptr(), F_REF, x_index.data_ptr() if x_index is not None else None,
            params.data_ptr(), cos_params.data_ptr(), N, err.data_ptr() if err is not None else None, grad.data_ptr(), r_id,
            ws.data_ptr(), ws_bytes, stream), "nlml_tucker_gradient_r")
    return (err, grad) if return_err else grad


def tucker_powell(Wm: torch.Tensor, x: torch.Tensor, cos_params: torch.Tensor, x0: torch.Tensor | None = None, order="reference"):
    """Batched Test() (TD_Tester.py:162-199): one Powell minimisation per row of x, on device.  order as in tucker_objective:
    "reference" (default, the parity mode) walks scipy's own trajectory on the reference's objective bits; "fast" (opt-in, ~3x the
    faces/s) minimises the matrix-core objective: same algorithm, but the flat minimum makes the END POINT sensitive to the last bits
    of the objective -- 6e-3 deg from scipy on clean grid faces (FX5), and on BASELINE config 3's noisy faces median 1.8e-3 deg (per face, largest of the three angles),
    10 % of the faces > 0.02 deg, 0.3 % > 1 deg, max 8.7 deg (bench.py extra.td_powell_fast_order reports it live).

    Wm f32[27R,1404] for an identity rank R = 1..16 (5 for the shipped artefacts): n = 3 + R parameters per face, scipy's limits
    maxiter = maxfev = 1000 n.

    Returns dict(x=f64[N,3+R] (w_y,w_p,w_r radians + u_id), fun=f64[N], nfev=i32[N], nit=i32[N], status=i32[N]).
    """
    Wm, x, cos_params, _, _, x0, r_id, N = _td_operands(Wm, x, cos_params, x0=x0)
    n_par = 3 + r_id
    order = _lib.td_order_from_name(order)
    dev = x.device
    res = torch.empty((N, n_par), dtype=torch.float64, device=dev)
    fun = torch.empty((N,), dtype=torch.float64, device=dev)
    nfev = torch.empty((N,), dtype=torch.int32, device=dev)
    nit = torch.empty((N,), dtype=torch.int32, device=dev)
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    with _on_device_of(("x", x), ("Wm", Wm), ("cos_params", cos_params), ("x0", x0)) as stream:
        _lib.check(_lib.lib().nlml_tucker_powell_r(Wm.data_ptr(), x.data_ptr(), F_REF, cos_params.data_ptr(), N,
                                                   x0.data_ptr() if x0 is not None else None, res.data_ptr(), fun.data_ptr(),
                                                   nfev.data_ptr(), nit.data_ptr(), status.data_ptr(), r_id, order, stream),
                   "nlml_tucker_powell_r")
    return {"x": res, "fun": fun, "nfev": nfev, "nit": nit, "status": status}


def cosine_table(angles_rad: torch.Tensor, cos_params: torch.Tensor) -> torch.Tensor:
    """U[i,j] = a_j*cos(b_j*w_i + c_j) + d_j in f64 (NLML_HPE_MLPHeadsTrainer.py:71-73,179-205).

    angles_rad f32[n] (radians), cos_params f64[R,4] rows (a,b,c,d) -> f64[n,R]."""
    _need_cuda(angles_rad, "angles_rad", torch.float32)
    _need_cuda(cos_params, "cos_params", torch.float64)
    if angles_rad.dim() != 1 or cos_params.dim() != 2 or cos_params.shape[1] != 4:
        raise ValueError(f"expected angles [n] and cos_params [R,4], got {tuple(angles_rad.shape)}, {tuple(cos_params.shape)}")
    angles_rad, cos_params = angles_rad.contiguous(), cos_params.contiguous()
    n, R = angles_rad.shape[0], cos_params.shape[0]
    out = torch.empty((n, R), dtype=torch.float64, device=angles_rad.device)
    with _on_device_of(("angles_rad", angles_rad), ("cos_params", cos_params)) as stream:
        _lib.check(_lib.lib().nlml_cosine_table(angles_rad.data_ptr(), n, cos_params.data_ptr(), R, out.data_ptr(), stream),
                   "nlml_cosine_table")
    return out


def mode5_product(core: torch.Tensor, U_feat: torch.Tensor) -> torch.Tensor:
    """W = core x_5 U_feat (TD_main.py:232-238): core f32[..., R5], U_feat f32[M, R5] -> W f32[..., M]."""
    _need_cuda(core, "core", torch.float32)
    _need_cuda(U_feat, "U_feat", torch.float32)
    if U_feat.dim() != 2 or core.dim() < 1 or core.shape[-1] != U_feat.shape[1]:
        raise ValueError(f"core [..., R5] and U_feat [M, R5] disagree: {tuple(core.shape)}, {tuple(U_feat.shape)}")
    lead = tuple(core.shape[:-1])
    c2 = core.contiguous().reshape(-1, core.shape[-1])
    U_feat = U_feat.contiguous()
    Q, R5, M = c2.shape[0], c2.shape[1], U_feat.shape[0]
    W = torch.empty((Q, M), dtype=torch.float32, device=core.device)
    with _on_device_of(("core", core), ("U_feat", U_feat)) as stream:
        _lib.check(_lib.lib().nlml_mode5_product(c2.data_ptr(), U_feat.data_ptr(), Q, R5, M, W.data_ptr(), stream),
                   "nlml_mode5_product")
    return W.reshape(lead + (M,))


# ---- K7: the Tucker decomposition's primitives (csrc/tucker_decompose.hip; the driver is nlml_hpe_amd/tucker_decompose.py) -----
def _k7_workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty((max(1, (nbytes + 7) // 8),), dtype=torch.float64, device=device)


def _need_f32_or_f64(t: torch.Tensor, name: str) -> int:
    """-> the entry points' f64 flag of a tensor that may be f32 (the tensor itself) or f64 (a projection kept unrounded)."""
    _need_cuda(t, name, t.dtype if t.dtype == torch.float64 else torch.float32)
    return int(t.dtype == torch.float64)


def _out_f64(out_dtype) -> int:
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"out_dtype: expected torch.float32 or torch.float64, got {out_dtype}")
    return int(out_dtype == torch.float64)


def _tensor5(X: torch.Tensor, name: str = "X") -> torch.Tensor:
    _need_f32_or_f64(X, name)
    if X.dim() != 5 or min(X.shape) < 1 or max(X.shape[1:4]) > _lib.POSE_BINS_MAX:
        raise ValueError(f"{name}: expected a non-empty [I,ny,np,nr,M] with at most {_lib.POSE_BINS_MAX} bins per pose mode, "
                         f"got {tuple(X.shape)}")
    return X.contiguous()


def mode_gram(A: torch.Tensor) -> torch.Tensor:
    """K7a: A f32[I,K] (or f64) -> G f64[I,I] = A A^T, f64 sums on the matrix cores; symmetric bit for bit, the same bits on every
    call."""
    a_f64 = _need_f32_or_f64(A, "A")
    if A.dim() != 2 or not 1 <= A.shape[0] <= _lib.MODE_GRAM_I_MAX or A.shape[1] < 1:
        raise ValueError(f"A: expected [I,K] with 1 <= I <= {_lib.MODE_GRAM_I_MAX} and K >= 1, got {tuple(A.shape)}")
    A = A.contiguous()
    I, K = A.shape
    G = torch.empty((I, I), dtype=torch.float64, device=A.device)
    ws = _k7_workspace(_lib.lib().nlml_mode_gram_workspace_bytes(I, K), A.device)
    with _on_device_of(("A", A)) as stream:
        _lib.check(_lib.lib().nlml_mode_gram_ex(A.data_ptr(), a_f64, I, K, G.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream),
                   "nlml_mode_gram")
    return G


def pose_grams(X: torch.Tensor, which=(True, True, True)):
    """K7b: X f32[I,ny,np,nr,M] (or f64) -> (Gy f64[ny,ny], Gp f64[np,np], Gr f64[nr,nr]), the Grams of the three pose-mode unfoldings in one
    pass over X.  which: a False entry skips that Gram (None in its place)."""
    X = _tensor5(X)
    I, ny, np_, nr, M = X.shape
    if ny * np_ * nr > _lib.POSE_GRAMS_MAX_CELLS:
        raise ValueError(f"X: {ny} x {np_} x {nr} pose cells, at most {_lib.POSE_GRAMS_MAX_CELLS} fit the kernel's LDS slab")
    which = tuple(bool(w) for w in which)
    if len(which) != 3 or not any(which):
        raise ValueError("which: three flags, at least one set")
    G = [torch.empty((n, n), dtype=torch.float64, device=X.device) if w else None for n, w in zip((ny, np_, nr), which)]
    ws = _k7_workspace(_lib.lib().nlml_pose_grams_workspace_bytes(I, ny, np_, nr, M), X.device)
    with _on_device_of(("X", X)) as stream:
        _lib.check(_lib.lib().nlml_pose_grams_ex(X.data_ptr(), int(X.dtype == torch.float64), I, ny, np_, nr, M,
                                                 *[g.data_ptr() if g is not None else None for g in G],
                                                 ws.data_ptr(), ws.numel() * 8, stream), "nlml_pose_grams")
    return tuple(G)


def project_identity(A: torch.Tensor, U: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """K7c: A f32[I,K], U f64[I,R] (R <= 16) -> f32[R,K] = U^T A, f64 sums, one rounding; out_dtype=torch.float64: the sums
    themselves."""
    out_f64 = _out_f64(out_dtype)
    _need_cuda(A, "A", torch.float32)
    _need_cuda(U, "U", torch.float64)
    if A.dim() != 2 or U.dim() != 2 or U.shape[0] != A.shape[0] or min(A.shape) < 1:
        raise ValueError(f"A [I,K] and U [I,R] disagree: {tuple(A.shape)}, {tuple(U.shape)}")
    if not _lib.TUCKER_RANK_MIN <= U.shape[1] <= _lib.TUCKER_RANK_MAX:
        raise ValueError(f"U: R = {U.shape[1]} outside [{_lib.TUCKER_RANK_MIN}, {_lib.TUCKER_RANK_MAX}]")
    A, U = A.contiguous(), U.contiguous()
    out = torch.empty((U.shape[1], A.shape[1]), dtype=out_dtype, device=A.device)
    with _on_device_of(("A", A), ("U", U)) as stream:
        _lib.check(_lib.lib().nlml_project_identity_ex(A.data_ptr(), A.shape[0], A.shape[1], U.data_ptr(), U.shape[1], out.data_ptr(),
                                                       out_f64, stream), "nlml_project_identity")
    return out


def project_pose(X: torch.Tensor, U_yaw=None, U_pitch=None, U_roll=None, out_dtype=torch.float32) -> torch.Tensor:
    """K7d: X f32[I,ny,np,nr,M] (or f64) x_2 U_yaw^T x_3 U_pitch^T x_4 U_roll^T -> f32[I,ny',np',nr',M] (or f64, unrounded); each factor
    f64[n,r] (r <= 3) or None, which leaves that mode as it is.  With all three None the result is a copy of X."""
    X = _tensor5(X)
    out_f64 = _out_f64(out_dtype)
    shape = list(X.shape)
    Us = []
    for k, (U, name) in enumerate(((U_yaw, "U_yaw"), (U_pitch, "U_pitch"), (U_roll, "U_roll"))):
        if U is not None:
            _need_cuda(U, name, torch.float64)
            if U.dim() != 2 or U.shape[0] != X.shape[1 + k] or not 1 <= U.shape[1] <= _lib.POSE_RANK_MAX:
                raise ValueError(f"{name}: expected [{X.shape[1 + k]}, r] with 1 <= r <= {_lib.POSE_RANK_MAX}, got {tuple(U.shape)}")
            U = U.contiguous()
            shape[1 + k] = U.shape[1]
        Us.append(U)
    out = torch.empty(shape, dtype=out_dtype, device=X.device)
    args = [a for U in Us for a in ((U.data_ptr(), U.shape[1]) if U is not None else (None, 0))]
    with _on_device_of(("X", X), ("U_yaw", Us[0]), ("U_pitch", Us[1]), ("U_roll", Us[2])) as stream:
        _lib.check(_lib.lib().nlml_project_pose_ex(X.data_ptr(), int(X.dtype == torch.float64), *X.shape, *args, out.data_ptr(), out_f64,
                                                   stream), "nlml_project_pose")
    return out


# ---- K11: expand a Tucker model and compare it with the tensor in one pass (csrc/tucker_residual.hip) ---------------------------
def _tucker_model(W: torch.Tensor, U_id: torch.Tensor, U_yaw: torch.Tensor, U_pitch: torch.Tensor, U_roll: torch.Tensor):
    """-> (W, [U_id, U_yaw, U_pitch, U_roll]) contiguous, checked against each other: W f32[R,ry,rp,rr,M], every factor f64[n,r]."""
    _need_cuda(W, "W", torch.float32)
    if W.dim() != 5 or min(W.shape) < 1:
        raise ValueError(f"W: expected a non-empty [R,ry,rp,rr,M], got {tuple(W.shape)}")
    if not _lib.TUCKER_RANK_MIN <= W.shape[0] <= _lib.TUCKER_RANK_MAX or max(W.shape[1:4]) > _lib.POSE_RANK_MAX:
        raise ValueError(f"W: identity rank in [{_lib.TUCKER_RANK_MIN}, {_lib.TUCKER_RANK_MAX}] and pose ranks <= {_lib.POSE_RANK_MAX} "
                         f"expected, got {tuple(W.shape)}")
    Us = []
    for k, (U, name) in enumerate(((U_id, "U_id"), (U_yaw, "U_yaw"), (U_pitch, "U_pitch"), (U_roll, "U_roll"))):
        _need_cuda(U, name, torch.float64)
        if U.dim() != 2 or U.shape[0] < 1 or U.shape[1] != W.shape[k]:
            raise ValueError(f"{name}: expected [n, {W.shape[k]}] (W is {tuple(W.shape)}), got {tuple(U.shape)}")
        if k and U.shape[0] > _lib.POSE_BINS_MAX:
            raise ValueError(f"{name}: at most {_lib.POSE_BINS_MAX} bins per pose mode, got {U.shape[0]}")
        Us.append(U.contiguous())
    return W.contiguous(), Us


def tucker_residual(X, W: torch.Tensor, U_id: torch.Tensor, U_yaw: torch.Tensor, U_pitch: torch.Tensor, U_roll: torch.Tensor,
                    want_res_id: bool = False, want_xhat: bool = False):
    """K11: X f32[I,ny,np,nr,M] against the Tucker model (W f32[R,ry,rp,rr,M], factors f64[n,r]) in one pass over X ->
    (sums f64[2] = {sum (X - X_hat)^2, sum X^2}, res_id f64[I] or None, xhat f32[I,ny,np,nr,M] or None); the relative reconstruction
    error is sqrt(sums[0] / sums[1]).  X = None: expand only -> (None, None, xhat).  The same bits on every call."""
    W, Us = _tucker_model(W, U_id, U_yaw, U_pitch, U_roll)
    shape = tuple(U.shape[0] for U in Us) + (W.shape[4],)
    if X is None:
        want_xhat, want_res_id = True, False
    else:
        X = _tensor5(X)
        if X.dtype != torch.float32 or tuple(X.shape) != shape:
            raise ValueError(f"X: expected float32 {shape} (the factors' rows by W's columns), got {X.dtype} {tuple(X.shape)}")
    dev = W.device
    I, ny, np_, nr, M = shape
    sums = torch.empty((2,), dtype=torch.float64, device=dev) if X is not None else None
    res_id = torch.empty((I,), dtype=torch.float64, device=dev) if want_res_id else None
    xhat = torch.empty(shape, dtype=torch.float32, device=dev) if want_xhat else None
    ws = _k7_workspace(_lib.lib().nlml_tucker_residual_workspace_bytes(I, ny, np_, nr, M), dev) if X is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    with _on_device_of(("W", W), ("X", X), ("U_id", Us[0]), ("U_yaw", Us[1]), ("U_pitch", Us[2]), ("U_roll", Us[3])) as stream:
        _lib.check(_lib.lib().nlml_tucker_residual(ptr(X), W.data_ptr(), *[U.data_ptr() for U in Us], I, ny, np_, nr, M, *W.shape[:4],
                                                   ptr(sums), ptr(res_id), ptr(xhat), ptr(ws), ws.numel() * 8 if ws is not None else 0,
                                                   stream), "nlml_tucker_residual")
    return sums, res_id, xhat


def tucker_to_tensor(W: torch.Tensor, U_id: torch.Tensor, U_yaw: torch.Tensor, U_pitch: torch.Tensor, U_roll: torch.Tensor) -> torch.Tensor:
    """K11's expand-only form: W x_1 U_id x_2 U_yaw x_3 U_pitch x_4 U_roll -> f32[I,ny,np,nr,M], f64 sums, one rounding (tensorly's
    tucker_to_tensor; a one-row U_id gives one identity)."""
    return tucker_residual(None, W, U_id, U_yaw, U_pitch, U_roll)[2]


# ---- K8: the cosine fit of the pose factors (csrc/cosine_fit.hip; the driver is nlml_hpe_amd/TD_Trainer.py) -------------------
def _fit_rows(y: torch.Tensor, w_deg: torch.Tensor):
    _need_cuda(y, "y", torch.float64)
    _need_cuda(w_deg, "w_deg", torch.float64)
    if y.dim() != 2 or w_deg.shape != y.shape:
        raise ValueError(f"y and w_deg: expected two [C,ld] tensors of one shape, got {tuple(y.shape)}, {tuple(w_deg.shape)}")
    return y.contiguous(), w_deg.contiguous()


def cosine_fit(y: torch.Tensor, w_deg: torch.Tensor, n, x0: torch.Tensor, xtol: float = 1e-4, ftol: float = 1e-4):
    """K8: C independent fits of a cos(b radians(w) + c) + d, each scipy's minimize(objective, x0, method='Powell') of
    TD_Trainer.objective (TD_Trainer.py:37-42,81-88), in one launch.

    y f64[C,ld] the samples and w_deg f64[C,ld] their angles in degrees, row f holding fit f's n[f] values first; n the row counts
    (a sequence or an integer tensor [C], 1 <= n[f] <= min(64, ld); an int: the same for every fit); x0 f64[C,4] the starts.

    Returns dict(x=f64[C,4] (a, b, c, d), fun=f64[C], nfev=i32[C], nit=i32[C], status=i32[C]); status as tucker_powell's.  A fit's
    result does not depend on its place in the batch.
    """
    y, w_deg = _fit_rows(y, w_deg)
    _need_cuda(x0, "x0", torch.float64)
    Cn, ld = y.shape
    if tuple(x0.shape) != (Cn, 4):
        raise ValueError(f"x0: expected [{Cn},4], got {tuple(x0.shape)}")
    if isinstance(n, int):
        n = [n] * Cn
    h_n = torch.as_tensor(n.detach().cpu() if torch.is_tensor(n) else list(n)).to(torch.int32).contiguous()
    if tuple(h_n.shape) != (Cn,):
        raise ValueError(f"n: expected {Cn} row counts, got shape {tuple(h_n.shape)}")
    if Cn and (int(h_n.min()) < 1 or int(h_n.max()) > min(_lib.COSINE_FIT_ROWS_MAX, ld)):
        raise ValueError(f"n: every row count must be in [1, min({_lib.COSINE_FIT_ROWS_MAX}, ld = {ld})], got {int(h_n.min())}..{int(h_n.max())}")
    dev = y.device
    x0 = x0.contiguous()
    d_n = h_n.to(dev)
    res = torch.empty((Cn, 4), dtype=torch.float64, device=dev)
    fun = torch.empty((Cn,), dtype=torch.float64, device=dev)
    nfev = torch.empty((Cn,), dtype=torch.int32, device=dev)
    nit = torch.empty((Cn,), dtype=torch.int32, device=dev)
    status = torch.empty((Cn,), dtype=torch.int32, device=dev)
    with _on_device_of(("y", y), ("w_deg", w_deg), ("x0", x0)) as stream:
        _lib.check(_lib.lib().nlml_cosine_fit(y.data_ptr(), w_deg.data_ptr(), ld, d_n.data_ptr(), h_n.data_ptr(), Cn, x0.data_ptr(),
                                              float(xtol), float(ftol), res.data_ptr(), fun.data_ptr(), nfev.data_ptr(), nit.data_ptr(),
                                              status.data_ptr(), stream), "nlml_cosine_fit")
    return {"x": res, "fun": fun, "nfev": nfev, "nit": nit, "status": status}


def cosine_fit_objective(y: torch.Tensor, w_deg: torch.Tensor, n, params: torch.Tensor, fit: int = 0) -> torch.Tensor:
    """The objective K8 minimises, evaluated on the device at params f64[N,4] against the rows of fit `fit` of y / w_deg f64[C,ld]
    (n as in cosine_fit) -> f64[N]: 1/2 sum_i (y_i - (a cos(b radians(w_i) + c) + d))^2 in the reference's operation order."""
    y, w_deg = _fit_rows(y, w_deg)
    _need_cuda(params, "params", torch.float64)
    if params.dim() != 2 or params.shape[1] != 4:
        raise ValueError(f"params: expected [N,4], got {tuple(params.shape)}")
    Cn, ld = y.shape
    fit = int(fit)
    if not 0 <= fit < Cn:
        raise ValueError(f"fit: {fit} outside [0, {Cn})")
    rows = int(n) if isinstance(n, int) else int(n[fit])
    if not 1 <= rows <= min(_lib.COSINE_FIT_ROWS_MAX, ld):
        raise ValueError(f"n: {rows} outside [1, min({_lib.COSINE_FIT_ROWS_MAX}, ld = {ld})]")
    params = params.contiguous()
    N = params.shape[0]
    out = torch.empty((N,), dtype=torch.float64, device=y.device)
    with _on_device_of(("y", y), ("w_deg", w_deg), ("params", params)) as stream:
        _lib.check(_lib.lib().nlml_cosine_fit_objective(y[fit].data_ptr(), w_deg[fit].data_ptr(), rows, params.data_ptr(), N,
                                                        out.data_ptr(), stream), "nlml_cosine_fit_objective")
    return out


# ---- K9: training steps of the encoder (csrc/encoder_train.hip; the driver is nlml_hpe_amd/EncoderTrainer.py) ------------------
def encoder_param_count(F: int) -> int:
    """Elements of the contiguous params / grads buffers W0,b0,...,W5,b5 for input width F."""
    total, fan_in = 0, int(F)
    for w in (1024, 512, 256, 128, 64, LATENT):
        total += w * fan_in + w
        fan_in = w
    return total


def encoder_param_views(buf, F: int) -> dict:
    """The state dict `encoder.{0,2,..,10}.{weight,bias}` as VIEWS of a contiguous params (or grads) buffer."""
    from .EncoderTrainer import state_dict_views
    return state_dict_views(buf, F)


def _encoder_dataset(x, labels, tables, params, order, n, batch):
    _need_cuda(x, "x", torch.float32)
    _need_cuda(labels, "labels", torch.int32)
    _need_cuda(params, "params", torch.float32)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] not in (136, F_REF) or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        raise ValueError(f"x: expected [N,136] or [N,1404] with unit column stride, got {tuple(x.shape)} strides {x.stride()}")
    N, F = x.shape
    if labels.dim() != 2 or labels.shape[0] != N or labels.shape[1] < 3:
        raise ValueError(f"labels: expected [{N},>=3], got {tuple(labels.shape)}")
    if len(tables) != 3:
        raise ValueError("tables: expected (t_yaw, t_pitch, t_roll)")
    tables = list(tables)
    for k, t in enumerate(tables):
        _need_cuda(t, "a target table", torch.float32)
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != 3:
            raise ValueError(f"a target table: expected [rows,3], got {tuple(t.shape)}")
        tables[k] = t.contiguous()
    if not params.is_contiguous() or params.numel() != encoder_param_count(F):
        raise ValueError(f"params: expected a contiguous buffer of {encoder_param_count(F)} elements, got {tuple(params.shape)}")
    batch = int(batch)
    if not 1 <= batch <= _lib.ENCODER_TRAIN_BATCH_MAX:
        raise ValueError(f"batch = {batch} outside [1, {_lib.ENCODER_TRAIN_BATCH_MAX}]")
    if order is not None:
        _need_cuda(order, "order", torch.int32)
        if order.dim() != 1:
            raise ValueError(f"order: expected a vector, got {tuple(order.shape)}")
        order = order.contiguous()
        n = order.shape[0] if n is None else int(n)
        if n > order.shape[0]:
            raise ValueError(f"n = {n} beyond the {order.shape[0]} entries of order")
    else:
        n = N if n is None else int(n)
        if n > N:
            raise ValueError(f"n = {n} beyond the {N} rows of x")
    if n < 0:
        raise ValueError("negative n")
    return labels.contiguous(), tables, order, n, batch, N, F


def _encoder_workspace(F, batch, workspace, device):
    need = _lib.lib().nlml_encoder_train_workspace_bytes(F, batch)
    if workspace is None:
        return torch.empty((need,), dtype=torch.uint8, device=device)
    if not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"workspace: expected a contiguous GPU buffer of at least {need} bytes")
    return workspace


def _table_args(tables):
    return [v for t in tables for v in (t.data_ptr(), t.shape[0])]


def encoder_train_steps(x, labels, tables, params, grads, order=None, n=None, batch=256, lr=1e-4, weight_decay=1e-5, max_norm=20.0,
                        zero_grad=False, workspace=None):
    """K9: ceil(n / batch) consecutive training steps of the encoder (NLML_HPE_EncoderTrainer.py:400-454) enqueued without a
    synchronisation: forward, the three-MSE loss, backward into the persistent accumulator `grads` (the reference never calls
    zero_grad; zero_grad=True overwrites it instead), clip_grad_norm_(max_norm) in place, SGD with weight decay.

    x f32[N,F] (F 136 or 1404; a padded row stride is fine), labels i32[N,>=3], tables (t_yaw, t_pitch, t_roll) f32[.,3],
    params / grads contiguous f32[encoder_param_count(F)] updated IN PLACE (encoder_param_views gives the state dict),
    order i32[n] the rows in visiting order (None: 0..n-1).
    -> (loss f32[steps], norm f32[steps] before clipping, status i32[1]: _lib.ENCODER_TRAIN_CLAMPED_* bits) on the device."""
    labels, tables, order, n, batch, N, F = _encoder_dataset(x, labels, tables, params, order, n, batch)
    _need_cuda(grads, "grads", torch.float32)
    if not grads.is_contiguous() or grads.numel() != params.numel():
        raise ValueError(f"grads: expected a contiguous buffer of {params.numel()} elements, got {tuple(grads.shape)}")
    dev = x.device
    steps = (n + batch - 1) // batch
    loss = torch.empty((steps,), dtype=torch.float32, device=dev)
    norm = torch.empty((steps,), dtype=torch.float32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = _encoder_workspace(F, batch, workspace, dev)
    with _on_device_of(("x", x), ("labels", labels), ("t_yaw", tables[0]), ("t_pitch", tables[1]), ("t_roll", tables[2]), ("params", params),
                       ("grads", grads), ("order", order), ("workspace", ws)) as stream:
        _lib.check(_lib.lib().nlml_encoder_train_steps(
            x.data_ptr(), x.stride(0), N, labels.data_ptr(), labels.shape[1], *_table_args(tables), params.data_ptr(), grads.data_ptr(), F,
            batch, order.data_ptr() if order is not None else None, n, float(lr), float(weight_decay), float(max_norm), int(bool(zero_grad)),
            loss.data_ptr(), norm.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), stream),
            "nlml_encoder_train_steps")
    return loss, norm, status


def encoder_eval_losses(x, labels, tables, params, order=None, n=None, batch=256, workspace=None):
    """The validation pass of K9: forward and loss only, batch after batch -> (loss f32[steps], status i32[1]) on the device.  The
    forward is the training step's, bit for bit."""
    labels, tables, order, n, batch, N, F = _encoder_dataset(x, labels, tables, params, order, n, batch)
    dev = x.device
    steps = (n + batch - 1) // batch
    loss = torch.empty((steps,), dtype=torch.float32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = _encoder_workspace(F, batch, workspace, dev)
    with _on_device_of(("x", x), ("labels", labels), ("t_yaw", tables[0]), ("t_pitch", tables[1]), ("t_roll", tables[2]), ("params", params),
                       ("order", order), ("workspace", ws)) as stream:
        _lib.check(_lib.lib().nlml_encoder_eval_losses(
            x.data_ptr(), x.stride(0), N, labels.data_ptr(), labels.shape[1], *_table_args(tables), params.data_ptr(), F, batch,
            order.data_ptr() if order is not None else None, n, loss.data_ptr(), status.data_ptr(), ws.data_ptr(),
            ws.numel() * ws.element_size(), stream), "nlml_encoder_eval_losses")
    return loss, status


# ---- K10: training steps of the three heads (csrc/heads_train.hip; the driver is nlml_hpe_amd/MLPHeadsTrainer.py) ----------------
def heads_param_count(R: int) -> int:
    """Elements of a head network's contiguous params / grads / m / v buffers W0,b0,...,W4,b4 for input width R (74,753 at R = 3)."""
    from .MLPHeadsTrainer import param_count
    return param_count(R)


def heads_param_views(buf, R: int) -> dict:
    """The state dict `model.{0,2,4,6,8}.{weight,bias}` as VIEWS of a contiguous params (grads, m, v) buffer, numpy or torch."""
    from .MLPHeadsTrainer import state_dict_views
    return state_dict_views(buf, R)


def _heads_nets(nets, batch, train):
    """Checks the networks of a K10 call (dicts: x, y, params[, grads, m, v][, order][, n][, step0]) -> (normalised dicts, R, batch)."""
    nets = [dict(net) for net in nets]
    if not 1 <= len(nets) <= _lib.HEADS_TRAIN_NETS_MAX:
        raise ValueError(f"expected 1..{_lib.HEADS_TRAIN_NETS_MAX} networks, got {len(nets)}")
    batch = int(batch)
    if not 1 <= batch <= _lib.ENCODER_TRAIN_BATCH_MAX:
        raise ValueError(f"batch = {batch} outside [1, {_lib.ENCODER_TRAIN_BATCH_MAX}]")
    R = None
    for i, net in enumerate(nets):
        x, y = net["x"], net["y"]
        _need_cuda(x, f"network {i}: x", torch.float32)
        _need_cuda(y, f"network {i}: y", torch.float32)
        if x.dim() != 2 or x.shape[0] < 1 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
            raise ValueError(f"network {i}: x: expected [N,R] with unit column stride, got {tuple(x.shape)} strides {x.stride()}")
        R = x.shape[1] if R is None else R
        if x.shape[1] != R or not 1 <= R <= _lib.HEADS_TRAIN_R_MAX:
            raise ValueError(f"network {i}: x has {x.shape[1]} columns: expected the same R in [1, {_lib.HEADS_TRAIN_R_MAX}] for every network")
        if y.dim() != 1 or y.shape[0] != x.shape[0]:
            raise ValueError(f"network {i}: y: expected [{x.shape[0]}], got {tuple(y.shape)}")
        net["y"] = y.contiguous()
        for key in ("params", "grads", "m", "v") if train else ("params",):
            t = net[key]
            _need_cuda(t, f"network {i}: {key}", torch.float32)
            if not t.is_contiguous() or t.numel() != heads_param_count(R):
                raise ValueError(f"network {i}: {key}: expected a contiguous buffer of {heads_param_count(R)} elements, got {tuple(t.shape)}")
        order = net.get("order")
        if order is not None:
            _need_cuda(order, f"network {i}: order", torch.int32)
            if order.dim() != 1:
                raise ValueError(f"network {i}: order: expected a vector, got {tuple(order.shape)}")
            net["order"] = order = order.contiguous()
        limit = order.shape[0] if order is not None else x.shape[0]
        n = limit if net.get("n") is None else int(net["n"])
        if not 1 <= n <= limit:
            raise ValueError(f"network {i}: n = {n} outside [1, {limit}]")
        net["n"] = n
        net["step0"] = int(net.get("step0") or 0)
        if net["step0"] < 0:
            raise ValueError(f"network {i}: negative step0")
    return nets, int(R), batch


def _heads_call(nets, R, batch, train, workspace):
    """The C array of nlml_heads_net, the outputs (loss, norm per network; status i32[n_nets]) and the workspace of a K10 call."""
    dev = nets[0]["x"].device
    arr = (_lib.HeadsNet * len(nets))()
    loss, norm = [], []
    status = torch.zeros((len(nets),), dtype=torch.int32, device=dev)
    for i, net in enumerate(nets):
        steps = (net["n"] + batch - 1) // batch
        loss.append(torch.empty((steps,), dtype=torch.float32, device=dev))
        norm.append(torch.empty((steps,), dtype=torch.float32, device=dev) if train else None)
        a = arr[i]
        a.x, a.ldx, a.N, a.y = net["x"].data_ptr(), net["x"].stride(0), net["x"].shape[0], net["y"].data_ptr()
        a.params = net["params"].data_ptr()
        if train:
            a.grads, a.m, a.v = net["grads"].data_ptr(), net["m"].data_ptr(), net["v"].data_ptr()
            a.norm_out = norm[i].data_ptr()
        a.order = net["order"].data_ptr() if net.get("order") is not None else None
        a.n, a.step0 = net["n"], net["step0"]
        a.loss_out, a.status = loss[i].data_ptr(), status.data_ptr() + 4 * i
    need = _lib.lib().nlml_heads_train_workspace_bytes(R, batch, len(nets))
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif not workspace.is_cuda or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"workspace: expected a contiguous GPU buffer of at least {need} bytes")
    operands = [(f"network {i}: {k}", net.get(k)) for i, net in enumerate(nets) for k in ("x", "y", "params", "grads", "m", "v", "order")]
    return arr, loss, norm, status, workspace, operands + [("workspace", workspace)]


def heads_train_steps(nets, batch=256, lr=5e-3, weight_decay=1e-5, max_norm=1.0, workspace=None):
    """K10: the training steps of up to three independent head networks (NLML_HPE_MLPHeadsTrainer.py:93-103) enqueued without a
    synchronisation, every launch shared by all of them: zero_grad, forward, MSELoss, backward, clip_grad_norm_(max_norm), Adam with
    L2 weight decay.  The call runs max_i ceil(n_i / batch) steps; a network whose rows are used up is left alone.

    nets  a sequence of dicts, one per network: x f32[N,R] (R 1..16, the same for all; a padded row stride is fine), y f32[N],
          params / grads / m / v contiguous f32[heads_param_count(R)] updated IN PLACE (heads_param_views gives the state dict),
          order i32[n] the rows in visiting order (absent or None: 0..n-1), n (default: all), step0 the Adam steps the network has
          taken before this call (default 0; the caller carries it: step0 += ceil(n / batch))
    -> (loss [f32[steps_i] per network], norm [f32[steps_i] before clipping], status i32[n_nets]: _lib.HEADS_TRAIN_CLAMPED_ORDER) on
    the device."""
    nets, R, batch = _heads_nets(nets, batch, True)
    arr, loss, norm, status, ws, operands = _heads_call(nets, R, batch, True, workspace)
    with _on_device_of(*operands) as stream:
        _lib.check(_lib.lib().nlml_heads_train_steps(C.addressof(arr), len(nets), R, batch, float(lr), float(weight_decay), float(max_norm),
                                                     ws.data_ptr(), ws.numel() * ws.element_size(), stream), "nlml_heads_train_steps")
    return loss, norm, status


def heads_eval_losses(nets, batch=256, workspace=None):
    """The validation pass of K10: forward and loss only, batch after batch, all networks in the same launches -> (loss [f32[steps_i]
    per network], status i32[n_nets]) on the device.  The forward is the training step's, bit for bit.  nets: x, y, params[, order, n]."""
    nets, R, batch = _heads_nets(nets, batch, False)
    arr, loss, _, status, ws, operands = _heads_call(nets, R, batch, False, workspace)
    with _on_device_of(*operands) as stream:
        _lib.check(_lib.lib().nlml_heads_eval_losses(C.addressof(arr), len(nets), R, batch, ws.data_ptr(), ws.numel() * ws.element_size(),
                                                     stream), "nlml_heads_eval_losses")
    return loss, status


# ---- K5 evaluation (nlml_pose_eval) -------------------------------------------------------------------------------------------
_eval_ws: dict = {}


def _eval_workspace(B: int, K: int, device) -> torch.Tensor:
    """The per-workgroup records of nlml_pose_eval (f64, 8-byte aligned), cached per device and stream; replaced when it must grow."""
    need = max(8, _lib.lib().nlml_pose_eval_workspace_bytes(B, K))
    key = (str(device), _stream_ptr(device))
    ws = _eval_ws.get(key)
    if ws is None or ws.numel() * 8 < need:
        ws = torch.empty(((need + 7) // 8,), dtype=torch.float64, device=device)
        _eval_ws[key] = ws
    return ws


def _eval_intervals(intervals):
    """[(axis, low, high), ...] -> (h_intervals f64[K,2], h_axes i32[K]) as ctypes arrays, K."""
    iv = [(int(a), float(lo), float(hi)) for a, lo, hi in intervals]
    K = len(iv)
    h_iv = (C.c_double * max(1, 2 * K))(*[v for _, lo, hi in iv for v in (lo, hi)])
    h_ax = (C.c_int32 * max(1, K))(*[a for a, _, _ in iv])
    return h_iv, h_ax, K


def pose_eval(pose: torch.Tensor, gt: torch.Tensor, valid: torch.Tensor | None = None, lo=None, hi=None, intervals=(), decimals: int = 3,
              return_per_face: bool = False, workspace: torch.Tensor | None = None):
    """The evaluation block of the test entry point in one native pass (nlml_pose_eval, two launches, no synchronisation).

    pose  f32[B,3] radians (the model's output; rounded as np.round(np.degrees(pose), decimals)) or f64[B,3] degrees (already
          post-processed; rounded only when decimals >= 0)
    gt    f64[B,3] degrees;  valid bool/u8[B] or None (every row has a face)
    lo, hi  3 floats, the inclusive GT range per axis (default: unbounded)
    intervals  [(axis, low, high), ...] half-open GT intervals, axis 0 yaw / 1 pitch / 2 roll, at most 64
    -> (record f64[12+2K], result f64[14+2K]) on the device (layouts: include/nlml_hpe.h, K5); with return_per_face also
       pred f64[B,3] and keep bool[B]."""
    if not pose.is_cuda:
        raise _lib.NlmlError(f"pose: expected a GPU tensor (there is no CPU fallback), got device {pose.device}")
    if pose.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"pose: expected float32 radians or float64 degrees, got {pose.dtype}")
    _need_cuda(gt, "gt", torch.float64)
    B = pose.shape[0]
    if pose.dim() != 2 or pose.shape[1] != 3 or tuple(gt.shape) != (B, 3):
        raise ValueError(f"pose and gt: expected [B,3] each, got {tuple(pose.shape)}, {tuple(gt.shape)}")
    if valid is not None:
        if not valid.is_cuda or valid.dtype not in (torch.bool, torch.uint8) or tuple(valid.shape) != (B,):
            raise ValueError(f"valid: expected a GPU bool/uint8 tensor [{B}], got {valid.dtype} {tuple(valid.shape)} on {valid.device}")
        valid = valid.contiguous()
        valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid
    pose, gt = pose.contiguous(), gt.contiguous()
    h_lo = (C.c_double * 3)(*([-float("inf")] * 3 if lo is None else [float(v) for v in lo]))
    h_hi = (C.c_double * 3)(*([float("inf")] * 3 if hi is None else [float(v) for v in hi]))
    h_iv, h_ax, K = _eval_intervals(intervals)
    L = _lib.lib()
    dev = pose.device
    ws = workspace if workspace is not None else _eval_workspace(B, K, dev)
    record = torch.empty((L.nlml_pose_eval_record_len(K) or 1,), dtype=torch.float64, device=dev)
    result = torch.empty((L.nlml_pose_eval_result_len(K) or 1,), dtype=torch.float64, device=dev)
    pred = torch.empty((B, 3), dtype=torch.float64, device=dev) if return_per_face else None
    keep = torch.empty((B,), dtype=torch.uint8, device=dev) if return_per_face else None
    f32 = pose.dtype == torch.float32
    with _on_device_of(("pose", pose), ("gt", gt), ("valid", valid), ("workspace", ws)) as stream:
        _lib.check(L.nlml_pose_eval(pose.data_ptr() if f32 else None, None if f32 else pose.data_ptr(),
                                    valid.data_ptr() if valid is not None else None, gt.data_ptr(), B, h_lo, h_hi, int(decimals),
                                    h_iv, h_ax, K, ws.data_ptr(), ws.numel() * ws.element_size(), record.data_ptr(), result.data_ptr(),
                                    pred.data_ptr() if pred is not None else None, keep.data_ptr() if keep is not None else None, stream),
                   "nlml_pose_eval")
    if return_per_face:
        return record, result, pred, keep.bool()
    return record, result


def pose_eval_merge(records: torch.Tensor, K: int):
    """Merge records f64[n, 12+2K] (several calls or ranks, in order) as nlml_pose_eval merges its own -> (record, result)."""
    _need_cuda(records, "records", torch.float64)
    Lr = _lib.lib().nlml_pose_eval_record_len(int(K))
    if Lr == 0:
        raise ValueError(f"K = {K}: at most {_lib.POSE_EVAL_MAX_INTERVALS} intervals")
    if records.dim() != 2 or records.shape[1] != Lr:
        raise ValueError(f"records: expected [n,{Lr}], got {tuple(records.shape)}")
    records = records.contiguous()
    dev = records.device
    record = torch.empty((Lr,), dtype=torch.float64, device=dev)
    result = torch.empty((_lib.lib().nlml_pose_eval_result_len(int(K)),), dtype=torch.float64, device=dev)
    with _on_device_of(("records", records)) as stream:
        _lib.check(_lib.lib().nlml_pose_eval_merge(records.data_ptr(), records.shape[0], int(K), record.data_ptr(), result.data_ptr(),
                                                   stream), "nlml_pose_eval_merge")
    return record, result


# ---------------------------------------------------------------------------------------------
# torch.ops.nlml_hpe.* (SURVEY.md 8b "Underlying op") come from COMPILED code: csrc/torch_ops.cpp, a TORCH_LIBRARY shim over the same
# C ABI (shape / dtype checks, torch's allocator, the operand device's current stream), built next to this file as
# libnlml_torch_ops.so by csrc/Makefile.  GPU backend only: a CPU tensor has no kernel to dispatch to and raises.  A missing library
# raises here -- the ops are part of the boundary.
TORCH_OPS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libnlml_torch_ops.so")


def _load_torch_ops():
    if not os.path.exists(TORCH_OPS_PATH):
        raise _lib.NlmlError(f"{TORCH_OPS_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(make -C nlml_hpe_amd/csrc); torch.ops.nlml_hpe.* are registered from it")
    _lib.lib()                                  # the C ABI library the shim links against, checked symbol by symbol first
    torch.ops.load_library(TORCH_OPS_PATH)
    # the registered ops; *_small take an explicit workspace, landmarks_to_pose_valid is the video tick's forward (pose + face mask)
    for name in ("normalize_ipd", "normalize_centroid", "encoder_heads_fwd", "landmarks_to_pose", "encoder_heads_fwd_small", "landmarks_to_pose_small",
                 "landmarks_to_pose_valid", "tucker_objective", "tucker_gradient", "tucker_powell", "video_post", "cosine_table", "pose_eval",
                 "pose_eval_merge", "compose_rotation_tensor", "rotate_landmarks", "mode_gram", "pose_grams", "project_identity",
                 "project_pose", "cosine_fit", "encoder_train_steps", "heads_train_steps", "tucker_residual"):
        getattr(torch.ops.nlml_hpe, name)       # AttributeError if the library did not register it


_load_torch_ops()
