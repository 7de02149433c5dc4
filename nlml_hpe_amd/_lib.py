"""ctypes binding of libnlml_hpe_hip.so -- the C ABI declared in include/nlml_hpe.h.

The library is built in-tree by ``nlml_hpe_amd/csrc/Makefile`` (``__graft_entry__.build()``)
and loaded from next to this file.  There is NO fallback: if the library is missing or a
symbol is absent, importing the ops raises -- the product path never routes through CPU code.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NLML_HPE_LIB overrides the path (A/B experiments with alternative builds); default: the in-tree build
LIB_PATH = os.environ.get("NLML_HPE_LIB") or os.path.join(_HERE, "libnlml_hpe_hip.so")

# Every symbol include/nlml_hpe.h declares: (restype, argtypes)
_c_f32p = C.c_void_p
# the K2 forwards: two argument shapes, (x, ldx, B, F | raw, B, normalize) + (blob, blob_bytes, out, latent, valid) [+ (workspace, ws_bytes)]
# + stream
_FWD_X = [C.c_void_p, C.c_int64, C.c_int64, C.c_int]
_FWD_RAW = [C.c_void_p, C.c_int64, C.c_int]
_FWD_OUT = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
_FWD_WS = [C.c_void_p, C.c_size_t]


def _k2_forwards():
    for form, ws in (("", []), ("_small", _FWD_WS), ("_streamed", _FWD_WS), ("_quad", _FWD_WS), ("_ws", _FWD_WS)):
        yield "nlml_encoder_heads_fwd" + form, (C.c_int, _FWD_X + _FWD_OUT + ws + [C.c_void_p])
        yield "nlml_landmarks_to_pose" + form, (C.c_int, _FWD_RAW + _FWD_OUT + ws + [C.c_void_p])


# the TD entry points: Wm, x, ldx, x_index, params, cos_params, N, err, x_hat | grad (objective, gradient) or Wm, x, ldx, cos_params, N, x0,
# result, fval, nfev, nit, status (Powell), + nothing | order | r_id, order (plain, _ex, _r) + stream
_TD_EVAL = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
_TD_POWELL = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 6


def _td_entries():
    for op, head in (("objective", _TD_EVAL), ("powell", _TD_POWELL)):
        for form, tail in (("", []), ("_ex", [C.c_int]), ("_r", [C.c_int, C.c_int])):
            yield f"nlml_tucker_{op}{form}", (C.c_int, head + tail + [C.c_void_p])
    # K3g: ..., r_id, workspace, workspace_bytes, stream | ..., r_id, h_v
    yield "nlml_tucker_gradient_r", (C.c_int, _TD_EVAL + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p])
    yield "nlml_tucker_gradient_host", (C.c_int, _TD_EVAL + [C.c_int, C.c_void_p])


_ROT_GRID = ([C.c_void_p, C.c_int64] + [C.c_void_p, C.c_int] * 3 + [C.c_int] * 4 + [C.c_void_p, C.c_void_p])

# K9: x, ldx, N, labels, ld_lab, (table, rows) x 3 | F, batch, order, n | lr, weight_decay, max_norm, zero_grad
_ET_DATA = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p, C.c_int] * 3
_ET_RUN = [C.c_int, C.c_int, C.c_void_p, C.c_int64]
_ET_HYPER = [C.c_double, C.c_double, C.c_double, C.c_int]



class HeadsNet(C.Structure):
    """nlml_heads_net: one network of a K10 call (include/nlml_hpe.h)."""
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int64), ("N", C.c_int64), ("y", C.c_void_p), ("params", C.c_void_p), ("grads", C.c_void_p),
                ("m", C.c_void_p), ("v", C.c_void_p), ("order", C.c_void_p), ("n", C.c_int64), ("step0", C.c_int64),
                ("loss_out", C.c_void_p), ("norm_out", C.c_void_p), ("status", C.c_void_p)]


# K10: nets, n_nets, R, batch[, lr, weight_decay, max_norm], workspace, workspace_bytes[, stream]
_HT_CALL = [C.c_void_p, C.c_int, C.c_int, C.c_int]

SYMBOLS = {
    **dict(_k2_forwards()),
    **dict(_td_entries()),
    "nlml_abi_version": (C.c_int, []),
    "nlml_last_error": (C.c_char_p, []),
    "nlml_normalize_ipd": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # raw, B, out, valid, stats[, stream]
    "nlml_normalize_centroid": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlml_normalize_centroid_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    # K6: base, I, rot_yaw, ny, rot_pitch, np, rot_roll, nr, order, zero_yaw, zero_pitch, zero_roll, out, out64[, stream]
    "nlml_compose_rotation_tensor": (C.c_int, _ROT_GRID + [C.c_void_p]),
    "nlml_compose_rotation_tensor_host": (C.c_int, _ROT_GRID),
    # lm, rot, out, out64, B[, stream]
    "nlml_rotate_landmarks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "nlml_rotate_landmarks_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "nlml_encoder_heads_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "nlml_encoder_heads_pack": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t]),
    "nlml_encoder_heads_fwd_debug": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_size_t,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlml_encoder_heads_small_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "nlml_encoder_heads_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "nlml_k2_quad_split": (C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_int64)]),
    # rows, ld, B, F, blob_bytes, quad_faces, ws_bytes
    "nlml_k2_quad_part": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]),
    "nlml_k2_quad_faces": (C.c_int, [C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]),
    "nlml_k2_small_batch_max": (C.c_int64, [C.c_int]),
    "nlml_tucker_gradient_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "nlml_video_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double,
                                  C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlml_video_post_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double,
                                     C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlml_pose_eval_record_len": (C.c_size_t, [C.c_int]),
    "nlml_pose_eval_result_len": (C.c_size_t, [C.c_int]),
    "nlml_pose_eval_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "nlml_pose_eval": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "nlml_pose_eval_merge": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlml_cosine_table": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nlml_mode5_product": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # K7 (Tucker decomposition): A, I, K, G, ws, ws_bytes | X, I, ny, np, nr, M, Gy, Gp, Gr, ws, ws_bytes | A, I, K, U, R, out |
    # X, I, ny, np, nr, M, (U, rank) x 3, out; + stream
    "nlml_mode_gram_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "nlml_mode_gram": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "nlml_pose_grams_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64]),
    "nlml_pose_grams": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "nlml_project_identity": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "nlml_project_pose": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64] + [C.c_void_p, C.c_int] * 3
                          + [C.c_void_p, C.c_void_p]),
    # the same with an f64 tensor in or out where the flag after its pointer is nonzero
    "nlml_mode_gram_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "nlml_pose_grams_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "nlml_project_identity_ex": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "nlml_project_pose_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64] + [C.c_void_p, C.c_int] * 3
                             + [C.c_void_p, C.c_int, C.c_void_p]),
    # K11 (expand and compare): X, W, U_id, Uy, Up, Ur, I, ny, np, nr, M, R, ry, rp, rr, sums, res_id, xhat, ws, ws_bytes[, stream]
    "nlml_tucker_residual_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64]),
    "nlml_tucker_residual": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64] + [C.c_int] * 4
                             + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "nlml_tucker_residual_host": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64] + [C.c_int] * 4
                                  + [C.c_void_p] * 4 + [C.c_size_t]),
    # K8 (cosine fit): y, w_deg, ld, [n,] h_n, C, x0, xtol, ftol, x, fun, nfev, nit, status[, stream] | y, w_deg, n, params, N, out[, stream]
    "nlml_cosine_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_double]
                        + [C.c_void_p] * 6),
    "nlml_cosine_fit_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_double]
                             + [C.c_void_p] * 5),
    "nlml_cosine_fit_objective": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "nlml_cosine_fit_objective_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    # K9 (encoder training): the dataset and tables, then params[, grads], F, batch, order, n[, lr, weight_decay, max_norm, zero_grad],
    # loss_out[, norm_out], status[, workspace, workspace_bytes, stream]
    "nlml_encoder_train_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "nlml_encoder_train_steps": (C.c_int, _ET_DATA + [C.c_void_p, C.c_void_p] + _ET_RUN + _ET_HYPER + [C.c_void_p] * 3
                                 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nlml_encoder_eval_losses": (C.c_int, _ET_DATA + [C.c_void_p] + _ET_RUN + [C.c_void_p] * 2 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nlml_encoder_train_steps_host": (C.c_int, _ET_DATA + [C.c_void_p, C.c_void_p] + _ET_RUN + _ET_HYPER + [C.c_void_p] * 3),
    "nlml_encoder_eval_losses_host": (C.c_int, _ET_DATA + [C.c_void_p] + _ET_RUN + [C.c_void_p] * 2),
    "nlml_heads_train_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "nlml_heads_train_steps": (C.c_int, _HT_CALL + [C.c_double] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nlml_heads_eval_losses": (C.c_int, _HT_CALL + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "nlml_heads_train_steps_host": (C.c_int, _HT_CALL + [C.c_double] * 3 + [C.c_void_p, C.c_size_t]),
    "nlml_heads_eval_losses_host": (C.c_int, _HT_CALL + [C.c_void_p, C.c_size_t]),
    "nlml_powell_state_bytes": (C.c_size_t, []),
    "nlml_powell_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double]),
    "nlml_powell_step": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "nlml_powell_result": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlml_powell_state_bytes_n": (C.c_size_t, [C.c_int]),
    "nlml_powell_init_n": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double]),
    "nlml_powell_step_n": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "nlml_powell_result_n": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

MODE_F32 = 0
MODE_BF16 = 1
MODE_F16X2 = 2
MODE_F16X2S = 3
MODE_NAMES = {"f32": MODE_F32, "bf16": MODE_BF16, "f16x2": MODE_F16X2, "f16x2s": MODE_F16X2S}
# What load_model / resolve_model / bench.py / NLML_HPE_MODE fall back to: the strict-fast mode -- at the reference's operating range
# 0.88x the pinned reference's distance from the exact result (FX3c) / 1.14x torch-f32's on the GPU box's host; 0.03-0.07 % of the faces
# differ from the reference's batched output by more than 1e-4 deg (f32 mode: 0.002-0.012 %).  "f16x2" (1.10x the pinned reference's error) is opt-in.
DEFAULT_MODE = MODE_F16X2S
DEFAULT_MODE_NAME = "f16x2s"
TD_ORDER_FAST = 0          # GEMM on the f64 matrix cores (<= 1e-12 rel. of the reference's objective)
TD_ORDER_REFERENCE = 1     # np.einsum's own operation order + numpy's pairwise sum: the reference's bits
TD_ORDER_NAMES = {"fast": TD_ORDER_FAST, "reference": TD_ORDER_REFERENCE}
ROT_INTRINSIC = 0          # NLML_ROT_INTRINSIC: stages pitch, yaw, roll
ROT_EXTRINSIC = 1          # NLML_ROT_EXTRINSIC: stages roll, yaw, pitch, the matrices transposed by the caller
ROT_ORDER_NAMES = {"intrinsic": ROT_INTRINSIC, "extrinsic": ROT_EXTRINSIC}
TUCKER_RANK_MIN, TUCKER_RANK_MAX = 1, 16  # NLML_TUCKER_RANK_MIN / NLML_TUCKER_RANK_MAX: identity ranks of the *_r entry points
MODE_GRAM_I_MAX = 4096             # NLML_GRAM_I_MAX
MODE_GRAM_KCHUNK = 4096            # NLML_GRAM_KCHUNK: the least columns of a K slice of nlml_mode_gram
POSE_BINS_MAX = 32                 # NLML_POSE_BINS_MAX
POSE_GRAMS_MAX_CELLS = 768         # NLML_POSE_GRAMS_MAX_CELLS
POSE_RANK_MAX = 3                  # NLML_POSE_RANK_MAX
COSINE_FIT_ROWS_MAX = 64          # NLML_COSINE_FIT_ROWS_MAX
ENCODER_TRAIN_BATCH_MAX = 256      # NLML_ENCODER_TRAIN_BATCH_MAX
ENCODER_TRAIN_CLAMPED_ORDER = 1    # NLML_ENCODER_TRAIN_CLAMPED_ORDER
ENCODER_TRAIN_CLAMPED_LABEL = 2    # NLML_ENCODER_TRAIN_CLAMPED_LABEL
HEADS_TRAIN_NETS_MAX = 3           # NLML_HEADS_TRAIN_NETS_MAX
HEADS_TRAIN_R_MAX = 16             # NLML_HEADS_TRAIN_R_MAX
HEADS_TRAIN_CLAMPED_ORDER = 1      # NLML_HEADS_TRAIN_CLAMPED_ORDER
HEADS_WIDTHS = (128, 256, 128, 64, 1)
POSE_EVAL_MAX_INTERVALS = 64       # NLML_POSE_EVAL_MAX_INTERVALS
POSE_EVAL_FACES_PER_RECORD = 2048  # NLML_POSE_EVAL_FACES_PER_RECORD


def td_order_from_name(order) -> int:
    if isinstance(order, str):
        if order not in TD_ORDER_NAMES:
            raise ValueError(f"unknown TD order {order!r}; expected one of {sorted(TD_ORDER_NAMES)}")
        return TD_ORDER_NAMES[order]
    if int(order) not in TD_ORDER_NAMES.values():
        raise ValueError(f"unknown TD order {order!r}")
    return int(order)


def rot_order_from_name(order) -> int:
    """Accepts a NLML_ROT_* constant or the reference's rotation_type string ("intrinsic", "extrinsic")."""
    if isinstance(order, str):
        if order not in ROT_ORDER_NAMES:
            raise ValueError("Rotation type must be 'intrinsic' or 'extrinsic'.")
        return ROT_ORDER_NAMES[order]
    if int(order) not in ROT_ORDER_NAMES.values():
        raise ValueError(f"unknown rotation order {order!r}")
    return int(order)


def tucker_rank_of_rows(rows: int, what: str = "Wm") -> int:
    """Identity rank R of a Wm with `rows` = 27 R rows; ValueError (naming the range) for anything else."""
    r, rem = divmod(int(rows), 27)
    if rem or not TUCKER_RANK_MIN <= r <= TUCKER_RANK_MAX:
        raise ValueError(f"{what}: expected 27*R rows (R*3*3*3) for an identity rank R in [{TUCKER_RANK_MIN}, {TUCKER_RANK_MAX}], "
                         f"got {rows}")
    return r


def mode_from_name(mode) -> int:
    """Accepts a NLML_MODE_* constant or its name ("f32", "bf16", "f16x2", "f16x2s")."""
    if isinstance(mode, str):
        if mode not in MODE_NAMES:
            raise ValueError(f"unknown mode {mode!r}; expected one of {sorted(MODE_NAMES)}")
        return MODE_NAMES[mode]
    if int(mode) not in MODE_NAMES.values():
        raise ValueError(f"unknown mode {mode!r}")
    return int(mode)

_lib = None


class NlmlError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NlmlError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C nlml_hpe_amd/csrc).  There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if handle.nlml_abi_version() != 2:
            raise NlmlError("libnlml_hpe_hip.so ABI version mismatch")
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().nlml_last_error()
        raise NlmlError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
