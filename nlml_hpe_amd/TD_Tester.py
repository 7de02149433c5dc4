"""Host-side mirror of the reference's TD_Tester module on the HIP kernels.

Same names and argument meaning as /root/reference/TD_Tester.py for the functions on the hot path:
  func(w, params)                                  :25-28
  objective(params, W, x, params_y, params_p, params_r)   :31-58   -> float (one evaluation, K3 kernel)
  compute_gradient(params, W, x, params_y, params_p, params_r) :60-102 -> f64[8] (the jac= the reference hands to Powell)
  Test(W, x, u_id_shape, Py, Pp, Pr, u_id, f_y, f_p, f_r) :162-291 -> (yaw deg, pitch deg, roll deg, u_id)
plus the batched forms this build adds: objective_batch, compute_gradient_batch, value_and_gradient_batch, Test_batch.
The module-level debug lists of the reference (:18-22, appended on every call, unbounded) are not kept.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops

_cache: dict = {}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


RANK_MIN, RANK_MAX = _lib.TUCKER_RANK_MIN, _lib.TUCKER_RANK_MAX   # identity ranks u_id_shape the device path takes


def _rank(u_id_shape) -> int:
    r = int(u_id_shape)
    if not RANK_MIN <= r <= RANK_MAX:
        raise ValueError(f"u_id_shape = {u_id_shape}: the device path takes identity ranks {RANK_MIN}..{RANK_MAX} "
                         "(W of shape [R,3,3,3,1404], 3 + R parameters)")
    return r


def _wm(W) -> torch.Tensor:
    """W f32[R,3,3,3,1404] -> device f32[27R,1404], cached per array (W is immutable shipped data); R = 1..16."""
    key = (id(W), str(_dev()))
    hit = _cache.get(key)
    if hit is None or hit[0] is not W:
        Wn = np.ascontiguousarray(np.asarray(W, dtype=np.float32)).reshape(-1, 1404)
        # R*3*3*3 rows, R in RANK_MIN..RANK_MAX (TD_Inference.py:51-56 takes R from the artefact and the first 3 cosine rows)
        _lib.tucker_rank_of_rows(Wn.shape[0], "W.reshape(-1, 1404)")
        hit = (W, torch.from_numpy(Wn).to(_dev()))
        _cache[key] = hit
    return hit[1]


def _cos(params_y, params_p, params_r) -> torch.Tensor:
    cp = np.stack([np.asarray(params_y, dtype=np.float64), np.asarray(params_p, dtype=np.float64),
                   np.asarray(params_r, dtype=np.float64)])
    if cp.shape != (3, 3, 4):
        raise ValueError(f"cosine parameter blocks must be (3,4) each, got {cp.shape}")
    return torch.from_numpy(cp).to(_dev())


def _x(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x.detach().to(torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if t.dim() == 1:
        t = t.unsqueeze(0)
    return t.to(_dev()).contiguous()


def _stage(params, W, X, params_y, params_p, params_r, x_index=None):
    """The operands of the batched TD calls on the device -> (Wm f32[27R,1404], X f32[M,1404], P f64[N,3+R], cos f64[3,3,4],
    x_index i32[N] or None)."""
    Wm = _wm(W)
    P = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 3 + Wm.shape[0] // 27)).to(_dev())
    xi = None if x_index is None else torch.from_numpy(np.ascontiguousarray(x_index, dtype=np.int32)).to(_dev())
    return Wm, _x(X), P, _cos(params_y, params_p, params_r), xi


def func(w, params):
    a, b, c, d = params
    return a * np.cos(b * w + c) + d


# Operation order of the device objective.  "reference" = np.einsum's own loop order and numpy's pairwise sum: the reference's
# objective bit for bit, hence scipy's own Powell trajectory and final angles (FX4, FX5) -- the DEFAULT of every function here,
# batched or not: it is the parity mode.  "fast" (opt-in) = the GEMM form on the f64 matrix cores: objective <= 1e-12 relative,
# ~3x the faces/s, but Powell's end point then differs from scipy's wherever the minimum is flat: 6e-3 deg on FX5's clean grid
# faces; on BASELINE config 3's 4,096 noisy faces median 1.8e-3 deg (per face, largest of the three angles), 10 % of the faces > 0.02 deg, 0.3 % > 1 deg, max 8.7 deg.
ORDER_REFERENCE, ORDER_FAST = "reference", "fast"


def objective_batch(params, W, X, params_y, params_p, params_r, x_index=None, return_xhat=False, order=ORDER_REFERENCE):
    """params f64[N,3+R] (R = W's identity rank); X f32[M,1404] (M == N, or rows selected by x_index i32[N]) -> err f64[N] (numpy)."""
    Wm, Xd, P, cp, xi = _stage(params, W, X, params_y, params_p, params_r, x_index)
    out = ops.tucker_objective(Wm, Xd, P, cp, x_index=xi, return_xhat=return_xhat, order=order)
    if return_xhat:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def objective(params, W, x, params_y, params_p, params_r, order=ORDER_REFERENCE):
    """One evaluation, same signature as the reference (:31); x may be a torch tensor or an array.  In the default order the
    value is the reference's, bit for bit."""
    return float(objective_batch(np.asarray(params, dtype=np.float64)[None], W, x, params_y, params_p, params_r, order=order)[0])


def value_and_gradient_batch(params, W, X, params_y, params_p, params_r, x_index=None):
    """Objective and analytic gradient (:31-58, :60-102) of N evaluations in one native call (K3g), both in the reference's own
    operation order: err carries objective_batch's bits, every gradient component the reference's.  params f64[N,3+R]; X f32[M,1404]
    (M == N, or rows selected by x_index i32[N]) -> (err f64[N], grad f64[N,3+R]) (numpy) -- what scipy's gradient methods (the
    reference's L-BFGS-B alternative, :253-256) consume per step."""
    Wm, Xd, P, cp, xi = _stage(params, W, X, params_y, params_p, params_r, x_index)
    err, grad = ops.tucker_gradient(Wm, Xd, P, cp, x_index=xi)
    return err.cpu().numpy(), grad.cpu().numpy()


IMPL_LIBRARY, IMPL_NATIVE = "library", "native"


def compute_gradient_batch(params, W, X, params_y, params_p, params_r, impl=IMPL_LIBRARY):
    """Analytic gradient of the objective (:60-102) for N evaluations at once, on the device in f64.

    impl="native": the K3g kernels (value_and_gradient_batch), the reference's gradient bit for bit.  impl="library" (the default,
    unchanged): the regrouped form below -- angles within 1e-10 of scale, the identity part within f32 rounding.

    With c = u (x) f_y (x) f_p (x) f_r, r = x - c^T Wm (x_hat from the K3 kernel) and g = Wm r, the reference's four
    gradient einsums are dot products with g:  d/dw_a = -<dc/dw_a, g>, dc/dw_y = u (x) f_y' (x) f_p (x) f_r with
    f' = f32(-a b sin(b w + c)) (:80-95).  The identity-mode term is reproduced as the reference writes it (:96): its inner
    einsum also sums over i, so grad_u[i] = -sum_m S[i,m] r[m] v[m], v = (1 (x) f_y (x) f_p (x) f_r)^T Wm, S[i] = sum_jkl W[i,j,k,l].
    The three small GEMMs are library f64 matmuls (rocBLAS through torch).  -> f64[N,3+R] (numpy), R = W's identity rank."""
    if impl == IMPL_NATIVE:
        return value_and_gradient_batch(params, W, X, params_y, params_p, params_r)[1]
    if impl != IMPL_LIBRARY:
        raise ValueError(f"unknown impl {impl!r}; expected 'library' or 'native'")
    Wm, Xd, P, cp, _ = _stage(params, W, X, params_y, params_p, params_r)     # cp: [3 angles, 3 rows, (a,b,c,d)]
    R = Wm.shape[0] // 27
    _, xh = ops.tucker_objective(Wm, Xd, P, cp, return_xhat=True)
    r = Xd.double() - xh                                                      # residuals, :77
    a, b, c, d = cp[..., 0], cp[..., 1], cp[..., 2], cp[..., 3]               # each [3,3]
    w = P[:, :3, None]                                                        # [N,3,1]
    f = (a * torch.cos(b * w + c) + d).float().double()                       # .astype(np.float32), :66-73
    df = (-a * b * torch.sin(b * w + c)).float().double()                     # :80-81,85-86,90-91
    u = P[:, 3:]
    ones = torch.ones_like(u)

    def coef(uu, fy, fp, fr):
        return torch.einsum("ni,nj,nk,nl->nijkl", uu, fy, fp, fr).reshape(P.shape[0], -1)

    W64 = Wm.double()
    g = r @ W64.T                                                             # [N,27R]
    gy = -(coef(u, df[:, 0], f[:, 1], f[:, 2]) * g).sum(1)
    gp = -(coef(u, f[:, 0], df[:, 1], f[:, 2]) * g).sum(1)
    gr = -(coef(u, f[:, 0], f[:, 1], df[:, 2]) * g).sum(1)
    # 'ijklm,j,k,l->m' (:96) sums over i as well, and all its operands are f32, so numpy evaluates it in f32: v is an f32
    # quantity in the reference (this part of the gradient is therefore pinned to f32 rounding only, ~1e-7 relative)
    v = (coef(ones, f[:, 0], f[:, 1], f[:, 2]).float() @ Wm).double()
    S = W64.reshape(R, 27, -1).sum(1)                                         # [R,1404]
    gu = -((r * v) @ S.T)
    return torch.cat([gy[:, None], gp[:, None], gr[:, None], gu], dim=1).cpu().numpy()


def compute_gradient(params, W, x, params_y, params_p, params_r, impl=IMPL_LIBRARY):
    """Same signature as the reference (:60); x may be a torch tensor or an array.  -> f64[3+R].  impl as in compute_gradient_batch."""
    return compute_gradient_batch(np.asarray(params, dtype=np.float64)[None], W, x, params_y, params_p, params_r, impl=impl)[0]


def Test_batch(W, X, u_id_shape, optimized_params_y, optimized_params_p, optimized_params_r, return_info=False,
               order=ORDER_REFERENCE):
    """Rows of X f32[N,1404] -> degrees f64[N,3] by device-side lock-step Powell (one launch)."""
    R = _rank(u_id_shape)
    Wm = _wm(W)
    if Wm.shape[0] != 27 * R:
        raise ValueError(f"u_id_shape = {R} but W has {Wm.shape[0]} = 27 * {Wm.shape[0] // 27} coefficient rows")
    res = ops.tucker_powell(Wm, _x(X), _cos(optimized_params_y, optimized_params_p, optimized_params_r), order=order)
    deg = np.degrees(res["x"].cpu().numpy())[:, :3]                               # :196-199
    if return_info:
        return deg, {k: v.cpu().numpy() for k, v in res.items()}
    return deg


def Test(W, x, u_id_shape, optimized_params_y, optimized_params_p, optimized_params_r, u_id, f_y, f_p, f_r,
         order=ORDER_REFERENCE):
    """Same signature and return tuple as the reference (:162-163, :291): u_id is passed through.  Default order: the reference's
    (scipy's own trajectory and end point on its own objective bits; ~25 ms per face instead of the reference's 2-4 s)."""
    deg = Test_batch(W, x, u_id_shape, optimized_params_y, optimized_params_p, optimized_params_r, order=order)[0]
    return deg[0], deg[1], deg[2], u_id
