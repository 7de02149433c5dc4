"""ctypes loader for the plain-C oracle (oracle/csrc/oracle.c).  TEST INFRASTRUCTURE."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.path.join(_HERE, "_build", "liboracle.so")
_lib = None


def build() -> str:
    subprocess.run(["make", "-s", "-C", _HERE], check=True)
    return _PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_PATH):
            build()
        _lib = C.CDLL(_PATH)
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def normalize_ipd(raw: np.ndarray, normalize: bool = True) -> np.ndarray:
    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, 1404)
    out = np.empty_like(raw)
    lib().oracle_normalize_ipd(_p(raw), C.c_int64(raw.shape[0]), C.c_int(int(normalize)), _p(out))
    return out


def ipd(raw: np.ndarray) -> np.ndarray:
    """f64[B]: the divisor of normalize_ipd per face."""
    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1, 1404)
    out = np.empty(raw.shape[0], np.float64)
    lib().oracle_ipd(_p(raw), C.c_int64(raw.shape[0]), _p(out))
    return out


def encoder_heads(x: np.ndarray, params, order: int = 2, want_latent=False, want_pre_tanh=False):
    """params: oracle.encoder_heads.Params.  order 0 = k ascending, 1 = one MFMA-order chain per output, 2 (default) = the f32
    HIP kernel's order: MFMA-order chains with layers 0 to 3 summed in blocks of 128 k (encoder_heads.hip fold_block)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, F = x.shape
    ew = [np.ascontiguousarray(w) for w, _ in params.enc]
    eb = [np.ascontiguousarray(b) for _, b in params.enc]
    hw = [np.ascontiguousarray(w) for n in ("yaw", "pitch", "roll") for w, _ in params.heads[n]]
    hb = [np.ascontiguousarray(b) for n in ("yaw", "pitch", "roll") for _, b in params.heads[n]]
    arr = lambda xs: (C.c_void_p * len(xs))(*[a.ctypes.data for a in xs])
    out = np.empty((B, 3), np.float32)
    lat = np.empty((B, 9), np.float32) if want_latent else None
    pre = np.empty((B, 64), np.float32) if want_pre_tanh else None
    lib().oracle_encoder_heads_f32(_p(x), C.c_int64(B), C.c_int(F), arr(ew), arr(eb), arr(hw), arr(hb), C.c_int(order),
                                   _p(out), _p(lat) if lat is not None else None, _p(pre) if pre is not None else None)
    res = [out]
    if want_latent:
        res.append(lat)
    if want_pre_tanh:
        res.append(pre)
    return res[0] if len(res) == 1 else tuple(res)


def tucker_fvec(params, cosp):
    """f64[N,3,3] holding the f32 f-vectors (f_y, f_p, f_r) of every parameter row, from oracle.tucker.f_vectors (numpy's cos)."""
    from . import tucker as TK
    params = np.asarray(params, dtype=np.float64)
    Py, Pp, Pr = np.asarray(cosp, dtype=np.float64).reshape(3, 3, 4)
    with np.errstate(all="ignore"):
        return np.array([np.stack(TK.f_vectors(p, Py, Pp, Pr)) for p in params], dtype=np.float64).reshape(len(params), 3, 3)


def tucker_objective_fast(Wm, x, params, cosp, x_index=None, ldx=None, want_xhat=False, variant=0, fvec=None):
    """The matrix-core ("fast") order of the TD objective for any identity rank R (oracle_tucker_objective_fast): Wm f32[27R,1404],
    params f64[N,3+R], x f32[M,1404] -- or, with ldx, a buffer of rows of that stride -- evaluation n on row x_index[n] (row n without).
    fvec f64[N,3,3]: tucker_fvec(params, cosp) unless given.  variant != 0: the deliberately wrong orders listed at the C function."""
    Wm = np.ascontiguousarray(Wm, dtype=np.float32).reshape(-1, 1404)
    R, rem = divmod(Wm.shape[0], 27)
    params = np.ascontiguousarray(params, dtype=np.float64)
    N = params.shape[0]
    if rem or not 1 <= R <= 16 or params.shape != (N, 3 + R):
        raise ValueError(f"Wm {Wm.shape} / params {params.shape}: expected [27R,1404] and [N,3+R] with R in 1..16")
    x = np.ascontiguousarray(x, dtype=np.float32)
    if ldx is None:
        x = x.reshape(-1, 1404)
        ldx, rows = 1404, x.shape[0]
    else:
        rows = x.size // ldx
        if ldx < 1404 or x.size != rows * ldx:
            raise ValueError("x: expected whole rows of stride ldx >= 1404")
    if x_index is not None:
        x_index = np.ascontiguousarray(x_index, dtype=np.int32)
        if x_index.shape != (N,) or (N and (x_index.min() < 0 or x_index.max() >= rows)):
            raise IndexError("x_index: expected [N] of row numbers")
    elif rows < N:
        raise ValueError(f"x has {rows} rows but params has {N}")
    fvec = np.ascontiguousarray(tucker_fvec(params, cosp) if fvec is None else fvec, dtype=np.float64)
    if fvec.shape != (N, 3, 3):
        raise ValueError("fvec: expected [N,3,3]")
    err = np.empty(N)
    xh = np.empty((N, 1404)) if want_xhat else None
    lib().oracle_tucker_objective_fast(_p(Wm), C.c_int(R), _p(x), C.c_int64(ldx), _p(x_index) if x_index is not None else None,
                                       _p(params), _p(fvec), C.c_int64(N), _p(err), _p(xh) if want_xhat else None, C.c_int(int(variant)))
    return (err, xh) if want_xhat else err


def tucker_objective(Wm, x, params, cosp, want_xhat=False, device_order=False, reference_order=False):
    """reference_order: np.einsum's own (i,j,k,l)-outer sum of separately rounded products and numpy's pairwise np.sum --
    bit-identical to the reference's objective (FX4); device_order: the fast kernel's reduction tree."""
    Wm = np.ascontiguousarray(Wm, dtype=np.float32).reshape(135, 1404)
    x = np.ascontiguousarray(x, dtype=np.float32)
    params = np.ascontiguousarray(params, dtype=np.float64)
    cosp = np.ascontiguousarray(cosp, dtype=np.float64)
    N = params.shape[0]
    err = np.empty(N)
    xh = np.empty((N, 1404)) if want_xhat else None
    if reference_order:
        lib().oracle_tucker_objective_reforder(_p(Wm), _p(x), _p(params), _p(cosp), C.c_int64(N), _p(err),
                                               _p(xh) if want_xhat else None)
        return (err, xh) if want_xhat else err
    lib().oracle_tucker_objective(_p(Wm), _p(x), _p(params), _p(cosp), C.c_int64(N), _p(err), _p(xh) if want_xhat else None,
                                  C.c_int(int(device_order)))
    return (err, xh) if want_xhat else err


# ---- K7: the summation orders of the Tucker decomposition's four primitives (oracle.c, "K7") ----------------------------------------
def _tensor_in(a):
    """-> (contiguous array, f64 flag): f64 stays f64 (a projection kept unrounded), anything else is taken as f32."""
    a = np.asarray(a)
    a = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
    return a, int(a.dtype == np.float64)


def mode_gram_plan(I: int, K: int):
    """K7a's slice rule -> (tile pairs, columns per slice, slices)."""
    v = [C.c_int64() for _ in range(3)]
    lib().oracle_mode_gram_plan(C.c_int64(I), C.c_int64(K), *[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def mode_gram(A, variant=0):
    """K7a's order: A f32 or f64 [I,K] -> G f64[I,I].  variant != 0: the wrong orders listed at oracle_mode_gram."""
    A, f64 = _tensor_in(A)
    I, K = A.shape
    G = np.empty((I, I))
    lib().oracle_mode_gram(_p(A), C.c_int(f64), C.c_int64(I), C.c_int64(K), _p(G), C.c_int(int(variant)))
    return G


def pose_grams(X, which=(True, True, True), variant=0):
    """K7b's order: X f32 or f64 [I,ny,np,nr,M] -> (Gy, Gp, Gr), None where `which` is false; 32-column slabs for f32 input, 16 for
    f64.  variant != 0: the wrong orders listed at oracle_pose_grams."""
    X, f64 = _tensor_in(X)
    I, ny, np_, nr, M = X.shape
    G = [np.empty((n, n)) if w else None for n, w in zip((ny, np_, nr), which)]
    lib().oracle_pose_grams(_p(X), C.c_int(f64), C.c_int64(I), C.c_int(ny), C.c_int(np_), C.c_int(nr), C.c_int64(M),
                            *[_p(g) if g is not None else None for g in G], C.c_int(int(variant)))
    return tuple(G)


def project_identity(A, U, out_dtype=np.float32, variant=0):
    """K7c's order: A f32[I,K], U f64[I,R] -> U^T A as f32 (one cast) or f64 [R,K].  variant != 0: see oracle_project_identity."""
    A = np.ascontiguousarray(A, dtype=np.float32)
    U = np.ascontiguousarray(U, dtype=np.float64)
    I, K = A.shape
    if U.ndim != 2 or U.shape[0] != I or not 1 <= U.shape[1] <= 16:
        raise ValueError(f"U {U.shape}: expected [{I},R] with R in 1..16")
    out = np.empty((U.shape[1], K), out_dtype)
    lib().oracle_project_identity(_p(A), C.c_int64(I), C.c_int64(K), _p(U), C.c_int(U.shape[1]), _p(out),
                                  C.c_int(int(out.dtype == np.float64)), C.c_int(int(variant)))
    return out


def project_pose(X, Uy=None, Up=None, Ur=None, out_dtype=np.float32, variant=0):
    """K7d's order: X f32 or f64 [I,ny,np,nr,M] contracted with every factor given (f64[n,r], r <= 3; None keeps the mode) -> f32 (one
    cast) or f64.  variant != 0: see oracle_project_pose."""
    X, f64 = _tensor_in(X)
    shape = list(X.shape)
    Us, args = [], []
    for k, U in enumerate((Uy, Up, Ur)):
        if U is not None:
            U = np.ascontiguousarray(U, dtype=np.float64)
            if U.ndim != 2 or U.shape[0] != X.shape[1 + k] or not 1 <= U.shape[1] <= 3:
                raise ValueError(f"factor {k} {U.shape}: expected [{X.shape[1 + k]},r] with r in 1..3")
            shape[1 + k] = U.shape[1]
        Us.append(U)
        args += [_p(U) if U is not None else None, C.c_int(U.shape[1] if U is not None else 0)]
    out = np.empty(shape, out_dtype)
    lib().oracle_project_pose(_p(X), C.c_int(f64), C.c_int64(X.shape[0]), C.c_int(X.shape[1]), C.c_int(X.shape[2]), C.c_int(X.shape[3]),
                              C.c_int64(X.shape[4]), *args, _p(out), C.c_int(int(out.dtype == np.float64)), C.c_int(int(variant)))
    return out
