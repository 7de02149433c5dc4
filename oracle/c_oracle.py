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


# ---- K9: the operation orders of one encoder-training step, launch by launch (oracle.c, "K9") ---------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _operand(a, rows):
    """A 2-D f32 array whose rows may be strided (the columns are not) -> (array kept alive, ld in floats, rows i32 or None)."""
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 2 or (a.shape[1] > 1 and a.strides[1] != 4) or a.strides[0] % 4:
        a = np.ascontiguousarray(a, dtype=np.float32)
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    return a, a.strides[0] // 4, rows


def et_gemm(A, B, K, start=None, a_kc=True, b_kc=False, a_rows=None, b_rows=None, M=None, N=None, variant=0):
    """K9's GEMM order (oracle_et_gemm) -> C f32[M,N] = sum_k a(m,k) b(k,n).  A: [M,>=K] k-contiguous or (a_kc False) [>=K,M] k-outer;
    B: [N,>=K] k-contiguous (b_kc) or [>=K,N] k-outer.  a_rows / b_rows gather the storage row of their operand (M or N must then be
    given for a k-contiguous one).  start f32[N]: wave 0's start.  variant != 0: the wrong orders listed at the C section."""
    A, lda, a_rows = _operand(A, a_rows)
    B, ldb, b_rows = _operand(B, b_rows)
    M = M if M is not None else (A.shape[0] if a_kc else A.shape[1])
    N = N if N is not None else (B.shape[0] if b_kc else B.shape[1])
    for name, arr, kc, rows, n in (("A", A, a_kc, a_rows, M), ("B", B, b_kc, b_rows, N)):
        vec, red = (arr.shape[0], arr.shape[1]) if kc else (arr.shape[1], arr.shape[0])
        idx = rows if rows is not None else None
        if kc:
            ok = red >= K and (idx is None and vec >= n or idx is not None and len(idx) >= n and idx[:n].min() >= 0 and idx[:n].max() < vec)
        else:
            ok = vec >= n and (idx is None and red >= K or idx is not None and len(idx) >= K and idx[:K].min() >= 0 and idx[:K].max() < red)
        if not ok:
            raise ValueError(f"et_gemm: operand {name} {arr.shape} does not cover {n} x {K}")
    if start is not None:
        start = _f32(start)
        if start.shape != (N,):
            raise ValueError("et_gemm: start: expected [N]")
    out = np.empty((M, N), np.float32)
    lib().oracle_et_gemm(_p(A), C.c_int64(lda), C.c_int(int(a_kc)), _p(a_rows) if a_rows is not None else None, _p(B), C.c_int64(ldb),
                         C.c_int(int(b_kc)), _p(b_rows) if b_rows is not None else None, _p(start) if start is not None else None,
                         C.c_int(M), C.c_int(N), C.c_int(K), _p(out), C.c_int64(N), C.c_int(int(variant)))
    return out


def et_bias_grad(delta, variant=0):
    """delta f32[B,out] -> db f32[out] in K9's sixteen runs of ceil(B/16) rows."""
    delta, ldd, _ = _operand(delta, None)
    out = np.empty(delta.shape[1], np.float32)
    lib().oracle_et_bias_grad(_p(delta), C.c_int64(ldd), C.c_int(delta.shape[0]), C.c_int(delta.shape[1]), _p(out), C.c_int(int(variant)))
    return out


def et_loss(pred, target, variant=0):
    """pred f32[B,9] (rows may be strided), target f32[B,9] -> dict(q [B], slots [256] after the tree, loss f32 scalar, delta6 [B,9])."""
    pred, ldp, _ = _operand(pred, None)
    target = _f32(target)
    B = pred.shape[0]
    if pred.shape[1] != 9 or target.shape != (B, 9) or not 1 <= B <= 256:
        raise ValueError("et_loss: expected pred and target [B,9] with B in 1..256")
    q, slots, loss, d6 = np.empty(B, np.float32), np.empty(256, np.float32), np.empty(1, np.float32), np.empty((B, 9), np.float32)
    lib().oracle_et_loss(_p(pred), C.c_int64(ldp), _p(target), C.c_int(B), _p(q), _p(slots), _p(loss), _p(d6), C.c_int(int(variant)))
    return {"q": q, "slots": slots, "loss": loss[0], "delta6": d6}


def et_n_partials(F):
    return int(lib().oracle_et_n_partials(C.c_int(F)))


def et_norm(F, G=None, partials=None, max_norm=20.0, variant=0):
    """K9's f64 norm of the flat accumulator G f32[params], or from given tile partials f64[n_partials] ->
    dict(partials, chains [512], tree [512] after the tree, norm f64, c f64)."""
    n = et_n_partials(F)
    if (G is None) == (partials is None):
        raise ValueError("et_norm: give G or partials")
    if G is not None:
        G = _f32(G).ravel()
        fan_in, total = F, 0
        for w in (1024, 512, 256, 128, 64, 9):
            total, fan_in = total + w * fan_in + w, w
        if G.shape != (total,):
            raise ValueError(f"et_norm: G: expected {total} elements")
    else:
        partials = np.ascontiguousarray(partials, dtype=np.float64)
        if partials.shape != (n,):
            raise ValueError(f"et_norm: partials: expected [{n}]")
    out, chains, tree = np.empty(n), np.empty(512), np.empty(512)
    norm, c = C.c_double(), C.c_double()
    lib().oracle_et_norm(_p(G) if G is not None else None, C.c_int(F), _p(partials) if partials is not None else None, C.c_double(max_norm),
                         _p(out), _p(chains), _p(tree), C.byref(norm), C.byref(c), C.c_int(int(variant)))
    return {"partials": out, "chains": chains, "tree": tree, "norm": norm.value, "c": c.value}


def et_update(p, g, c, lr, wd, variant=0):
    """-> (p_new, g_new) f32 of K9's update; c, lr, wd are rounded to f32 as the entry point's arguments are."""
    p, g = _f32(p).copy(), _f32(g).copy()
    if p.shape != g.shape:
        raise ValueError("et_update: p and g differ in shape")
    lib().oracle_et_update(_p(p), _p(g), C.c_int64(p.size), C.c_float(c), C.c_float(lr), C.c_float(wd), C.c_int(int(variant)))
    return p, g


def et_act_grad(s, a, tanh_layer):
    """s * act'(a) element by element (ReLU, or the tanh layer's fmaf(-a, a, 1))."""
    s, a = _f32(s), _f32(a)
    if s.shape != a.shape:
        raise ValueError("et_act_grad: s and a differ in shape")
    out = np.empty_like(s)
    lib().oracle_et_act_grad(_p(s), _p(a), C.c_int64(s.size), C.c_int(int(tanh_layer)), _p(out))
    return out


def et_tanhf(z):
    """This machine's libm tanhf (the host form's layer 4)."""
    z = _f32(z)
    out = np.empty_like(z)
    lib().oracle_et_tanhf(_p(z), C.c_int64(z.size), _p(out))
    return out
