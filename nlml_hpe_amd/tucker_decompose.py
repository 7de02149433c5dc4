"""Tucker decomposition of the rotation training tensor (TD_main.py:181), on the device.

The reference's line is ``core, factors = tucker(tensor, rank=[5, 3, 3, 3, 1404])`` (tensorly): HOSVD initialisation followed by
HOOI sweeps (De Lathauwer, De Moor, Vandewalle 2000).  This module restates that published algorithm over four device primitives
(csrc/tucker_decompose.hip, K7a..K7d: ops.mode_gram, ops.pose_grams, ops.project_identity, ops.project_pose); nothing of tensorly is
used.  Every unfolding's leading left singular vectors are taken as the leading eigenvectors of its f64 Gram matrix.

Why the feature mode never appears: every shipped configuration has R_features = I_features = 1404, so the feature factor is square
and orthogonal, and

    W = core x_5 U_feat = X x_1 U_id^T x_2 U_yaw^T x_3 U_pitch^T x_4 U_roll^T

needs no 1404 x 1404 eigenproblem.  ``tucker`` therefore returns W itself -- the tensor K3, K3g and the Powell kernel consume --
and refuses any rank[4] other than the feature extent.  ``thin_core`` splits W into a (core, U_feat) pair for
artefacts.core_to_W / nlml_mode5_product where one is wanted.

Sign convention: each factor column is flipped so that its entry of largest magnitude (the lowest index on a tie) is positive, the
convention all 14 columns of the shipped Factor_Matrices.npz follow.

The error ``tucker`` reports by default, sqrt(|X|^2 - |W|^2) / |X|, equals the reconstruction error only in exact arithmetic with
exactly orthonormal factors, and cancels where the fit is good.  ``reconstruction_error`` measures |X - X_hat| / |X| itself, as the
reference does (TD_main.py:221-224), in one pass over X that never holds X_hat (K11, csrc/tucker_residual.hip); ``tucker_to_tensor``
is the expansion alone, ``tucker(error="residual")`` uses the measured error per sweep, and ``singular_values`` gives the spectrum of
the four unfoldings the ranks are chosen by (TD_main.py:186-209).

``decompose_to_npz`` writes Factor_Matrices.npz only.  ``train_to_npz`` goes on to TD_Trainer's cosine fit of the pose factors (K8)
and writes Trained_data.npz as well: the two files the TD path loads.
"""
from __future__ import annotations

import os

import numpy as np

IDENTITY_RANK_MAX = 16     # NLML_TUCKER_RANK_MAX: the TD kernels' (and K7c's) limit
POSE_RANK_MAX = 3          # NLML_POSE_RANK_MAX: W is [R,3,3,3,M] for every consumer


def fix_signs(U):
    """Flip each column so that its entry of largest magnitude (lowest index on a tie) is positive.  U: numpy [n,R]."""
    U = np.array(U, dtype=np.float64, copy=True)
    for r in range(U.shape[1]):
        if U[np.argmax(np.abs(U[:, r])), r] < 0:
            U[:, r] = -U[:, r]
    return U


def _leading_numpy(G, R):
    w, V = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    return fix_signs(V[:, ::-1][:, :R])


class _NumpyBackend:
    """The four primitives in numpy f64 on the host: the CPU tests' path and the timing baseline."""

    def __init__(self, tensor):
        if hasattr(tensor, "detach"):
            tensor = tensor.detach().cpu().numpy()
        self.source = tensor
        self.X = np.ascontiguousarray(tensor, dtype=np.float64)

    def mode_gram(self, T):
        A = T.reshape(T.shape[0], -1)
        return A @ A.T

    def pose_gram(self, T, mode):
        A = np.moveaxis(T, mode, 0).reshape(T.shape[mode], -1)
        return A @ A.T

    def pose_grams(self, T):
        return [self.pose_gram(T, mode) for mode in (1, 2, 3)]

    def project_identity(self, T, U):
        return np.tensordot(U.T, T, axes=(1, 0))

    def project_pose(self, T, Uy, Up, Ur):
        for mode, U in ((1, Uy), (2, Up), (3, Ur)):
            if U is not None:
                T = np.moveaxis(np.tensordot(U.T, T, axes=(1, mode)), 0, mode)
        return T

    def leading(self, G, R):
        return _leading_numpy(G, R)

    def trace(self, G):
        return float(np.trace(G))

    def sumsq(self, T):
        return float(np.sum(np.square(T, dtype=np.float64)))

    def out_tensor(self, T):
        return np.ascontiguousarray(T, dtype=np.float32)

    def out_factor(self, U):
        return U

    def residual_sums(self, W32, U):
        return _residual_host(np.ascontiguousarray(self.source, dtype=np.float32), W32, U)[0]


class _DeviceBackend:
    """The four primitives as HIP kernels; factors stay on the device as f64, and so does every projected tensor between two steps
    (a factor computed from an f32-rounded projection would sit 2^-24 from the exact one, far outside the f64 Grams' own error);
    only W is rounded to f32, once.  The eigen-solve of a small f64 Gram is plumbing: torch.linalg.eigh on the device, numpy on
    the host where that solver is unavailable."""

    def __init__(self, tensor):
        import torch

        from . import ops
        self.torch, self.ops = torch, ops
        if not torch.is_tensor(tensor):
            tensor = torch.as_tensor(np.ascontiguousarray(tensor, dtype=np.float32))
        if not tensor.is_cuda:
            tensor = tensor.to("cuda")
        if tensor.dtype != torch.float32:
            raise TypeError(f"tensor: expected float32, got {tensor.dtype}")
        self.X = tensor.contiguous()

    def mode_gram(self, T):
        return self.ops.mode_gram(T.reshape(T.shape[0], -1))

    def pose_gram(self, T, mode):
        return self.ops.pose_grams(T, which=[m == mode for m in (1, 2, 3)])[mode - 1]

    def pose_grams(self, T):
        return self.ops.pose_grams(T)             # one pass over the tensor for all three

    def project_identity(self, T, U):
        return self.ops.project_identity(T.reshape(T.shape[0], -1), U, out_dtype=self.torch.float64).reshape(
            (U.shape[1],) + tuple(T.shape[1:]))

    def project_pose(self, T, Uy, Up, Ur):
        return self.ops.project_pose(T, Uy, Up, Ur, out_dtype=self.torch.float64)

    def leading(self, G, R):
        torch = self.torch
        try:
            w, V = torch.linalg.eigh(G)
            V = V.flip(1)[:, :R]
            rows = V.abs().argmax(dim=0)           # the first index of the maximum, as numpy's argmax
            sign = torch.where(V[rows, torch.arange(R, device=V.device)] < 0, -1.0, 1.0).to(V.dtype)
            return (V * sign).contiguous()
        except RuntimeError:
            return torch.from_numpy(_leading_numpy(G.cpu().numpy(), R)).to(G.device)

    def trace(self, G):
        return float(self.torch.trace(G))

    def sumsq(self, T):
        return float(T.double().square().sum())

    def out_tensor(self, T):
        return T.to(self.torch.float32)

    def out_factor(self, U):
        return U

    def residual_sums(self, W32, U):
        return self.ops.tucker_residual(self.X, W32, *U)[0].cpu().numpy()


def _check_rank(shape, rank):
    if len(shape) != 5:
        raise ValueError(f"tensor: expected [I, ny, np, nr, M], got {tuple(shape)}")
    rank = [int(r) for r in rank]
    if len(rank) != 5:
        raise ValueError(f"rank: expected [R_identity, R_yaw, R_pitch, R_roll, R_features], got {rank}")
    if rank[4] != shape[4]:
        raise ValueError(
            f"rank[4] = {rank[4]} but the tensor has {shape[4]} features: only R_features = I_features is supported.  With a square "
            "(orthogonal) feature factor W = core x_5 U_feat equals the tensor projected on the four other factors, so no feature "
            "eigenproblem is solved; a smaller R_features would need that 1404 x 1404 problem and is out of scope")
    if not 1 <= rank[0] <= min(IDENTITY_RANK_MAX, shape[0]):
        raise ValueError(f"rank[0] = {rank[0]}: the identity rank must be in 1..{min(IDENTITY_RANK_MAX, shape[0])} "
                         f"({IDENTITY_RANK_MAX} is the limit of the TD kernels, {shape[0]} the number of identities)")
    for k, name in ((1, "yaw"), (2, "pitch"), (3, "roll")):
        if not 1 <= rank[k] <= min(POSE_RANK_MAX, shape[k]):
            raise ValueError(f"rank[{k}] = {rank[k]}: the {name} rank must be in 1..{min(POSE_RANK_MAX, shape[k])}")
    return rank


def tucker(tensor, rank, n_iter_max=100, tol=1e-4, backend="device", return_errors=False, error="norms"):
    """HOSVD + HOOI of tensor f32[I,ny,np,nr,M] -> (W f32[R_id,r_yaw,r_pitch,r_roll,M], [U_id, U_yaw, U_pitch, U_roll]).

    rank          [R_identity, R_yaw, R_pitch, R_roll, R_features]; R_features must equal M (see the module docstring),
                  R_identity <= 16, the pose ranks <= 3
    n_iter_max    HOOI sweeps at most (0: the HOSVD factors and their projection)
    tol           stop when the relative reconstruction error sqrt(|X|^2 - |W|^2) / |X| changes by less than tol between two sweeps
    backend       "device": HIP kernels, a GPU tensor in, GPU tensors out (factors f64);  "numpy": the same driver over numpy f64
                  versions of the four primitives (host arrays in and out)
    return_errors also return the list of the sweeps' relative reconstruction errors
    error         "norms": the error above, from |X|^2 and |W|^2;  "residual": |X - X_hat| / |X| measured by K11 on the sweep's W
                  rounded to f32 (the W that is returned) and its f64 factors -- one more pass over X per sweep; the stop rule uses it
    """
    if backend not in ("device", "numpy"):
        raise ValueError(f"backend: expected 'device' or 'numpy', got {backend!r}")
    if error not in ("norms", "residual"):
        raise ValueError(f"error: expected 'norms' or 'residual', got {error!r}")
    rank = _check_rank(tuple(tensor.shape), rank)
    be = _DeviceBackend(tensor) if backend == "device" else _NumpyBackend(tensor)
    X = be.X

    # HOSVD: the leading eigenvectors of each mode's Gram of the full tensor
    G_id = be.mode_gram(X)
    norm2 = be.trace(G_id)
    U = [be.leading(G_id, rank[0])] + [be.leading(G, rank[mode]) for mode, G in zip((1, 2, 3), be.pose_grams(X))]

    def project(U):
        Z = be.project_identity(X, U[0])
        return Z, be.project_pose(Z, U[1], U[2], U[3])

    errors = []
    W = None
    for _ in range(int(n_iter_max)):
        # mode 1: the pose modes contracted first (27 M columns), then its Gram
        U[0] = be.leading(be.mode_gram(be.project_pose(X, U[1], U[2], U[3])), rank[0])
        Z = be.project_identity(X, U[0])
        for mode in (1, 2, 3):
            others = [None if m == mode else U[m] for m in (1, 2, 3)]
            U[mode] = be.leading(be.pose_gram(be.project_pose(Z, *others), mode), rank[mode])
        W = be.project_pose(Z, U[1], U[2], U[3])
        if error == "residual":
            ss = be.residual_sums(be.out_tensor(W), U)
            errors.append(float(np.sqrt(ss[0] / ss[1])) if ss[1] > 0 else 0.0)
        else:
            errors.append(float(np.sqrt(max(norm2 - be.sumsq(W), 0.0) / norm2)) if norm2 > 0 else 0.0)
        if len(errors) >= 2 and abs(errors[-2] - errors[-1]) < tol:
            break
    if W is None:
        W = project(U)[1]
    out = (be.out_tensor(W), [be.out_factor(u) for u in U])
    return out + (errors,) if return_errors else out


# ---- K11: the true reconstruction error, the expansion, the spectrum ---------------------------------------------------------------
def _to_numpy(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _host_model(W, factors):
    """-> (W f32[R,ry,rp,rr,M], [U_id, U_yaw, U_pitch, U_roll] f64), contiguous host arrays; upcasting an f32 factor is exact."""
    W = np.ascontiguousarray(_to_numpy(W), dtype=np.float32)
    U = [np.ascontiguousarray(_to_numpy(u), dtype=np.float64) for u in factors]
    if W.ndim != 5 or len(U) != 4 or any(u.ndim != 2 or u.shape[1] != W.shape[k] for k, u in enumerate(U)):
        raise ValueError(f"W {W.shape} and the four factors {[u.shape for u in U]} do not form a Tucker model [R,ry,rp,rr,M], [n,r]")
    return W, U


def _residual_host(X, W, factors, want_res_id=False, want_xhat=False):
    """nlml_tucker_residual_host (no GPU involved): X f32[I,ny,np,nr,M] or None -> (sums f64[2], res_id f64[I], xhat f32), None where
    not asked for."""
    from . import _lib

    W, U = _host_model(W, factors)
    shape = tuple(u.shape[0] for u in U) + (W.shape[4],)
    if X is not None:
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.shape != shape:
            raise ValueError(f"tensor {X.shape}: the factors' rows and W's columns give {shape}")
    else:
        want_xhat, want_res_id = True, False
    L = _lib.lib()
    I, ny, np_, nr, M = shape
    sums = np.zeros(2, np.float64) if X is not None else None
    res_id = np.zeros(I, np.float64) if want_res_id else None
    xhat = np.zeros(shape, np.float32) if want_xhat else None
    nbytes = L.nlml_tucker_residual_workspace_bytes(I, ny, np_, nr, M) if X is not None else 0
    ws = np.zeros(max(1, nbytes // 8), np.float64)
    ptr = lambda a: a.ctypes.data if a is not None else None
    _lib.check(L.nlml_tucker_residual_host(ptr(X), W.ctypes.data, *[u.ctypes.data for u in U], I, ny, np_, nr, M, *W.shape[:4], ptr(sums),
                                           ptr(res_id), ptr(xhat), ws.ctypes.data, ws.nbytes), "nlml_tucker_residual_host")
    return sums, res_id, xhat


def _device_model(W, factors, device=None):
    import torch

    def put(a, dtype):
        t = a.detach() if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(_to_numpy(a)))
        return t.to(device=device or "cuda", dtype=dtype)
    if len(factors) != 4:
        raise ValueError(f"factors: expected [U_id, U_yaw, U_pitch, U_roll], got {len(factors)} entries")
    return put(W, torch.float32), [put(u, torch.float64) for u in factors]


def _check_backend(backend):
    if backend not in ("device", "numpy"):
        raise ValueError(f"backend: expected 'device' or 'numpy', got {backend!r}")


def reconstruction_error(tensor, W, factors, backend="device", per_identity=False):
    """The relative reconstruction error |X - X_hat| / |X| of the Tucker model (W, factors) against tensor f32[I,ny,np,nr,M], measured
    directly (TD_main.py:221-224): X_hat = W x_1 U_id x_2 U_yaw x_3 U_pitch x_4 U_roll is formed element by element in f64 and
    compared in the same pass (K11); nothing of the tensor's size is allocated.  -> sqrt(ss_res / ss_x) as a float; per_identity=True:
    (that, res_id f64[I]) with each identity's sum of squared residuals, which shows the identities the model fits badly.

    W          f32[R,ry,rp,rr,M] (what ``tucker`` returns and Trained_data.npz holds)
    factors    [U_id, U_yaw, U_pitch, U_roll]: the f64 device tensors ``tucker`` returns, or the f32 arrays of Factor_Matrices.npz
               (upcasting them is exact, so the error is that of the artefacts as written)
    backend    "device": one GPU pass;  "numpy": the host form of the same operation order (no GPU involved), the same bits"""
    _check_backend(backend)
    if backend == "numpy":
        sums, res_id, _ = _residual_host(_to_numpy(tensor), W, factors, want_res_id=per_identity)
    else:
        from . import ops
        X = _DeviceBackend(tensor).X
        Wd, U = _device_model(W, factors, X.device)
        sums, res_id, _ = ops.tucker_residual(X, Wd, *U, want_res_id=per_identity)
        sums, res_id = sums.cpu().numpy(), res_id.cpu().numpy() if per_identity else None
    err = float(np.sqrt(sums[0] / sums[1])) if sums[1] > 0 else 0.0
    return (err, res_id) if per_identity else err


def tucker_to_tensor(W, factors, backend="device"):
    """tensorly's tucker_to_tensor for this module's models: W x_1 U_id x_2 U_yaw x_3 U_pitch x_4 U_roll -> f32[I,ny,np,nr,M] (f64 sums,
    one rounding; K11's expand-only form).  A one-row U_id gives a single identity's landmarks at every pose.  backend "device": a GPU
    tensor;  "numpy": a host array from the host form, the same bits."""
    _check_backend(backend)
    if backend == "numpy":
        return _residual_host(None, W, factors)[2]
    from . import ops
    Wd, U = _device_model(W, factors)
    return ops.tucker_to_tensor(Wd, *U)


def singular_values(tensor, backend="device"):
    """The singular values of the four unfoldings (identity, yaw, pitch, roll) of tensor f32[I,ny,np,nr,M] and their energies, the
    numbers TD_main.py:186-209 prints and the ranks of config_TD_main.yaml are chosen by.  -> (values, energies): two lists of four
    descending f64 arrays, energies = s / s.sum() * 100 as the reference computes them.

    No SVD of an unfolding is taken: the values are the square roots of the eigenvalues of the f64 Grams K7a and K7b give (clamped
    at 0).  A Gram squares the condition number, so values below roughly sqrt(2^-53) * s_max (1e-8 of the largest) are rounding
    noise, not spectrum; the energies of such values are below 1e-6 % and print as 0.00 %.  The identity Gram limits I to 4096."""
    _check_backend(backend)
    be = _DeviceBackend(tensor) if backend == "device" else _NumpyBackend(tensor)
    if len(be.X.shape) != 5:
        raise ValueError(f"tensor: expected [I, ny, np, nr, M], got {tuple(be.X.shape)}")
    values = []
    for G in [be.mode_gram(be.X)] + list(be.pose_grams(be.X)):
        w = np.linalg.eigvalsh(np.asarray(_to_numpy(G), dtype=np.float64))[::-1]
        values.append(np.sqrt(np.maximum(w, 0.0)))
    return values, [s / s.sum() * 100 if s.sum() > 0 else np.zeros_like(s) for s in values]


def thin_core(W):
    """W f32[R,a,b,c,M] -> (core f32[R,a,b,c,Q], U_feat f32[M,Q]), Q = min(R a b c, M): the thin SVD of W's mode-5 unfolding in torch
    f64, so that W = core x_5 U_feat (artefacts.core_to_W, nlml_mode5_product) with an orthonormal U_feat.  For the shipped ranks
    Q = 135."""
    import torch

    Wt = W if torch.is_tensor(W) else torch.as_tensor(np.asarray(W))
    lead, M = tuple(Wt.shape[:-1]), Wt.shape[-1]
    A, S, Bh = torch.linalg.svd(Wt.reshape(-1, M).double(), full_matrices=False)   # Wm = A diag(S) Bh
    core = (A * S).to(torch.float32).reshape(lead + (S.shape[0],))
    return core.contiguous(), Bh.T.to(torch.float32).contiguous()


def decompose_to_npz(tensor, config, out_dir, backend="device", **kwargs):
    """Decompose with the ranks of config["tensor_decom_ranks"] (configs/config_TD_main.yaml) and write <out_dir>/Factor_Matrices.npz
    with the reference's keys and dtypes (TD_main.py:261): f32 U_yaw, U_pitch, U_roll, U_id.  Returns (W, factors) as ``tucker``.
    Trained_data.npz is not written: it also holds TD_Trainer's cosine fit; train_to_npz runs that and writes both files.
    return_errors=True: (W, factors, the sweeps' errors)."""
    r = config["tensor_decom_ranks"]
    rank = [r["R_identity"], r["R_yaw"], r["R_pitch"], r["R_roll"], r["R_features"]]
    return_errors = kwargs.pop("return_errors", False)
    W, factors, errors = tucker(tensor, rank, backend=backend, return_errors=True, **kwargs)
    host = [np.asarray(u.detach().cpu().numpy() if hasattr(u, "detach") else u, dtype=np.float32) for u in factors]
    os.makedirs(out_dir, exist_ok=True)
    np.savez(os.path.join(out_dir, "Factor_Matrices.npz"), U_yaw=host[1], U_pitch=host[2], U_roll=host[3], U_id=host[0])
    return (W, factors, errors) if return_errors else (W, factors)


def _bins(spec):
    """The angle bins of a configuration entry {min_bin, max_bin, interval} as TD_main.py builds them: np.arange(min, max, interval)."""
    return np.arange(spec["min_bin"], spec["max_bin"], spec["interval"])


def train_to_npz(tensor, config, out_dir, backend="device", **kwargs):
    """The training chain behind the tensor (TD_main.py:181-262): decompose with the ranks of config["tensor_decom_ranks"], fit the
    three pose factors' cosines over the bins of config["yaw_bins"], ["pitch_bins"], ["roll_bins"] (TD_Trainer.Train, K8) and write
    BOTH artefacts to out_dir with the reference's keys and dtypes:

      Factor_Matrices.npz   f32 U_yaw, U_pitch, U_roll, U_id                      (as decompose_to_npz)
      Trained_data.npz      f64 optimized_yaw, optimized_pitch, optimized_roll [R_pose,4]; f32 W [R,ry,rp,rr,M]; f32 CoreTensor

    The fit runs on the f32 factors that are written -- the columns every consumer of the files sees.  CoreTensor is W itself:
    with rank[4] equal to the feature extent the feature factor is square and orthogonal, any orthogonal U_feat (and the matching
    core) reproduces the same W, and U_feat = I is the choice that needs no 1404 x 1404 eigenproblem (``thin_core`` gives a thin
    pair where one is wanted).  No consumer of this package reads CoreTensor for anything but its presence.

    backend "device": K7 and K8 on the GPU;  "numpy": the numpy decomposition and the host form of the fit (no GPU involved).
    Returns (W, factors, (optimized_yaw, optimized_pitch, optimized_roll)); return_errors=True: and the sweeps' errors."""
    from . import TD_Trainer

    bins = [_bins(config[k]) for k in ("yaw_bins", "pitch_bins", "roll_bins")]
    return_errors = kwargs.pop("return_errors", False)
    W, factors, errors = decompose_to_npz(tensor, config, out_dir, backend=backend, return_errors=True, **kwargs)
    fm = np.load(os.path.join(out_dir, "Factor_Matrices.npz"))
    pairs = [(fm[k], b) for k, b in zip(("U_yaw", "U_pitch", "U_roll"), bins)]
    for (U, b), name in zip(pairs, ("yaw", "pitch", "roll")):
        if U.shape[0] != len(b):
            raise ValueError(f"{name}: the tensor has {U.shape[0]} bins but config[{name}_bins] gives {len(b)}")
    optimized = TD_Trainer.Train(*pairs, backend="device" if backend == "device" else "host")
    Wh = np.ascontiguousarray(W.detach().cpu().numpy() if hasattr(W, "detach") else W, dtype=np.float32)
    np.savez(os.path.join(out_dir, "Trained_data.npz"), optimized_yaw=optimized[0], optimized_pitch=optimized[1],
             optimized_roll=optimized[2], CoreTensor=Wh, W=Wh)
    return (W, factors, optimized, errors) if return_errors else (W, factors, optimized)
