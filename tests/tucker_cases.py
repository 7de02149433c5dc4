"""The f64 numpy oracle and the shared cases of the Tucker decomposition tests (nlml_hpe_amd/tucker_decompose.py, K7a..K7d).

The oracle is written independently of the driver: it takes singular vectors of the UNFOLDINGS (np.linalg.svd), never a Gram
matrix, for the HOSVD start and for every HOOI update, and measures the reconstruction error directly as |X - X_hat| / |X|.
It shares with the driver only the published algorithm and the sign rule (largest-magnitude entry positive, lowest index on a tie).
"""
import functools

import numpy as np

U53 = 2.0 ** -53
YAW = np.arange(-50, 51, 10)        # configs/config_TD_main.yaml: 11, 9 and 7 bins, degrees
PITCH = np.arange(-40, 41, 10)
ROLL = np.arange(-30, 31, 10)


# ---- tensors -------------------------------------------------------------------------------------------------------------------
def base_landmarks(I=37, points=52, seed=0):
    """A mean face (half as deep as it is wide and tall, as faces are) plus 8 identity modes of scales 1 .. 0.002 (geometric),
    rounded to f32 -> f32[I, points, 3]."""
    rng = np.random.default_rng(seed)
    mean = rng.normal(size=(points, 3)) * np.array([1.0, 1.0, 0.5])
    modes = rng.normal(size=(8, points, 3))
    coef = rng.normal(size=(I, 8)) * np.geomspace(1.0, 0.002, 8)
    return (mean + np.tensordot(coef, modes, axes=1)).astype(np.float32)


def _axis_matrix(axis, deg):
    c, s = np.cos(np.radians(float(deg))), np.sin(np.radians(float(deg)))
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis].astype(np.float64)


def rotation_tensor(base, yaw=YAW, pitch=PITCH, roll=ROLL):
    """Every identity's landmarks at every (yaw, pitch, roll) bin, intrinsic order (pitch about x, yaw about y, roll about z),
    f64 arithmetic, one rounding -> f32[I, ny, np, nr, 3 points]."""
    base = np.asarray(base, np.float64)
    I, P = base.shape[0], base.shape[1]
    out = np.empty((I, len(yaw), len(pitch), len(roll), 3 * P), np.float32)
    for a, y in enumerate(yaw):
        for b, p in enumerate(pitch):
            for c, r in enumerate(roll):
                M = _axis_matrix("z", r) @ _axis_matrix("y", y) @ _axis_matrix("x", p)
                out[:, a, b, c, :] = (base @ M.T).reshape(I, -1)
    return out


@functools.lru_cache(maxsize=None)
def rotation_case():
    """The host tests' rotation tensor: 37 identities, 52 points, the reference's bins."""
    X = rotation_tensor(base_landmarks())
    X.setflags(write=False)
    return X


def random_tucker_tensor(shape=(37, 5, 4, 3, 40), rank=(5, 3, 3, 3), noise=0.6, seed=3):
    """A random Tucker model of the given ranks (orthonormal factors, a core with a spread spectrum) plus Gaussian noise of relative
    Frobenius size `noise`, rounded to f32.  The noise is large enough that HOOI moves the factors away from the HOSVD start for
    several sweeps (the tests assert it on the oracle)."""
    rng = np.random.default_rng(seed)
    core = rng.normal(size=tuple(rank) + (shape[4],))
    core *= np.geomspace(1.0, 0.3, rank[0])[:, None, None, None, None]
    T = core
    for mode, (n, r) in enumerate(zip(shape[:4], rank)):
        Q = np.linalg.qr(rng.normal(size=(n, r)))[0]
        T = np.moveaxis(np.tensordot(Q, T, axes=(1, mode)), 0, mode)
    E = rng.normal(size=shape)
    return (T + E * (noise * np.linalg.norm(T) / np.linalg.norm(E))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def noisy_case():
    X = random_tucker_tensor()
    X.setflags(write=False)
    return X


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def unfold(T, mode):
    return np.moveaxis(T, mode, 0).reshape(T.shape[mode], -1)


def sign_rule(U):
    U = U.copy()
    for r in range(U.shape[1]):
        k = int(np.argmax(np.abs(U[:, r])))
        if U[k, r] < 0:
            U[:, r] *= -1.0
    return U


def leading_svd(A, R):
    """-> (U f64[n,R] under the sign rule, all singular values).  A wide A goes through the Householder QR of its transpose first
    (A = R^T Q^T, so A's left singular vectors and singular values are R^T's): what LAPACK's own driver does for such a shape,
    without computing the long right singular vectors nobody reads.  No Gram matrix is formed."""
    if A.shape[1] > 4 * A.shape[0]:
        A = np.linalg.qr(A.T, mode="r").T
    Uf, s, _ = np.linalg.svd(A, full_matrices=False)
    return sign_rule(Uf[:, :R]), s


def contract(T, U, mode):
    """T x_mode U^T."""
    return np.moveaxis(np.tensordot(U.T, T, axes=(1, mode)), 0, mode)


def expand(T, U, mode):
    """T x_mode U."""
    return np.moveaxis(np.tensordot(U, T, axes=(1, mode)), 0, mode)


def hosvd(X, rank):
    """-> (factors [4], singular values of the four unfoldings)."""
    X = np.asarray(X, np.float64)
    pairs = [leading_svd(unfold(X, m), rank[m]) for m in range(4)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def hooi(X, rank, sweeps):
    """-> one record per sweep: {"U": the four factors after it, "W": X projected on them, "err": |X - X_hat| / |X| computed
    directly, "sv": the singular values of the unfolding each factor was taken from}."""
    X = np.asarray(X, np.float64)
    U = hosvd(X, rank)[0]
    out = []
    for _ in range(sweeps):
        sv = [None] * 4
        for m in range(4):
            Y = X
            for k in range(4):
                if k != m:
                    Y = contract(Y, U[k], k)
            U[m], sv[m] = leading_svd(unfold(Y, m), rank[m])
        W = X
        for k in range(4):
            W = contract(W, U[k], k)
        Xh = W
        for k in range(4):
            Xh = expand(Xh, U[k], k)
        out.append({"U": [u.copy() for u in U], "W": W, "err": float(np.linalg.norm(X - Xh) / np.linalg.norm(X)), "sv": sv})
    return out


@functools.lru_cache(maxsize=None)
def oracle(case, sweeps):
    """Cached by case name: "rotation" | "noisy" -> (HOSVD factors, HOSVD singular values, HOOI records)."""
    X = {"rotation": rotation_case, "noisy": noisy_case}[case]()
    rank = (5, 3, 3, 3)
    f, s = hosvd(X, rank)
    return f, s, hooi(X, rank, sweeps)


# ---- the measures ---------------------------------------------------------------------------------------------------------------
def subspace_distance(U, V):
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    return float(np.linalg.norm(U @ U.T - V @ V.T, 2))


def davis_kahan(X, mode, sv, R):
    """The Davis-Kahan bound 2 |dG|_F / gap on the distance between the leading-R eigenspaces of the mode's Gram G and of a Gram
    summed in f64: |dG| <= 2 K 2^-53 tr(G) with K the length of a row of the FULL tensor's unfolding (every sum behind a projected
    tensor's Gram has at most that many terms) and tr(G) = |X|^2; gap = sv[R-1]^2 - sv[R]^2 on the oracle's own singular values."""
    X64 = np.asarray(X, np.float64)
    K = X64.size // X64.shape[mode]
    dG = 2.0 * K * U53 * float(np.sum(X64 * X64))
    gap = float(sv[R - 1] ** 2 - (sv[R] ** 2 if len(sv) > R else 0.0))
    return 2.0 * dG / gap


def span_residual(U, bins_deg):
    """Distance of U's columns from span{1, cos w, sin w} at the bins: the largest column norm of U - P U."""
    w = np.radians(np.asarray(bins_deg, np.float64))
    B = np.linalg.qr(np.stack([np.ones_like(w), np.cos(w), np.sin(w)], axis=1))[0]
    U = np.asarray(U, np.float64)
    return float(np.max(np.linalg.norm(U - B @ (B.T @ U), axis=0)))


def exact_ints(shape, seed, amax=1024):
    """Integer-valued f32 with |a| <= amax: products and their f64 sums are exact while the count stays below 2^53 / amax^2."""
    return np.random.default_rng(seed).integers(-amax, amax + 1, size=shape).astype(np.float32)


# ---- the checks the host and the GPU tests share ------------------------------------------------------------------------------------
RANK = (5, 3, 3, 3)
U52 = 2.0 ** -52


def full_rank(X):
    return list(RANK) + [X.shape[4]]


def check_against(X, U, ref_U, ref_sv, what):
    for m in range(4):
        bound = davis_kahan(X, m, ref_sv[m], RANK[m])
        d = subspace_distance(U[m], ref_U[m])
        print(f"{what} mode {m}: subspace distance {d:.3e}, Davis-Kahan bound {bound:.3e}")
        assert d <= bound, (what, m, d, bound)


def check_properties(X, W, U, err):
    """Shared with the GPU tests: orthonormal factors, the sign rule, an all-orthogonal W with descending mode norms, and the error
    formula against the directly computed |X - X_hat| / |X|.  W and U as numpy arrays."""
    X64, W64 = np.asarray(X, np.float64), np.asarray(W, np.float64)
    for m in range(4):
        n, R = U[m].shape
        assert (n, R) == (X.shape[m], RANK[m])
        # eigh's vectors are orthonormal to a small multiple of n u (LAPACK's own claim); 64 n u leaves room for its constant
        assert np.abs(U[m].T @ U[m] - np.eye(R)).max() <= 64 * n * U52
        rows = np.argmax(np.abs(U[m]), axis=0)
        assert np.all(U[m][rows, np.arange(R)] > 0), "sign rule: the largest-magnitude entry of every column is positive"
    assert W.shape == RANK + (X.shape[4],)
    # W's mode-n Gram is diag(eigenvalues) up to the eigen-solve's residual (~ n u tr) and, for an f32 W, its 2^-24 rounding
    tr = float(np.sum(W64 * W64))
    slack = 1e-6 if W.dtype == np.float32 else 1e-12
    for m in range(4):
        G = unfold(W64, m) @ unfold(W64, m).T
        assert np.abs(G - np.diag(np.diag(G))).max() <= slack * tr, "all-orthogonal"
        norms = np.sqrt(np.diag(G))
        assert np.all(norms[:-1] >= norms[1:] * (1 - slack)), "descending mode norms"
    Xh = W64
    for m in range(4):
        Xh = expand(Xh, U[m], m)
    direct = np.linalg.norm(X64 - Xh) / np.linalg.norm(X64)
    assert abs(err - direct) <= (1e-6 if W.dtype == np.float32 else 1e-9), (err, direct)
