"""Test helper: the inputs on which the matrix-core ("fast") order of the TD path is pinned bit for bit, and the host statement of that
order they are compared with (oracle.c_oracle.tucker_objective_fast).  Shared by tests/test_td_fast_order_host.py (which shows, without
a GPU, that the model is the established rank-5 order and that these inputs tell wrong orders apart) and tests/test_td_fast_order_gpu.py
(which runs the kernels on exactly them).  Deterministic data preparation on top of tests/rank_fixture.py; no test here, and nothing
here looks at the code under test.

  objective_case   R -> the 37 draws of rank_fixture (parameters and noisy faces) and the model's err / x_hat for them, made once;
  shared_rows      the same parameters over the first 7 faces through x_index = arange(37) * 3 % 7;
  exact_case       R -> integer data on which every order gives the same, exactly representable answer (int64 numpy has it);
  powell_*         the faces and starts of the Powell replays.
"""
from __future__ import annotations

import numpy as np

import powell_cases as PC
import rank_fixture as RF
from nlml_hpe_amd import synth
from oracle import c_oracle as CO

F = 1404
RANKS = (1, 2, 3, 4, 5, 8, 16)      # 27 R mod 4 = 3, 2, 1, 0 (ranks 1..4: 1, 2, 3, 0 padding rows; 7, 14, 21, 27 K steps: every residue mod 3);
#                                     5 the tuned kernels; 8; 16 the full coefficient table
BATCHES = (1, 15, 16, 17, 37)       # one evaluation; one short of, exactly, one more than a workgroup; two workgroups + 5
N_MAX = 37
SHARED_ROWS = 7
VARIANTS = {1: "q descending", 2: "multiply and add not fused", 3: "residual summed left to right", 4: "wave 7's repeated columns counted",
            5: "coefficient rounded to f32"}
ERR_ONLY = (3, 4)                   # these two leave x_hat as it is by construction: they re-order or extend the residual sum alone


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float64)
    return a.view(np.uint64)


def mismatches(a, b) -> int:
    """Words that differ (no NaN is expected on either side: a NaN equals only the same NaN here)."""
    return int((bits(a) != bits(b)).sum())


def cos_params(art: dict) -> np.ndarray:
    return np.ascontiguousarray(np.stack(RF.cos_rows(art)), np.float64)


_OBJ = {}


def objective_case(art: dict, R: int) -> dict:
    """W f32[R,3,3,3,1404], Wm f32[27R,1404], P f64[37,3+R], X f32[37,1404], cp f64[3,3,4], fvec f64[37,3,3] and the model's err f64[37],
    x_hat f64[37,1404] (read-only).  Evaluation n is independent of the batch, so a batch of N < 37 is the first N rows."""
    if R not in _OBJ:
        W = RF.rank_W(art["W"], R)
        c = dict(R=R, W=W, Wm=np.ascontiguousarray(W.reshape(-1, F)), P=RF.params(R, N_MAX), X=RF.noisy_faces(art, R, N_MAX), cp=cos_params(art))
        c["fvec"] = CO.tucker_fvec(c["P"], c["cp"])
        c["err"], c["x_hat"] = CO.tucker_objective_fast(c["Wm"], c["X"], c["P"], c["cp"], want_xhat=True, fvec=c["fvec"])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _OBJ[R] = c
    return _OBJ[R]


def shared_rows(art: dict, R: int) -> dict:
    """The 37 parameter sets of objective_case on its first 7 faces: x_index, the 7 rows, and the model's answer for the gathered
    contiguous call."""
    c = objective_case(art, R)
    xi = (np.arange(N_MAX) * 3 % SHARED_ROWS).astype(np.int32)
    X7 = np.ascontiguousarray(c["X"][:SHARED_ROWS])
    err, xh = CO.tucker_objective_fast(c["Wm"], np.ascontiguousarray(X7[xi]), c["P"], c["cp"], want_xhat=True, fvec=c["fvec"])
    return dict(c, x_index=xi, X7=X7, err=err, x_hat=xh)


def padded(X: np.ndarray, ldx: int, spare_rows: int = 0) -> np.ndarray:
    """X's rows at stride ldx, NaN in the pad columns (and in `spare_rows` more rows) -> f32[len(X) + spare_rows, ldx]."""
    out = np.full((len(X) + spare_rows, ldx), np.nan, np.float32)
    out[:len(X), :F] = X
    return out


# ---- exactly summable inputs ------------------------------------------------------------------------------------------------------

EXACT_RANKS = (1, 2, 3, 4, 5, 6, 7, 16)
EXACT_BATCHES = (1, 17, 37)
EXACT_D = np.array([[1, 2, -3], [-1, 4, 2], [3, -2, 1]], np.int64)
_EXACT = {}


def exact_case(R: int) -> dict:
    """Cosine rows (0, 1, 0, d): f = 0 cos(w) + d = d exactly, whatever the angle.  Integer u_id in [-4, 4], integer Wm in [-1024, 1024],
    x = x_hat + integers in [-1000, 1000].  The int64 computation is done here; the bounds that make it THE answer in any summation
    order (every partial sum an integer below 2^23, x below 2^24 and so exact in f32, the sum of squares below 2^53) are asserted by the
    tests from `abs_sum`, `X` and `ss`.  The x rows are stored permuted behind two NaN rows and reached through x_index."""
    if R not in _EXACT:
        g = synth.rng(RF.SEED + R, 601)
        Wi = g.integers(-1024, 1025, size=(27 * R, F), dtype=np.int64)
        ui = g.integers(-4, 5, size=(N_MAX, R), dtype=np.int64)
        noise = g.integers(-1000, 1001, size=(N_MAX, F), dtype=np.int64)
        P = np.empty((N_MAX, 3 + R))
        P[:, :3] = g.uniform(-1.5, 1.5, size=(N_MAX, 3))             # the angles do not matter: a = 0
        P[:, 3:] = ui
        cp = np.zeros((3, 3, 4))
        cp[:, :, 1] = 1.0
        cp[:, :, 3] = EXACT_D
        ci = np.einsum("ni,j,k,l->nijkl", ui, EXACT_D[0], EXACT_D[1], EXACT_D[2]).reshape(N_MAX, 27 * R)
        xh = ci @ Wi
        abs_sum = np.abs(ci) @ np.abs(Wi)                            # bounds every partial sum of every chain in any order
        Xi = xh + noise
        ss = (noise ** 2).sum(axis=1)
        perm = g.permutation(N_MAX)
        _EXACT[R] = dict(R=R, Wm=Wi.astype(np.float32), P=P, cp=cp, x_hat_int=xh, abs_sum=abs_sum, X_int=Xi, X=Xi.astype(np.float32), ss=ss,
                         err=0.5 * ss.astype(np.float64), x_hat=xh.astype(np.float64), perm=perm)
    return _EXACT[R]


def exact_batch(c: dict, N: int):
    """The first N evaluations of exact_case: (x buffer f32[2 + N, 1404] -- two NaN rows, then the N rows permuted --, x_index i32[N])."""
    perm = np.argsort(np.argsort(c["perm"][:N]))                     # a permutation of 0..N-1
    buf = np.full((2 + N, F), np.nan, np.float32)
    buf[2 + perm] = c["X"][:N]
    return buf, (2 + perm).astype(np.int32)


# ---- Powell replays ---------------------------------------------------------------------------------------------------------------

POWELL_RANKS = (1, 3, 8)
START_R3 = (0.1, -0.05, 0.02, 0.01, -0.02, 0.03)                     # the start of test_td_rank_gpu.test_device_powell_takes_a_start


def model_objective(Wm: np.ndarray, cp: np.ndarray, face: np.ndarray):
    """p -> the matrix-core objective of one face on the host, for powell_cases.host_run."""
    Wm = np.ascontiguousarray(Wm, np.float32)
    x = np.ascontiguousarray(face, np.float32)[None]

    def fun(p):
        return float(CO.tucker_objective_fast(Wm, x, np.asarray(p, np.float64)[None], cp)[0])
    return fun


def powell_runs(art: dict, R: int):
    """-> (faces f32[3,1404], x0 f64[3,3+R]): two grid faces from zeros and one from a start (rank 3: START_R3; else that start's
    pattern, the identity part 0.01 (-1)^i (1 + i))."""
    faces = RF.grid_faces(art, R)[[0, 1, 0]]
    x0 = np.zeros((3, 3 + R))
    x0[2, :3] = START_R3[:3]
    x0[2, 3:] = START_R3[3:] if R == 3 else [0.01 * (-1) ** i * (1 + i) for i in range(R)]
    return np.ascontiguousarray(faces), x0


def powell_rank5_batch(art: dict):
    """17 faces = one workgroup + 1: three (face, start) pairs in turn (the batch of test_device_powell_takes_a_start_at_rank_five)
    -> (faces f32[17,1404], x0 f64[17,8], pairs i64[17])."""
    pairs = np.arange(PC.EV + 1) % 3
    x0 = np.outer([1.0, 0.5, 2.0], [0.1, -0.05, 0.02, 0.01, -0.02, 0.03, 0.02, -0.01])[pairs]
    faces = RF.grid_faces(art, 5)[[0, 2, 3]][pairs]
    return np.ascontiguousarray(faces), np.ascontiguousarray(x0), pairs
