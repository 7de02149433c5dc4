"""GPU: the four primitives of the Tucker decomposition (csrc/tucker_decompose.hip, K7a..K7d) and the driver on them.

Exactly summable inputs (integer-valued f32, |a| <= 1024) make every f64 sum exact whatever its order, so the Grams must equal the
integer Gram bit for bit; random inputs are held to the f64 accumulation bound.  Shapes sit below, at and above every size at which
the kernels change path: one matrix-core tile (16), one workgroup tile (128), one LDS stage (32 columns), K not a multiple of 4
(scalar loads), more than one K slice, a partial last slice.

What this file does not reach is in tests/test_tucker_order_gpu.py (inputs in tests/tucker_order_cases.py, their host side in
tests/test_tucker_order_host.py): exact answers for K7a with three and more tile rows, at NLML_GRAM_I_MAX and with slices longer than
NLML_GRAM_KCHUNK; for K7b where a workgroup takes several slabs and on its n > 16 branch for every mode; every rank instance of K7c;
every rank triple, NULL pattern and dtype form of K7d; the scalar-load forms through an unaligned base pointer; and, on random
inputs, each kernel's summation order bit for bit against the host models of oracle/csrc/oracle.c."""
import functools

import numpy as np
import pytest
import torch

import tucker_cases as TC
from nlml_hpe_amd import CreateTensor as CT
from nlml_hpe_amd import _lib, ops
from nlml_hpe_amd import tucker_decompose as TD
from tucker_cases import RANK, check_against, check_properties, full_rank

pytestmark = pytest.mark.gpu
U53, U24 = 2.0 ** -53, 2.0 ** -24
SHAPES = [(3, 11, 9, 7, 1404), (37, 5, 4, 3, 100), (2, 1, 1, 1, 7), (1, 32, 2, 2, 33)]
NULLS = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]          # 1: that factor is None


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def exact_gram(A):
    """A: integer-valued, |a| <= 1024, K < 2^33: every partial sum is an integer below 2^53, so the f64 product is the integer
    Gram whatever order BLAS adds in; small cases go through int64 itself."""
    if A.shape[0] ** 2 * A.shape[1] <= 5e7:
        Ai = A.astype(np.int64)
        G = (Ai @ Ai.T).astype(np.float64)
    else:
        G = A.astype(np.float64) @ A.astype(np.float64).T
    assert np.all(G == np.rint(G)) and np.abs(G).max() < 2.0 ** 53
    return G


# ---- K7a ------------------------------------------------------------------------------------------------------------------------
KCH = _lib.MODE_GRAM_KCHUNK
# the last pair: three K slices with one tile (the workspace query below confirms it), the last of them 7 columns -- a partial slice,
# a partial LDS stage and a K that is no multiple of 4
K7A_EXACT = [(I, K) for I in (1, 15, 16, 17, 37, 130) for K in (1, 3, 4, 5, 1403, 27 * 1404)] + [(37, 2 * KCH + 7)]


@pytest.mark.parametrize("I,K", K7A_EXACT)
def test_mode_gram_exact(device, I, K):
    if (I, K) == K7A_EXACT[-1]:
        assert _lib.lib().nlml_mode_gram_workspace_bytes(I, K) == 3 * 128 * 128 * 8
    if K == 27 * 1404:
        assert _lib.lib().nlml_mode_gram_workspace_bytes(I, K) > (1 if I <= 128 else 3) * 128 * 128 * 8, "more than one K slice"
    A = TC.exact_ints((I, K), seed=I * 100003 + K)
    At = torch.from_numpy(A).to(device)
    G = ops.mode_gram(At)
    assert G.shape == (I, I) and G.dtype == torch.float64
    assert same_bits(G, G.T), "the mirror half equals the upper half bit for bit"
    assert same_bits(G, ops.mode_gram(At)), "two runs give the same bits"
    assert np.array_equal(G.cpu().numpy(), exact_gram(A))


@pytest.mark.parametrize("I,K", [(37, 1403), (130, 27 * 1404), (17, 2 * KCH + 7)])
def test_mode_gram_random(device, I, K):
    A = np.random.default_rng(K).normal(size=(I, K)).astype(np.float32)
    G = ops.mode_gram(torch.from_numpy(A).to(device))
    A64 = A.astype(np.float64)
    assert same_bits(G, G.T)
    assert np.all(np.abs(G.cpu().numpy() - A64 @ A64.T) <= 2 * K * U53 * (np.abs(A64) @ np.abs(A64).T))


# ---- K7b ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_pose_grams_exact(device, shape):
    X = TC.exact_ints(shape, seed=sum(shape))
    Xt = torch.from_numpy(X).to(device)
    want = [exact_gram(TC.unfold(X, m)) for m in (1, 2, 3)]
    G = ops.pose_grams(Xt)
    for g, w in zip(G, want):
        assert np.array_equal(g.cpu().numpy(), w)
        assert same_bits(g, g.T)
    for g, g2 in zip(G, ops.pose_grams(Xt)):
        assert same_bits(g, g2), "two runs give the same bits"
    for skip in range(3):
        part = ops.pose_grams(Xt, which=[m != skip for m in range(3)])
        assert part[skip] is None
        assert all(same_bits(part[m], G[m]) for m in range(3) if m != skip), "a skipped output changes nothing else"


def test_pose_grams_random(device):
    shape = SHAPES[1]
    X = np.random.default_rng(1).normal(size=shape).astype(np.float32)
    G = ops.pose_grams(torch.from_numpy(X).to(device))
    for m in (1, 2, 3):
        A = TC.unfold(X.astype(np.float64), m)
        assert np.all(np.abs(G[m - 1].cpu().numpy() - A @ A.T) <= 2 * A.shape[1] * U53 * (np.abs(A) @ np.abs(A).T))


# ---- K7c ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_project_identity(device, shape):
    I, K = shape[0], int(np.prod(shape[1:]))
    R = min(5, I)
    rng = np.random.default_rng(K + I)
    A = rng.normal(size=(I, K)).astype(np.float32)
    U = rng.normal(size=(I, R))
    At, Ut = torch.from_numpy(A).to(device), torch.from_numpy(U).to(device)
    out = ops.project_identity(At, Ut)
    assert out.shape == (R, K) and out.dtype == torch.float32
    ref = U.T @ A.astype(np.float64)
    bound = U24 * np.abs(ref) + I * U53 * (np.abs(U).T @ np.abs(A.astype(np.float64)))   # one f32 rounding + the I-term fma chain
    assert np.all(np.abs(out.cpu().numpy().astype(np.float64) - ref) <= bound)
    assert same_bits(out, ops.project_identity(At, Ut)), "two runs give the same bits"
    pick = torch.eye(I, dtype=torch.float64, device=device)[:, [I - 1 - r for r in range(R)]]     # one-hot columns: rows of A, exactly
    assert same_bits(ops.project_identity(At, pick), At[[I - 1 - r for r in range(R)]])


# ---- K7d ------------------------------------------------------------------------------------------------------------------------
def contract_pose(X64, Us):
    T = X64
    for m, U in zip((1, 2, 3), Us):
        if U is not None:
            T = TC.contract(T, U, m)
    return T


@pytest.mark.parametrize("shape", SHAPES)
def test_project_pose(device, shape):
    rng = np.random.default_rng(sum(shape) + 1)
    X = rng.normal(size=shape).astype(np.float32)
    X64 = X.astype(np.float64)
    Xt = torch.from_numpy(X).to(device)
    Ufull = [rng.normal(size=(n, min(3, n))) for n in shape[1:4]]
    for nulls in NULLS:
        Us = [None if z else u for z, u in zip(nulls, Ufull)]
        Ut = [None if u is None else torch.from_numpy(u).to(device) for u in Us]
        out = ops.project_pose(Xt, *Ut)
        ref = contract_pose(X64, Us)
        assert out.shape == ref.shape
        if all(nulls):
            assert same_bits(out, Xt), "nothing to contract: a bit-for-bit copy"
            continue
        terms = int(np.prod([u.shape[0] for u in Us if u is not None]))
        spread = contract_pose(np.abs(X64), [None if u is None else np.abs(u) for u in Us])
        assert np.all(np.abs(out.cpu().numpy().astype(np.float64) - ref) <= U24 * np.abs(ref) + terms * U53 * spread), nulls
        assert same_bits(out, ops.project_pose(Xt, *Ut)), "two runs give the same bits"
    # identity-matrix factors select: exact
    eyes = [torch.eye(n, dtype=torch.float64, device=device)[:, :min(3, n)] for n in shape[1:4]]
    assert same_bits(ops.project_pose(Xt, *eyes), Xt[:, :eyes[0].shape[1], :eyes[1].shape[1], :eyes[2].shape[1]])
    assert same_bits(ops.project_pose(Xt, None, eyes[1], None), Xt[:, :, :eyes[1].shape[1]])


# ---- the f64 forms: a projected tensor kept unrounded between two steps ------------------------------------------------------------
def test_f64_tensors_in_and_out(device):
    """K7a and K7b on an f64 copy of exactly summable inputs give the f32 input's bits (the same exact sums); K7c and K7d with f64 out
    give sums that round to the f32 form's bits, within the accumulation bound alone of the f64 reference; K7d takes f64 in."""
    f64 = torch.float64
    for I, K in ((17, 5), (130, 1403), (37, 2 * KCH + 7)):
        A = torch.from_numpy(TC.exact_ints((I, K), seed=K)).to(device)
        G = ops.mode_gram(A.double())
        assert same_bits(G, ops.mode_gram(A)) and same_bits(G, G.T) and same_bits(G, ops.mode_gram(A.double()))
    for shape in SHAPES:
        X = torch.from_numpy(TC.exact_ints(shape, seed=sum(shape))).to(device)
        for g32, g64 in zip(ops.pose_grams(X), ops.pose_grams(X.double())):
            assert same_bits(g32, g64)
        rng = np.random.default_rng(sum(shape))
        Xr = rng.normal(size=shape).astype(np.float32)
        Xt = torch.from_numpy(Xr).to(device)
        Us = [rng.normal(size=(n, min(3, n))) for n in shape[1:4]]
        Ut = [torch.from_numpy(u).to(device) for u in Us]
        out64 = ops.project_pose(Xt, *Ut, out_dtype=f64)
        assert out64.dtype == f64 and same_bits(out64.float(), ops.project_pose(Xt, *Ut)), "the f32 form is the f64 form rounded once"
        ref = contract_pose(Xr.astype(np.float64), Us)
        # three nested chains of nr, np and ny terms: (1 + u)^(nr + np + ny) - 1 relative on every term's magnitude -- for the kernel's
        # fma chains and as much again for the reference's own three f64 contractions
        depth = sum(shape[1:4])
        spread = contract_pose(np.abs(Xr.astype(np.float64)), [np.abs(u) for u in Us])
        assert np.all(np.abs(out64.cpu().numpy() - ref) <= 2 * depth * U53 * spread)
        assert same_bits(ops.project_pose(Xt.double(), *Ut, out_dtype=f64), out64), "f64 in: the same sums"
        assert same_bits(ops.project_pose(Xt.double(), *Ut), out64.float())
        assert same_bits(ops.project_pose(Xt.double(), None, None, None, out_dtype=f64), Xt.double())
        assert same_bits(ops.project_pose(Xt, None, None, None, out_dtype=f64), Xt.double()), "no factor, f64 out: a widening copy"
        I = shape[0]
        U = torch.from_numpy(rng.normal(size=(I, min(5, I)))).to(device)
        z64 = ops.project_identity(Xt.reshape(I, -1), U, out_dtype=f64)
        assert z64.dtype == f64 and same_bits(z64.float(), ops.project_identity(Xt.reshape(I, -1), U))


def test_compiled_torch_ops_give_the_same_bits(device):
    """torch.ops.nlml_hpe.* (csrc/torch_ops.cpp) call the same entry points as the ctypes wrappers; their Meta kernels give the shapes."""
    rng = np.random.default_rng(4)
    X = torch.from_numpy(rng.normal(size=SHAPES[1]).astype(np.float32)).to(device)
    A = X.reshape(X.shape[0], -1)
    U = torch.from_numpy(rng.normal(size=(X.shape[0], 5))).to(device)
    Up = torch.from_numpy(rng.normal(size=(X.shape[2], 3))).to(device)
    T = torch.ops.nlml_hpe
    assert same_bits(T.mode_gram(A), ops.mode_gram(A))
    assert all(same_bits(a, b) for a, b in zip(T.pose_grams(X), ops.pose_grams(X)))
    assert same_bits(T.project_identity(A, U), ops.project_identity(A, U))
    assert same_bits(T.project_pose(X, None, Up, None), ops.project_pose(X, None, Up, None))
    Xm, Um, Upm = X.to("meta"), U.to("meta"), Up.to("meta")
    assert T.mode_gram(Xm.reshape(37, -1)).shape == (37, 37) and [g.shape[0] for g in T.pose_grams(Xm)] == [5, 4, 3]
    assert T.project_identity(Xm.reshape(37, -1), Um).shape == (5, A.shape[1])
    assert T.project_pose(Xm, None, Upm, None).shape == (37, 5, 3, 3, 100)


# ---- offsets beyond 4 GiB -------------------------------------------------------------------------------------------------------
def test_offsets_beyond_4_gib(device):
    """(1104, 11, 9, 7, 1404) f32 = 4.297 GB, the smallest identity count of the reference's grid whose last block crosses 2^32 bytes.
    Identities 1100..1103 are copies of identities 0..3, so K7a's rows and columns 1100..1103 must repeat rows and columns 0..3 bit
    for bit (the same products in the same order, from addresses 4 GiB apart), and K7c with one-hot columns must return those
    identities' slices."""
    I = 1104
    base = np.random.default_rng(11).normal(size=(I, 468, 3)).astype(np.float32)
    base[1100:] = base[:4]
    X, _ = CT.Compose_Tensor(base, (I, 11, 9, 7, 1404), TC.YAW, TC.PITCH, TC.ROLL)
    assert X.numel() * 4 > 2 ** 32
    A = X.reshape(I, -1)
    G = ops.mode_gram(A)
    assert same_bits(G, G.T)
    assert same_bits(G[1100:, :1100], G[:4, :1100]) and same_bits(G[1100:, 1100:], G[:4, :4])
    assert not same_bits(G[1099, :1099], G[3, :1099])
    ids = [0, 551, 1101, 1103]
    out = ops.project_identity(A, torch.eye(I, dtype=torch.float64, device=device)[:, ids])
    assert same_bits(out, A[ids])
    assert same_bits(out[2], A[1]) and same_bits(out[3], A[3])
    del X, A, G, out
    torch.cuda.empty_cache()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rotation_e2e(device):
    """The prototype's rotation tensor at full width: 37 identities, 468 points, the reference's bins, composed on the device ->
    (X on the device, X on the host, the oracle's record after one HOOI sweep)."""
    X, _ = CT.Compose_Tensor(TC.base_landmarks(37, 468), (37, 11, 9, 7, 1404), TC.YAW, TC.PITCH, TC.ROLL)
    Xh = X.cpu().numpy()
    return X, Xh, TC.hooi(Xh, RANK, 1)[0]


def host(U):
    return [u.cpu().numpy() for u in U]


def test_rotation_tensor_end_to_end(device):
    X, Xh, rec = rotation_e2e(device)
    sv = rec["sv"]
    assert (sv[0][4] ** 2 - sv[0][5] ** 2) / sv[0][0] ** 2 >= 1e-3
    W, U, errs = TD.tucker(X, full_rank(X), n_iter_max=1, backend="device", return_errors=True)
    U = host(U)
    check_against(Xh, U, rec["U"], sv, "device, one sweep")
    for m, bins in ((1, TC.YAW), (2, TC.PITCH), (3, TC.ROLL)):
        r = TC.span_residual(U[m], bins)
        print(f"mode {m}: distance from span{{1, cos, sin}} {r:.3e}")
        assert r <= 1e-6
    check_properties(Xh, W.cpu().numpy(), U, errs[-1])
    Wn, Un = TD.tucker(Xh, full_rank(X), n_iter_max=1, backend="numpy")
    for m in range(4):
        d, bound = TC.subspace_distance(U[m], Un[m]), 2 * TC.davis_kahan(Xh, m, sv[m], RANK[m])
        print(f"mode {m}: device against numpy backend {d:.3e}, twice the bound {bound:.3e}")
        assert d <= bound
    # the default stop rule: the second sweep confirms the first
    assert len(TD.tucker(X, full_rank(X), backend="device", return_errors=True)[2]) == 2
    # W is what K3 consumes
    params = torch.zeros((4, 8), dtype=torch.float64, device=device)
    cosp = torch.ones((3, 3, 4), dtype=torch.float64, device=device)
    err = ops.tucker_objective(W.reshape(135, 1404), X[:4, 5, 4, 3].contiguous(), params, cosp)
    assert err.shape == (4,) and bool(torch.isfinite(err).all())


def test_noisy_tensor_on_the_device(device):
    """The non-rotation tensor, sweep by sweep, against the oracle within the same Davis-Kahan bound."""
    Xh = TC.noisy_case()
    X = torch.from_numpy(np.array(Xh)).to(device)
    recs = TC.oracle("noisy", 3)[2]
    for n in (1, 2, 3):
        W, U, errs = TD.tucker(X, full_rank(X), n_iter_max=n, tol=0, backend="device", return_errors=True)
        check_against(Xh, host(U), recs[n - 1]["U"], recs[n - 1]["sv"], f"device, sweep {n}")
    check_properties(Xh, W.cpu().numpy(), host(U), errs[-1])
