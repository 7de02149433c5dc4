"""CPU: the Tucker decomposition driver (nlml_hpe_amd/tucker_decompose.py) on its numpy backend against the independent f64 oracle
of tests/tucker_cases.py, its properties, its artefact writers, and the argument contract of the four K7 entry points (every check
returns before any GPU call, so none of this needs a GPU)."""
import numpy as np
import pytest
import torch

import tucker_cases as TC
from nlml_hpe_amd import _lib
from nlml_hpe_amd import tucker_decompose as TD

RANK, full_rank, check_against, check_properties = TC.RANK, TC.full_rank, TC.check_against, TC.check_properties


# ---- against the oracle ---------------------------------------------------------------------------------------------------------
def test_rotation_tensor_against_oracle():
    """I = 37, 52 points, the reference's bins.  The bound means something only with a clear gap: the identity mode's
    gap / sigma_1^2 >= 1e-3 is asserted on the oracle (its spectrum here: 2663, 1654, 492, 263, 154 | 44).  The pose modes have rank
    exactly 3, so their gap is sigma_3^2 itself -- for the roll bins of +-30 degrees that is 6.5e-4 sigma_1^2, whence their own
    assertion is on the bound: below 1e-6 for every mode."""
    X = TC.rotation_case()
    f, s, recs = TC.oracle("rotation", 3)
    assert (s[0][4] ** 2 - s[0][5] ** 2) / s[0][0] ** 2 >= 1e-3
    for m in range(4):
        assert TC.davis_kahan(X, m, s[m], RANK[m]) <= 1e-6
        if m:
            assert s[m][3] <= 1e-6 * s[m][0], "a rotation tensor's pose modes have rank 3 (up to the f32 rounding of its entries)"
    W, U = TD.tucker(X, full_rank(X), n_iter_max=0, backend="numpy")
    check_against(X, U, f, s, "HOSVD")
    W, U, errs = TD.tucker(X, full_rank(X), backend="numpy", return_errors=True)
    assert len(errs) == 2, "HOOI is converged after one sweep on a rotation tensor: the second only confirms it"
    check_against(X, U, recs[1]["U"], recs[1]["sv"], "HOOI")
    for m, bins in ((1, TC.YAW), (2, TC.PITCH), (3, TC.ROLL)):
        assert TC.span_residual(U[m], bins) <= 1e-6, "pose factors lie in span{1, cos w, sin w} at the bins"


def test_noisy_tensor_sweep_by_sweep():
    """A random Tucker model of ranks (5,3,3,3) in (37,5,4,3,40) plus noise.  On the oracle: HOOI moves U_id by more than 1e-3 from
    its HOSVD start, and the factors still change between the second and the third sweep by far more than the bound, so three
    sweeps are needed and each sweep's comparison can tell one sweep from the next."""
    X = TC.noisy_case()
    f, s, recs = TC.oracle("noisy", 3)
    assert TC.subspace_distance(f[0], recs[2]["U"][0]) > 1e-3
    bound0 = TC.davis_kahan(X, 0, recs[2]["sv"][0], RANK[0])
    assert TC.subspace_distance(recs[0]["U"][0], recs[1]["U"][0]) > 1e3 * bound0
    assert TC.subspace_distance(recs[1]["U"][0], recs[2]["U"][0]) > 10 * bound0, "the third sweep still moves the factor"
    for n in (1, 2, 3):
        W, U, errs = TD.tucker(X, full_rank(X), n_iter_max=n, tol=0, backend="numpy", return_errors=True)
        assert len(errs) == n
        check_against(X, U, recs[n - 1]["U"], recs[n - 1]["sv"], f"sweep {n}")
        assert abs(errs[-1] - recs[n - 1]["err"]) <= 1e-9


def test_tol_stop_rule():
    """Stop at the first sweep whose error differs from the previous sweep's by less than tol -- read off the oracle's sequence."""
    X = TC.noisy_case()
    errs = [r["err"] for r in TC.oracle("noisy", 3)[2]]
    d12, d23 = abs(errs[0] - errs[1]), abs(errs[1] - errs[2])
    assert d12 > 100 * d23 > 0, "the oracle's error sequence separates a tol between its first two differences"
    tol = np.sqrt(d12 * d23)
    assert len(TD.tucker(X, full_rank(X), tol=tol, backend="numpy", return_errors=True)[2]) == 3      # d12 >= tol, d23 < tol
    assert len(TD.tucker(X, full_rank(X), tol=2 * d12, backend="numpy", return_errors=True)[2]) == 2  # d12 < tol
    assert len(TD.tucker(X, full_rank(X), tol=tol, n_iter_max=2, backend="numpy", return_errors=True)[2]) == 2
    assert len(TD.tucker(X, full_rank(X), tol=0, n_iter_max=5, backend="numpy", return_errors=True)[2]) == 5


# ---- properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rotation", "noisy"])
def test_properties_numpy(case):
    X = {"rotation": TC.rotation_case, "noisy": TC.noisy_case}[case]()
    W, U, errs = TD.tucker(X, full_rank(X), n_iter_max=3, tol=0, backend="numpy", return_errors=True)
    assert W.dtype == np.float32
    check_properties(X, W, U, errs[-1])


def test_thin_core_round_trip():
    """thin_core's (core, U_feat) give W back through core x_5 U_feat -- the host equivalent of artefacts.core_to_W."""
    X = TC.rotation_case()
    W, _ = TD.tucker(X, full_rank(X), n_iter_max=1, backend="numpy")
    core, U_feat = TD.thin_core(W)
    Q = min(135, X.shape[4])
    assert core.shape == (5, 3, 3, 3, Q) and U_feat.shape == (X.shape[4], Q)
    assert core.dtype == torch.float32 and U_feat.dtype == torch.float32
    assert (U_feat.double().T @ U_feat.double() - torch.eye(Q, dtype=torch.float64)).abs().max() <= 1e-6
    back = (core.double().reshape(-1, Q) @ U_feat.double().T).reshape(W.shape).numpy()
    # the f32 roundings of core and U_feat: each term off by 2 * 2^-24 |core||U_feat|, and sum_q |core_q||U_feat_mq| <= |core row| |U_feat
    # row| <= the row norm of W's unfolding (Cauchy-Schwarz, U_feat orthonormal); doubled for the products of the two roundings' slack
    rows = np.linalg.norm(np.asarray(W, np.float64).reshape(-1, X.shape[4]), axis=1).max()
    assert np.abs(back - W).max() <= 4 * 2.0 ** -24 * rows


def test_decompose_to_npz(tmp_path):
    X = TC.rotation_case()
    cfg = {"tensor_decom_ranks": {"R_identity": 5, "R_yaw": 3, "R_pitch": 3, "R_roll": 3, "R_features": X.shape[4]}}
    W, U = TD.decompose_to_npz(X, cfg, str(tmp_path), backend="numpy", n_iter_max=1)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["Factor_Matrices.npz"], "Trained_data.npz needs the cosine fit: not written"
    d = np.load(tmp_path / "Factor_Matrices.npz")
    assert d.files == ["U_yaw", "U_pitch", "U_roll", "U_id"]
    for key, m in (("U_id", 0), ("U_yaw", 1), ("U_pitch", 2), ("U_roll", 3)):
        assert d[key].dtype == np.float32 and d[key].shape == (X.shape[m], RANK[m])
        assert np.array_equal(d[key], U[m].astype(np.float32))


def test_ranks_refused():
    X = TC.noisy_case()
    with pytest.raises(ValueError, match="R_features = I_features"):
        TD.tucker(X, [5, 3, 3, 3, X.shape[4] - 1], backend="numpy")
    with pytest.raises(ValueError, match="identity rank"):
        TD.tucker(np.zeros((20, 2, 2, 2, 3), np.float32), [17, 2, 2, 2, 3], backend="numpy")
    with pytest.raises(ValueError, match="pitch rank"):
        TD.tucker(X, [5, 3, 4, 3, X.shape[4]], backend="numpy")
    with pytest.raises(ValueError, match="backend"):
        TD.tucker(X, full_rank(X), backend="tensorly")


# ---- the argument contract of the four entry points -------------------------------------------------------------------------------
E_BADARG = -1
_mem = np.zeros(256, np.uint8)
A16 = (_mem.ctypes.data + 15) & ~15     # real memory behind every address (nothing may read it before the checks fail)
BIG = 1 << 40                           # a workspace size no query exceeds for these shapes


def k7_call(name, **over):
    """One call of a K7 entry point with small valid arguments, `over` replacing some -> (rc, message)."""
    a = dict(A=A16, X=A16, I=4, K=8, ny=2, np=2, nr=2, M=8, G=A16, Gy=A16, Gp=A16, Gr=A16, U=A16, R=2, Uy=A16, ry=2, Up=A16, rp=2,
             Ur=A16, rr=2, out=A16, ws=A16, ws_bytes=BIG)
    a.update(in64=0, out64=0)
    a.update(over)
    args = {"nlml_mode_gram": ["A", "I", "K", "G", "ws", "ws_bytes"],
            "nlml_pose_grams": ["X", "I", "ny", "np", "nr", "M", "Gy", "Gp", "Gr", "ws", "ws_bytes"],
            "nlml_project_identity": ["A", "I", "K", "U", "R", "out"],
            "nlml_project_pose": ["X", "I", "ny", "np", "nr", "M", "Uy", "ry", "Up", "rp", "Ur", "rr", "out"],
            "nlml_mode_gram_ex": ["A", "in64", "I", "K", "G", "ws", "ws_bytes"],
            "nlml_pose_grams_ex": ["X", "in64", "I", "ny", "np", "nr", "M", "Gy", "Gp", "Gr", "ws", "ws_bytes"],
            "nlml_project_identity_ex": ["A", "I", "K", "U", "R", "out", "out64"],
            "nlml_project_pose_ex": ["X", "in64", "I", "ny", "np", "nr", "M", "Uy", "ry", "Up", "rp", "Ur", "rr", "out", "out64"]}[name]
    L = _lib.lib()
    rc = getattr(L, name)(*[a[k] for k in args], None)
    return rc, L.nlml_last_error().decode()


# every refusal the contract names, for every entry point that has the argument in question
K7_BAD = [
    ("nlml_mode_gram", dict(A=None), "null buffer"), ("nlml_mode_gram", dict(G=None), "null buffer"),
    ("nlml_mode_gram", dict(ws=None), "null buffer"),
    ("nlml_mode_gram", dict(A=A16 + 2), "aligned"), ("nlml_mode_gram", dict(G=A16 + 4), "aligned"),
    ("nlml_mode_gram", dict(ws=A16 + 4), "aligned"),
    ("nlml_mode_gram", dict(I=0), "I outside"), ("nlml_mode_gram", dict(I=4097), "I outside"), ("nlml_mode_gram", dict(K=0), "K < 1"),
    ("nlml_mode_gram", dict(ws_bytes=0), "workspace too small"),
    ("nlml_pose_grams", dict(X=None), "null buffer"), ("nlml_pose_grams", dict(ws=None), "null buffer"),
    ("nlml_pose_grams", dict(Gy=None, Gp=None, Gr=None), "null buffer"),
    ("nlml_pose_grams", dict(X=A16 + 1), "aligned"), ("nlml_pose_grams", dict(Gp=A16 + 4), "aligned"),
    ("nlml_pose_grams", dict(I=0), "I < 1"), ("nlml_pose_grams", dict(M=0), "I < 1"),
    ("nlml_pose_grams", dict(ny=33), "outside 1..NLML_POSE_BINS_MAX"), ("nlml_pose_grams", dict(nr=0), "outside 1..NLML_POSE_BINS_MAX"),
    ("nlml_pose_grams", dict(ny=32, np=32, nr=2), "NLML_POSE_GRAMS_MAX_CELLS"),
    ("nlml_pose_grams", dict(ws_bytes=8), "workspace too small"),
    ("nlml_project_identity", dict(A=None), "null buffer"), ("nlml_project_identity", dict(U=None), "null buffer"),
    ("nlml_project_identity", dict(out=None), "null buffer"),
    ("nlml_project_identity", dict(A=A16 + 2), "aligned"), ("nlml_project_identity", dict(U=A16 + 4), "aligned"),
    ("nlml_project_identity", dict(I=0), "I < 1"), ("nlml_project_identity", dict(K=0), "I < 1"),
    ("nlml_project_identity", dict(R=17), "R outside"), ("nlml_project_identity", dict(R=0), "R outside"),
    ("nlml_project_pose", dict(X=None), "null buffer"), ("nlml_project_pose", dict(out=None), "null buffer"),
    ("nlml_project_pose", dict(out=A16 + 2), "aligned"), ("nlml_project_pose", dict(Up=A16 + 4), "aligned"),
    ("nlml_project_pose", dict(I=0), "I < 1"), ("nlml_project_pose", dict(ny=33), "outside 1..NLML_POSE_BINS_MAX"),
    ("nlml_project_pose", dict(ry=17), "rank of a given factor"), ("nlml_project_pose", dict(rr=4), "rank of a given factor"),
    ("nlml_project_pose", dict(rp=0), "rank of a given factor"),
]
# the *_ex forms run the same checks (the plain forms are calls of them); an f64 tensor must be 8-byte aligned
K7_BAD += [(n + "_ex", o, m) for n, o, m in K7_BAD]
K7_BAD += [("nlml_mode_gram_ex", dict(in64=1, A=A16 + 4), "aligned"), ("nlml_pose_grams_ex", dict(in64=1, X=A16 + 4), "aligned"),
           ("nlml_project_identity_ex", dict(out64=1, out=A16 + 4), "aligned"), ("nlml_project_pose_ex", dict(in64=1, X=A16 + 4), "aligned"),
           ("nlml_project_pose_ex", dict(out64=1, out=A16 + 4), "aligned")]


@pytest.mark.parametrize("name,over,message", K7_BAD, ids=[f"{n[5:]}-{'-'.join(f'{k}={v}' if not isinstance(v, int) or v < 1000 else k for k, v in o.items())}" for n, o, _ in K7_BAD])
def test_k7_bad_arguments(name, over, message):
    rc, msg = k7_call(name, **over)
    assert rc == E_BADARG
    assert msg.startswith(name[5:].replace("_ex", "") + ": ") and message in msg, msg


def test_k7_workspace_queries():
    L = _lib.lib()
    assert L.nlml_mode_gram_workspace_bytes(0, 8) == 0 and L.nlml_mode_gram_workspace_bytes(4097, 8) == 0
    assert L.nlml_pose_grams_workspace_bytes(1, 33, 1, 1, 8) == 0 and L.nlml_pose_grams_workspace_bytes(1, 32, 32, 2, 8) == 0
    tile = 128 * 128 * 8
    assert L.nlml_mode_gram_workspace_bytes(37, 5) == tile                      # one tile, one K slice
    assert L.nlml_mode_gram_workspace_bytes(130, _lib.MODE_GRAM_KCHUNK + 1) == 3 * 2 * tile   # three tiles of the triangle, two slices
    # one partial per slab of 16 columns (the f64 form's; the f32 form's slabs are 32 wide and use half of it), at most 1024
    assert L.nlml_pose_grams_workspace_bytes(3, 11, 9, 7, 1404) == 3 * 88 * (121 + 81 + 49) * 8
    assert L.nlml_pose_grams_workspace_bytes(1620, 11, 9, 7, 1404) == 1024 * (121 + 81 + 49) * 8
    # the refusal of a short workspace is exact to the byte
    need = L.nlml_mode_gram_workspace_bytes(4, 8)
    assert k7_call("nlml_mode_gram", ws_bytes=need - 1)[0] == E_BADARG
