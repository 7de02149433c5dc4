"""CPU: the TD path for identity ranks other than 5 -- everything that needs no GPU.

The rank-aware Powell state machine (nlml_powell_*_n, powell.h with n = 3 + R as a field of the state) against scipy on the
reference's objective (oracle.tucker is generic in the rank) and against FX10, the reference's own Test() at ranks 1, 3 and 8; the
range errors of the *_r entry points; the Meta kernels' shapes; the fixture's recipe."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
from scipy.optimize import minimize

import rank_fixture as RF
from nlml_hpe_amd import _lib
from nlml_hpe_amd.powell_host import minimize_powell
from oracle import tucker as TK

REF = "/root/reference"
E_SHAPE = -3


@pytest.fixture(scope="module")
def fx10(golden_dir):
    return np.load(os.path.join(golden_dir, "fx10_td_identity_rank.npz"))


def test_fixture_inputs_regenerate(fx10, tucker_art):
    """The fixture stores seeds, not inputs: the synthetic identity slices of rank 8 must come out as they were."""
    assert int(fx10["seed"]) == RF.SEED and tuple(fx10["ranks"]) == RF.RANKS and np.array_equal(fx10["picks"], np.array(RF.PICKS))
    W8 = RF.rank_W(tucker_art["W"], 8)
    assert W8.shape == (8, 3, 3, 3, 1404) and np.array_equal(W8[:5], tucker_art["W"])
    assert RF.slices_checksum(W8[5:]) == str(fx10["r8_slices_sha256"])


@pytest.mark.parametrize("R", RF.RANKS)
def test_oracle_objective_is_the_references_at_every_rank(R, fx10, tucker_art):
    """oracle.tucker (the checker of the GPU tests where FX10 has no entry) gives FX10's bits."""
    W, P, X = RF.rank_W(tucker_art["W"], R), RF.params(R), RF.noisy_faces(tucker_art, R, RF.N_PARAMS)
    Py, Pp, Pr = RF.cos_rows(tucker_art)
    err = np.array([TK.objective(p, W, x, Py, Pp, Pr) for p, x in zip(P, X)])
    assert np.array_equal(err, fx10[f"r{R}_err"])
    assert np.array_equal(np.stack([TK.x_hat(p, W, Py, Pp, Pr) for p in P[:RF.N_XHAT]]), fx10[f"r{R}_x_hat"])


@pytest.mark.parametrize("R", RF.RANKS)
def test_rank_aware_state_machine_follows_scipy_on_the_tucker_objective(R, fx10, tucker_art):
    """scipy.optimize.minimize(method='Powell') from zeros(3 + R) on the reference's objective, and the rank-aware machine stepped
    on the host with the same objective: same trial points, same nfev, same x and fun -- and both are FX10's (the reference's own
    Test() on that face)."""
    W = RF.rank_W(tucker_art["W"], R)
    Py, Pp, Pr = RF.cos_rows(tucker_art)
    i = 1
    x = RF.grid_faces(tucker_art, R)[i]
    fun = lambda p: TK.objective(p, W, x, Py, Pp, Pr)
    ref_pts = []

    def f(p):
        ref_pts.append(np.array(p, dtype=np.float64))
        return fun(p)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = minimize(f, np.zeros(3 + R), method="Powell")
    pts = []
    got = minimize_powell(fun, np.zeros(3 + R), record=pts)
    assert got.nfev == ref.nfev and got.nit == ref.nit
    assert len(pts) == len(ref_pts) and all(np.array_equal(a, b) for a, b in zip(pts, ref_pts)), "trial points diverge from scipy"
    assert np.array_equal(got.x, ref.x) and got.fun == ref.fun
    assert got.nfev == fx10[f"r{R}_nfev"][i]
    assert np.array_equal(got.x, fx10[f"r{R}_res_x"][i]) and got.fun == fx10[f"r{R}_res_fun"][i]
    assert np.array_equal(np.degrees(got.x)[:3], fx10[f"r{R}_deg"][i])


def _rosen(x):
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2))


def _flat_dir(x):                       # ignores most of the variables: zero-progress line searches
    return float((x[0] - 1) ** 2 + (x[1] + 2) ** 4 + np.sin(x[2]) ** 2)


def _nan_region(x):
    return float(np.sum((x - 0.5) ** 2)) if x[0] < 0.4 else float("nan")


@pytest.mark.parametrize("n", [4, 6, 11, 19])
@pytest.mark.parametrize("fun", [_rosen, _flat_dir, _nan_region])
def test_rank_aware_state_machine_follows_scipy(fun, n):
    """The branches the Tucker objective seldom takes (bracket recovery, NaN, zero-progress directions), at the ends of the range of n."""
    pts_ref = []

    def f(x):
        pts_ref.append(np.array(x, dtype=np.float64))
        return fun(x)
    x0 = np.linspace(-1.2, 1.0, n) if fun is _rosen else np.zeros(n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = minimize(f, x0, method="Powell")
    pts = []
    got = minimize_powell(fun, x0, record=pts)
    assert got.nfev == ref.nfev and got.nit == ref.nit
    assert len(pts) == len(pts_ref) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(pts, pts_ref))
    assert np.array_equal(got.x, ref.x, equal_nan=True)
    assert got.fun == ref.fun or (np.isnan(got.fun) and np.isnan(ref.fun))


def test_rank_aware_machine_at_eight_parameters_is_the_eight_parameter_machine():
    x0 = np.linspace(-1.2, 1.0, 8)
    a, b = [], []
    ra = minimize_powell(_rosen, x0, record=a)
    rb = minimize_powell(_rosen, x0, record=b, rank_aware=True)
    assert ra.nfev == rb.nfev and ra.nit == rb.nit and ra.status == rb.status and ra.fun == rb.fun
    assert np.array_equal(ra.x, rb.x) and len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


def test_abi_rank_range_errors():
    L = _lib.lib()
    assert L.nlml_abi_version() == 2
    for r in (0, 17, -1):
        assert L.nlml_tucker_objective_r(None, None, 1404, None, None, None, 0, None, None, r, _lib.TD_ORDER_REFERENCE, None) == E_SHAPE
        msg = L.nlml_last_error().decode()
        assert "[1, 16]" in msg and str(r) in msg, msg
        assert L.nlml_tucker_powell_r(None, None, 1404, None, 0, None, None, None, None, None, None, r, _lib.TD_ORDER_FAST, None) == E_SHAPE
        assert "[1, 16]" in L.nlml_last_error().decode()
    for r in (1, 5, 16):   # in range: N == 0 is a no-op that needs no buffers
        assert L.nlml_tucker_objective_r(None, None, 1404, None, None, None, 0, None, None, r, _lib.TD_ORDER_REFERENCE, None) == 0
        assert L.nlml_tucker_powell_r(None, None, 1404, None, 0, None, None, None, None, None, None, r, _lib.TD_ORDER_REFERENCE, None) == 0
    assert L.nlml_tucker_objective_r(None, None, 1404, None, None, None, 0, None, None, 3, 7, None) == -1   # unknown order
    assert L.nlml_powell_state_bytes_n(3) == 0 and L.nlml_powell_state_bytes_n(20) == 0
    assert L.nlml_powell_state_bytes_n(4) == L.nlml_powell_state_bytes_n(19) > L.nlml_powell_state_bytes()
    buf = C.create_string_buffer(L.nlml_powell_state_bytes_n(19))
    z = np.zeros(20)
    for n in (3, 20):
        assert L.nlml_powell_init_n(buf, n, z.ctypes.data_as(C.c_void_p), 1e-4, 1e-4) == E_SHAPE
    with pytest.raises(ValueError, match=r"\[1, 16\]"):
        minimize_powell(_rosen, np.zeros(3))
    with pytest.raises(ValueError, match=r"\[1, 16\]"):
        minimize_powell(_rosen, np.zeros(20))


def test_host_layer_names_the_range():
    import torch  # noqa: F401
    from nlml_hpe_amd import TD_Tester as HT, weights
    for bad in (0, 17):
        with pytest.raises(ValueError, match="1..16"):
            HT._rank(bad)
    assert [HT._rank(r) for r in (1, 5, 16)] == [1, 5, 16]
    for rows in (0, 26, 28, 27 * 17):
        with pytest.raises(ValueError, match=r"\[1, 16\]"):
            _lib.tucker_rank_of_rows(rows)
    assert _lib.tucker_rank_of_rows(135) == 5 and _lib.tucker_rank_of_rows(27 * 16) == 16
    W = np.zeros((3, 3, 3, 3, 1404), np.float32)
    assert weights.check_tucker_rank(W, np.zeros((10, 3))) == 3
    with pytest.raises(ValueError):
        weights.check_tucker_rank(W, np.zeros((10, 5)))
    with pytest.raises(ValueError):
        weights.check_tucker_rank(np.zeros((17, 3, 3, 3, 1404), np.float32), np.zeros((10, 17)))


def test_meta_kernels_take_the_rank_from_Wm():
    import torch
    from nlml_hpe_amd import ops  # noqa: F401  (registers torch.ops.nlml_hpe.*)
    meta = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device="meta")
    for R in (1, 3, 5, 8, 16):
        res = torch.ops.nlml_hpe.tucker_powell(meta(27 * R, 1404), meta(9, 1404), meta(3, 3, 4, dtype=torch.float64), "reference")
        assert [tuple(t.shape) for t in res] == [(9, 3 + R), (9,), (9,), (9,), (9,)] and res[0].dtype == torch.float64
        e = torch.ops.nlml_hpe.tucker_objective(meta(27 * R, 1404), meta(6, 1404), meta(6, 3 + R, dtype=torch.float64),
                                                meta(3, 3, 4, dtype=torch.float64), "fast")
        assert tuple(e.shape) == (6,) and e.dtype == torch.float64


def test_synth_grid_faces_follow_the_artefacts_rank(tucker_art):
    from nlml_hpe_amd import synth
    idx = synth.tucker_grid_indices(5, seed=2)
    for R in (3, 8):
        art = dict(tucker_art, W=RF.rank_W(tucker_art["W"], R), U_id=RF.rank_U_id(tucker_art["U_id"], R))
        X = synth.tucker_grid_faces(art, idx, noise=0.0)
        want = np.stack([TK.grid_reconstruction(art["W"].astype(np.float64), art["U_id"][i].astype(np.float64), art["U_yaw"][j].astype(np.float64),
                                                art["U_pitch"][k].astype(np.float64), art["U_roll"][l].astype(np.float64)) for i, j, k, l in idx])
        assert X.shape == (5, 1404) and np.allclose(X, want, rtol=1e-5, atol=1e-6)
    assert synth.tucker_params(4, 8).shape == (4, 11)


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout")
def test_fx10_regenerates_bit_identically(tmp_path, repo_root, golden_dir):
    env = dict(os.environ, NLML_GOLDEN_OUT=str(tmp_path), MPLBACKEND="Agg", PYTHONDONTWRITEBYTECODE="1")
    res = subprocess.run([sys.executable, os.path.join(golden_dir, "make_golden_rank.py")], cwd=repo_root, env=env,
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    a, b = np.load(os.path.join(str(tmp_path), "fx10_td_identity_rank.npz")), np.load(os.path.join(golden_dir, "fx10_td_identity_rank.npz"))
    assert set(a.files) == set(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), k
