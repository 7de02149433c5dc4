"""The cosine fit of the pose factors without a GPU: the host forms of K8 (nlml_cosine_fit_objective_host, nlml_cosine_fit_host,
csrc/cosine_fit_ref.h), the Fourier start, the entry points' refusals, TD_Trainer and train_to_npz.

WHAT IS HELD TO WHAT.
  objective   bit for bit to tests/cosine_fit_cases.objective_py: Python floats in the stated order, the cos from multi-precision
              arithmetic rounded once, the square as e * e.  Shares no code with the header.
  fit         bit for bit (x, fun, nfev, nit, status) to scipy's own minimize(method='Powell') driven with the host objective: the
              machine of powell.h is checked against scipy for eight and n parameters elsewhere; here for four, on this objective.
  reference   against the literal reference (FX13, recorded by tests/golden/make_golden_cosine_fit.py), which cannot be matched bit
              for bit (np.cos and the scalar ** 2 are not correctly rounded in glibc): fun within Powell's own stopping rule, the
              parameters within 4 x the distance of the reference FROM ITSELF -- the shipped optimized_* against FX13's re-run, read
              from the two files.  Measured ratios (this fit against FX13, over that distance), per axis: yaw 1.20, pitch 0.93,
              roll 0.0003 (profiles/cosine_fit.md).
"""
import os
import subprocess

import numpy as np
import pytest

import cosine_fit_cases as CC
from cosine_fit_cases import same_bits
from nlml_hpe_amd import _lib

BADARG = -1
FAKE = 0x1000            # a non-null, aligned address no refused call may touch


def _err():
    return (_lib.lib().nlml_last_error() or b"").decode()


@pytest.fixture(scope="module")
def visits():
    """name -> (scipy result, visited points, the host objective's values there) for the nine shipped columns: scipy's real Powell
    over the HOST objective, run once."""
    cols, g = CC.shipped_columns(), CC.shipped_guess()
    out = {}
    for k, (name, (y, w)) in enumerate(cols.items()):
        out[name] = CC.scipy_powell(lambda p, y=y, w=w: float(CC.host_objective(y, w, p)[0]), g[k])
    return out


# ---- 1. the objective ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.CHEAPEST)
def test_objective_equals_the_oracle_on_every_visited_point(visits, name):
    y, w = CC.shipped_columns()[name]
    _, P, vals = visits[name]
    assert len(P) >= 400
    assert same_bits(CC.host_objective(y, w, P), vals), "one batched call gives the values of the single calls"
    want = np.array([CC.objective_py(p, y, w) for p in P])
    bad = np.flatnonzero(CC.bits(want) != CC.bits(vals))
    assert bad.size == 0, f"{name}: {bad.size} of {len(P)} values differ from the oracle, first at {P[bad[0]]}"


def test_objective_visits_about_two_thousand_points(visits):
    assert 1500 <= sum(len(visits[n][1]) for n in CC.CHEAPEST) <= 3000


@pytest.mark.parametrize("n", [1, 2, 7, 63, 64])
def test_objective_row_counts(n):
    y, w = CC.random_column(n, seed=n)
    P = CC.random_params(24, seed=100 + n)
    got = CC.host_objective(y, w, P)
    assert same_bits(got, np.array([CC.objective_py(p, y, w) for p in P]))


def test_objective_signed_zeros_and_non_finite_rows():
    w = np.array([-10.0, 0.0, 10.0, -0.0])
    for y in (np.zeros(4), -np.zeros(4), np.array([0.0, -0.0, 0.0, -0.0])):
        P = np.array([[0.0, 0.0, 0.0, 0.0], [-0.0, 1.0, -0.0, -0.0], [0.0, -0.0, 0.0, -0.0], [-0.0, -0.0, -0.0, 0.0]])
        got = CC.host_objective(y, w, P)
        assert same_bits(got, np.array([CC.objective_py(p, y, w) for p in P]))
        assert same_bits(got, np.zeros(4)), "+0.0, not -0.0"
    y, w = CC.random_column(7, seed=3)
    P = CC.random_params(4, seed=4)
    for bad in (np.nan, np.inf, -np.inf):
        yb = y.copy()
        yb[2] = bad
        got = CC.host_objective(yb, w, P)
        assert same_bits(got, np.array([CC.objective_py(p, yb, w) for p in P]))
        assert np.all(np.isnan(got)) if np.isnan(bad) else np.all(got == np.inf)
    for k in range(4):                                   # a non-finite parameter: NaN (Inf - Inf, 0 * Inf or cos(Inf) on the way)
        Pb = P.copy()
        Pb[:, k] = np.inf
        assert same_bits(CC.host_objective(y, w, Pb), np.array([CC.objective_py(p, y, w) for p in Pb]))
    wb = w.copy()
    wb[0] = np.nan
    assert np.all(np.isnan(CC.host_objective(y, wb, P)))


def test_objective_where_the_model_cancels_against_the_samples():
    """y_i a few units in the last place from a cos(b w_i + c) + d: e_i is the rounding error of m_i and the value hangs on the last
    bit of the cos."""
    rng = np.random.default_rng(9)
    w = CC.YAW.astype(np.float64)
    P = CC.random_params(64, seed=10)
    for p in P:
        t = p[1] * (w * CC.DEG2RAD) + p[2]
        y = p[0] * np.cos(t) + p[3]
        for _ in range(int(rng.integers(0, 3))):
            y = np.nextafter(y, np.inf)
        got = CC.host_objective(y, w, p[None])
        assert same_bits(got, np.array([CC.objective_py(p, y, w)]))
        assert got[0] < 1e-28


# ---- 2. the fit against scipy ---------------------------------------------------------------------------------------------------------
def test_fit_equals_scipy_on_the_nine_shipped_columns(visits):
    cols = CC.shipped_columns()
    got = CC.host_fit(list(cols.values()), CC.shipped_guess())
    for k, name in enumerate(cols):
        want = CC.scipy_outputs(visits[name][0])
        for key in CC.OUTPUTS:
            assert same_bits(got[key][k], want[key]), (name, key, got[key][k], want[key])
        print(f"{name}: nfev {got['nfev'][k]} nit {got['nit'][k]} status {got['status'][k]} fun {got['fun'][k]:.6e}")
    assert (got["status"] == CC.PW_MAXFEV).any(), "at least one shipped column ends at scipy's maxfev"
    assert np.all(got["nfev"][got["status"] == CC.PW_MAXFEV] == CC.MAXFEV)
    assert same_bits(got["x"], CC.host_fit(list(cols.values()), CC.shipped_guess(), ld=17)["x"]), "a padded stride changes nothing"


@pytest.mark.parametrize("name", ["nan", "inf_angle", "inf", "constant", "one_row", "rows64"])
def test_fit_equals_scipy_off_the_happy_path(name):
    (y, w), x0 = CC.edge_columns()[name]
    got = CC.host_fit([(y, w)], x0)
    with np.errstate(all="ignore"):
        res, _, _ = CC.scipy_powell(lambda p: float(CC.host_objective(y, w, p)[0]), x0)
    want = CC.scipy_outputs(res)
    for key in CC.OUTPUTS:
        assert same_bits(got[key][0], want[key]), (name, key, got[key][0], want[key])
    if name in ("nan", "inf_angle"):
        assert got["status"][0] == CC.PW_NAN and got["nfev"][0] == CC.NAN_NFEV
    if name == "inf":                        # the constant +Inf: 2 (fx - fval) is NaN, no stopping rule fires before maxfev
        assert got["status"][0] == CC.PW_MAXFEV and got["nfev"][0] == CC.MAXFEV and got["fun"][0] == np.inf


def test_fit_tolerances_reach_the_machine():
    (y, w) = CC.shipped_columns()["pitch1"]
    x0 = CC.shipped_guess()[4]
    got = CC.host_fit([(y, w)], x0, xtol=1e-2, ftol=1e-3)
    res, _, _ = CC.scipy_powell(lambda p: float(CC.host_objective(y, w, p)[0]), x0, xtol=1e-2, ftol=1e-3)
    want = CC.scipy_outputs(res)
    assert all(same_bits(got[k][0], want[k]) for k in CC.OUTPUTS)
    assert got["nfev"][0] < CC.host_fit([(y, w)], x0)["nfev"][0]


# ---- 3. against the literal reference --------------------------------------------------------------------------------------------------
def test_fit_against_the_reference():
    fx = CC.golden()
    _, shipped_opt = CC.shipped()
    cols = CC.shipped_columns()
    x0 = np.concatenate([fx[f"guess_{a}"] for a in CC.AXES])             # the reference's own start
    got = CC.host_fit(list(cols.values()), x0)
    assert np.all(np.abs(got["fun"] - fx["fun"]) <= 1e-4 * np.abs(fx["fun"]) + 1e-20), (got["fun"], fx["fun"])
    assert (fx["status"] == 1).any(), "the recorded run has columns that end at maxfev; they are compared like the others"
    for k, a in enumerate(CC.AXES):
        itself = np.abs(shipped_opt[a] - fx[f"optimized_{a}"]).max()
        ours = np.abs(got["x"][3 * k:3 * k + 3] - fx[f"optimized_{a}"]).max()
        print(f"{a}: this fit against FX13 {ours:.3e}, the reference against itself {itself:.3e}, ratio {ours / itself:.2f}")
        assert itself > 0
        assert ours <= 4 * itself, (a, ours, itself)


# ---- 4. the start ----------------------------------------------------------------------------------------------------------------------
def test_fourier_start_equals_the_reference():
    import scipy
    fx = CC.golden()
    got = CC.shipped_guess()
    want = np.concatenate([fx[f"guess_{a}"] for a in CC.AXES])
    if scipy.__version__ == str(fx["scipy_version"]):
        assert same_bits(got, want)
    else:
        assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want))


def test_fourier_start_keeps_the_column_dtype():
    """The shipped columns are f32 and scipy.fft keeps single precision; an f64 copy of the same column gives other bits."""
    from nlml_hpe_amd import TD_Trainer
    U, w = CC.shipped_pairs()[0]
    g32, g64 = TD_Trainer.est_params_by_Uniform_Fourier(U, w), TD_Trainer.est_params_by_Uniform_Fourier(U.astype(np.float64), w)
    assert not same_bits(g32, g64) and np.allclose(g32, g64, rtol=1e-5, atol=1e-7)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def _fit_args(y=FAKE, w=FAKE, ld=11, n=FAKE, h_n=(11, 9), C=2, x0=FAKE, x=FAKE, device=True):
    hn = np.array(h_n, np.int32) if h_n is not None else None
    args = [y, w, ld] + ([n] if device else []) + [hn.ctypes.data if hn is not None else None, C, x0, 1e-4, 1e-4, x, None, None, None, None]
    return args + ([None] if device else []), hn


@pytest.mark.parametrize("case, kw, text", [
    ("null y before a negative C", dict(y=None, C=-1), "null buffer"),
    ("null w_deg", dict(w=None), "null buffer"),
    ("null n", dict(n=None), "null buffer"),
    ("null h_n", dict(h_n=None), "null buffer"),
    ("null x0", dict(x0=None), "null buffer"),
    ("null x", dict(x=None), "null buffer"),
    ("negative C before a bad n", dict(C=-2, h_n=(0, 9)), "negative C"),
    ("n of 0 before ld < n", dict(h_n=(12, 0)), "n[1] = 0 outside [1, 64]"),
    ("n of 65", dict(h_n=(65, 9), ld=80), "n[0] = 65 outside [1, 64]"),
    ("ld below an n", dict(h_n=(11, 9), ld=10), "ld = 10 < n[0] = 11"),
    ("ld below an n before misalignment", dict(h_n=(11, 9), ld=10, y=FAKE + 4), "ld = 10"),
    ("misaligned y", dict(y=FAKE + 4), "8-byte aligned"),
    ("misaligned n", dict(n=FAKE + 2), "4-byte aligned"),
])
def test_fit_entry_point_refuses(case, kw, text):
    args, keep = _fit_args(**kw)
    assert _lib.lib().nlml_cosine_fit(*args) == BADARG, case
    assert text in _err() and _err().startswith("cosine_fit:"), (case, _err())
    if "n" not in kw and "aligned" not in text:
        hargs, keep = _fit_args(device=False, **kw)
        assert _lib.lib().nlml_cosine_fit_host(*hargs) == BADARG, case
        assert text in _err() and _err().startswith("cosine_fit_host:"), (case, _err())


def test_fit_entry_point_with_no_fits_launches_nothing():
    L = _lib.lib()
    assert L.nlml_cosine_fit(None, None, 0, None, None, 0, None, 1e-4, 1e-4, None, None, None, None, None, None) == 0
    assert L.nlml_cosine_fit(FAKE + 4, FAKE, 0, FAKE, FAKE, 0, FAKE, 1e-4, 1e-4, FAKE, None, None, None, None, None) == 0   # nothing looked at
    assert L.nlml_cosine_fit_host(None, None, 0, None, 0, None, 1e-4, 1e-4, None, None, None, None, None) == 0


@pytest.mark.parametrize("case, args, text", [
    ("null y before a negative N", (None, FAKE, 5, FAKE, -1, FAKE), "null buffer"),
    ("null params", (FAKE, FAKE, 5, None, 3, FAKE), "null buffer"),
    ("null out", (FAKE, FAKE, 5, FAKE, 3, None), "null buffer"),
    ("negative N before a bad n", (FAKE, FAKE, 0, FAKE, -3, FAKE), "negative N"),
    ("n of 0", (FAKE, FAKE, 0, FAKE, 3, FAKE), "n = 0 outside [1, 64]"),
    ("n of 65, no points", (None, None, 65, None, 0, None), "n = 65 outside [1, 64]"),
    ("misaligned params", (FAKE, FAKE, 5, FAKE + 4, 3, FAKE), "8-byte aligned"),
])
def test_objective_entry_point_refuses(case, args, text):
    assert _lib.lib().nlml_cosine_fit_objective(*args, None) == BADARG, case
    assert text in _err() and _err().startswith("cosine_fit_objective:"), (case, _err())
    if "aligned" not in text:
        assert _lib.lib().nlml_cosine_fit_objective_host(*args) == BADARG, case
        assert text in _err() and _err().startswith("cosine_fit_objective_host:"), (case, _err())


def test_objective_entry_point_with_no_points_launches_nothing():
    assert _lib.lib().nlml_cosine_fit_objective(None, None, 5, None, 0, None, None) == 0
    assert _lib.lib().nlml_cosine_fit_objective_host(None, None, 5, None, 0, None) == 0


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    import torch

    from nlml_hpe_amd import ops
    y = torch.zeros((2, 11), dtype=torch.float64)
    with pytest.raises(_lib.NlmlError, match="GPU tensor"):
        ops.cosine_fit(y, y, [11, 9], torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(_lib.NlmlError, match="GPU tensor"):
        ops.cosine_fit_objective(y, y, [11, 9], torch.zeros((3, 4), dtype=torch.float64))


# ---- 6. the layers above ---------------------------------------------------------------------------------------------------------------
def test_train_on_the_host_backend():
    from nlml_hpe_amd import TD_Trainer
    pairs = CC.shipped_pairs()
    out = TD_Trainer.Train(*pairs, backend="host", return_info=True)
    want = CC.host_fit(list(CC.shipped_columns().values()), CC.shipped_guess())
    assert [o.shape for o in out[:3]] == [(3, 4)] * 3 and all(o.dtype == np.float64 for o in out[:3])
    assert same_bits(np.concatenate(out[:3]), want["x"])
    assert all(same_bits(out[3][k], want[k]) for k in CC.OUTPUTS)
    U, w = pairs[1]
    g = TD_Trainer.est_params_by_Uniform_Fourier(U, w)
    assert same_bits(TD_Trainer.optimize_for_matrix_using_grads(U, w, g, backend="host"), out[1])
    y, wd = CC.shipped_columns()["pitch0"]
    assert TD_Trainer.objective(out[1][0], U[:, 0], w) == want["fun"][3] == CC.host_objective(y, wd, out[1][0])[0]
    assert TD_Trainer.func(0.5, 2.0, 1.0, 0.0, 1.0) == 2.0 * np.cos(0.5) + 1.0
    with pytest.raises(ValueError, match="backend"):
        TD_Trainer.Train(*pairs, backend="scipy")


def test_train_to_npz_writes_both_artefacts(tmp_path):
    import tucker_cases as TC
    from nlml_hpe_amd import tucker_decompose as TD
    from nlml_hpe_amd import weights
    X = TC.rotation_tensor(TC.base_landmarks(6, 468, seed=2))
    assert X.shape == (6, 11, 9, 7, 1404)
    W, factors, optimized = TD.train_to_npz(X, CC.CHAIN_CONFIG, str(tmp_path), backend="numpy", n_iter_max=1)
    assert sorted(os.listdir(tmp_path)) == ["Factor_Matrices.npz", "Trained_data.npz"]
    td, fm = np.load(tmp_path / "Trained_data.npz"), np.load(tmp_path / "Factor_Matrices.npz")
    assert sorted(td.files) == ["CoreTensor", "W", "optimized_pitch", "optimized_roll", "optimized_yaw"]
    assert sorted(fm.files) == ["U_id", "U_pitch", "U_roll", "U_yaw"]
    for k, a in enumerate(CC.AXES):
        o = td[f"optimized_{a}"]
        assert o.dtype == np.float64 and o.shape == (3, 4) and np.isfinite(o).all() and same_bits(o, optimized[k])
        assert fm[f"U_{a}"].dtype == np.float32 and fm[f"U_{a}"].shape == (len(CC.BINS[a]), 3)
    assert td["W"].dtype == np.float32 and td["W"].shape == (5, 3, 3, 3, 1404) and same_bits(td["W"], np.asarray(W, np.float32))
    assert same_bits(td["CoreTensor"], td["W"]), "U_feat = I: the core is W"
    assert fm["U_id"].shape == (6, 5)
    art = weights.load_tucker_artefacts(str(tmp_path))
    assert same_bits(art["optimized_yaw"], optimized[0]) and art["W"].shape == (5, 3, 3, 3, 1404)
    # the fitted curves pass through the factor columns they were fitted to
    for k, a in enumerate(CC.AXES):
        U, w = fm[f"U_{a}"].astype(np.float64), np.radians(CC.BINS[a])
        o = td[f"optimized_{a}"]
        fit = o[:, 0] * np.cos(o[:, 1] * w[:, None] + o[:, 2]) + o[:, 3]
        assert np.abs(fit - U).max() <= 0.05, (a, np.abs(fit - U).max())
    with pytest.raises(ValueError, match="bins"):
        TD.train_to_npz(X[:, :10], CC.CHAIN_CONFIG, str(tmp_path / "short"), backend="numpy", n_iter_max=1)


# ---- 7. the host forms as a stand-alone program under the sanitizers -------------------------------------------------------------------
def test_host_forms_under_asan_ubsan(tmp_path, repo_root):
    """tests/native/cosine_fit_host.cpp includes the header, fits the nine columns written to a file here and prints the results;
    built with -fsanitize=address,undefined and run directly.  Its results are the library's, bit for bit."""
    cols = list(CC.shipped_columns().values())
    Y, W, n = CC.pack(cols, ld=11)
    Y, W = np.nan_to_num(Y, nan=0.0), np.nan_to_num(W, nan=0.0)
    x0 = CC.shipped_guess()
    data = tmp_path / "columns.txt"
    with open(data, "w") as f:
        f.write(f"{len(cols)} 11\n")
        for k in range(len(cols)):
            f.write(f"{n[k]} " + " ".join(float(v).hex() for v in np.concatenate([Y[k], W[k], x0[k]])) + "\n")
    exe = tmp_path / "cosine_fit_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-o", str(exe), os.path.join(repo_root, "tests", "native", "cosine_fit_host.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    lines = [ln.split() for ln in res.stdout.splitlines() if ln.startswith("fit ")]
    assert len(lines) == len(cols) and "cosine fit host ok" in res.stdout
    want = CC.host_fit(cols, x0)
    for k, t in enumerate(lines):
        x = np.array([float.fromhex(v) for v in t[2:6]])
        assert same_bits(x, want["x"][k]) and same_bits(np.float64(float.fromhex(t[6])), want["fun"][k])
        assert [int(v) for v in t[7:10]] == [want["nfev"][k], want["nit"][k], want["status"][k]]
