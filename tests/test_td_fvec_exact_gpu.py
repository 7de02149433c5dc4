"""GPU: the f-vector entries f = float32(a cos(b w + c) + d), their derivatives df = float32(((-a) b) sin(b w + c)) and the bare
correctly rounded cos of csrc/cr_cos.h, AS THE DEVICE COMPILER BUILT THEM, bit for bit against tests/cr_reference.py (multi-precision
cos / sin, rounded once; tests/test_cr_reference_host.py ties it to the host build of the header) -- never against another device
result, and with no tolerance:

  * the bare cr_cos through the cosine table on ~100,000 hard arguments (artefacts.hip);
  * the f entry at every compile site that has a read-out -- the reference order at rank 5 and at ranks 1 and 16 (the two
    instantiations of tucker_objective.hip's kernel), the matrix-core order at ranks 5 and 1 (tucker_common.h, tucker_rank.h), the gradient at ranks 5 and 1
    (tucker_gradient.hip) -- on inputs built so that the float32 depends on the last bits of the cos: every one of them takes the
    header's double-double path, and a cos one ulp off would change 7 to 30 % of the results;
  * the df entry (the only read-out of cr_sin) the same way;
  * objective and gradient on the points scipy's Powell really visits (|w| to 2.6, |u_id| beyond 1.5: far outside the draws of the
    other bit-exact tests), where a handful of entries take the slow path in every run.

NOT covered here: the Powell kernel's own instantiation of the f-vectors (the instantiations of tucker_powell.hip's kernel) has
no read-out -- one flipped evaluation need not move nfev -- and stays covered by the trajectory tests of tests/test_gpu_parity.py and
tests/test_td_rank_gpu.py only."""
import os

import numpy as np
import pytest
import torch

import cr_reference as CR
import rank_fixture as RF
import td_gradient_common as GC
from nlml_hpe_amd import ops, powell_host, synth
from oracle import tucker as TK

pytestmark = pytest.mark.gpu

F = 1404
SITES = [("reference", 5), ("reference", 1), ("reference", 16), ("fast", 5), ("fast", 1), ("gradient", 5), ("gradient", 1)]


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint64 if v.dtype == np.float64 else np.uint32)


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_bare_cr_cos_on_the_device_is_correctly_rounded(device):
    """rows[j] = (1, 1, t_j, 0) at the angle 0: 1 * 0 + t_j = t_j and 1 * cos + 0 = cos are exact, so the table IS cr_cos(t_j).
    |t| <= 2^20: the correctly rounded value, bit for bit.  Beyond, the header hands over to the device library: within 2 ulp, the
    premise of the header's fast path.  NaN and +-Inf give NaN."""
    hard = CR.hard_arguments(0)
    far = np.array([np.nextafter(2.0 ** 20, np.inf), -np.nextafter(2.0 ** 20, np.inf), 3.0e6, -1.0e7, 1.0e10, 123456789.125, 1.0e15,
                    -1.0e22, 2.0 ** 600, 1.0e300, -1.7e308])
    bad = np.array([np.nan, np.inf, -np.inf])
    t = np.concatenate([hard, far, bad])
    want = CR.cr_cos(t)
    zero = torch.zeros(1, dtype=torch.float32, device=device)
    got = np.empty_like(t)
    for s in range(0, len(t), 65536):
        rows = np.zeros((len(t[s:s + 65536]), 4))
        rows[:, 0], rows[:, 1], rows[:, 2] = 1.0, 1.0, t[s:s + 65536]
        got[s:s + 65536] = ops.cosine_table(zero, _t(rows, device)).cpu().numpy()[0]
    n = len(hard)
    ulp = np.abs(got[n:n + len(far)] - want[n:n + len(far)]) / np.spacing(np.abs(want[n:n + len(far)]))
    print(f"device cr_cos: {int((_bits(got[:n]) != _bits(want[:n])).sum())} of {n} hard arguments differ from the correctly rounded value; "
          f"beyond 2^20 the library is within {ulp.max():.2f} ulp")
    assert np.array_equal(_bits(got[:n]), _bits(want[:n]))
    assert (ulp <= 2.0).all()
    assert np.isnan(got[-3:]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cos_cases(tucker_art):
    """The tie / near-tie sets and the reference's float32 for each: computed once, shared by the sites, left unchanged."""
    out = []
    for name, axis, j, row, w, _ in CR.tie_cases_cos(tucker_art):
        f = CR.f_entry(row[0], row[1], w, row[2], row[3])
        f.setflags(write=False)
        out.append((name, axis, j, row, w, f))
    return out


def _f_readout(site, R, axis, j, row, w, device):
    """The f entry of cosine row j of `axis` at the angles w, read out of a whole objective: Wm is zero except a 1 in column 0 of the
    row (identity 0, j on `axis`, 0 on the other two), every other cosine row is (0, 1, 0, 1) -- f = 0 cos + 1 = 1 exactly --
    u_id = (1, 0, ...) and x = 0.  Then x_hat[:, 0] = 1 * 1 * f * 1 * 1 = f and err = 0.5 f^2, both without a rounding (f has 24 bits).
    -> (x_hat[:, 0] or None, err or None)."""
    n = len(w)
    Wm = torch.zeros((27 * R, F), dtype=torch.float32, device=device)
    Wm[j * (9, 3, 1)[axis], 0] = 1.0
    cp = np.zeros((3, 3, 4))
    cp[:, :, 1] = cp[:, :, 3] = 1.0
    cp[axis, j] = row
    P = np.zeros((n, 3 + R))
    P[:, axis], P[:, 3] = w, 1.0
    x = torch.zeros((1, F), dtype=torch.float32, device=device)
    idx = torch.zeros(n, dtype=torch.int32, device=device)
    if site == "gradient":
        err, _ = ops.tucker_gradient(Wm, x, _t(P, device), _t(cp, device), x_index=idx)
        return None, err.cpu().numpy()
    err, xh = ops.tucker_objective(Wm, x, _t(P, device), _t(cp, device), x_index=idx, return_xhat=True, order=site)
    xh = xh.cpu().numpy()
    assert not xh[np.isfinite(xh[:, 0]), 1:].any()                           # every other column of a finite evaluation is 0
    return xh[:, 0].copy(), (err.cpu().numpy() if site == "reference" else None)


@pytest.mark.parametrize("site,R", SITES)
def test_f_entry_on_the_device_is_the_reference_float32_at_forced_ties(site, R, cos_cases, device):
    """2,005 evaluations per call: every one of the 16 evaluation slots, 125 full workgroups and a partial last one."""
    total = bad = 0
    for name, axis, j, row, w, f in cos_cases:
        xh0, err = _f_readout(site, R, axis, j, row, w, device)
        f64 = f.astype(np.float64)
        miss = 0
        if xh0 is not None:
            miss = int((_bits(xh0) != _bits(f64)).sum())
        if err is not None:
            miss = max(miss, int((_bits(err) != _bits(0.5 * f64 * f64)).sum()))
        print(f"{site} R={R} {name} (axis {axis}, row {j}): {miss} of {len(w)} f entries differ from the reference float32")
        total, bad = total + len(w), bad + miss
    print(f"{site} R={R}: {bad} mismatches of {total} slow-path entries")
    assert bad == 0


@pytest.mark.parametrize("site,R", SITES)
def test_f_entry_with_nan_and_inf_angles_is_nan_and_stays_in_its_evaluation(site, R, tucker_art, device):
    row = tuple(CR.shipped_rows(tucker_art)[1, 2])
    w = np.array([np.nan, 0.25, np.inf, -np.inf, -0.5] + [0.1 * k for k in range(14)])       # 19: two passes of slots
    xh0, err = _f_readout(site, R, 1, 2, row, w, device)
    f = CR.f_entry(row[0], row[1], w, row[2], row[3]).astype(np.float64)
    nan = np.isnan(w) | np.isinf(w)
    assert np.isnan(f[nan]).all() and not np.isnan(f[~nan]).any()
    for got, want in ((xh0, f), (err, 0.5 * f * f)):
        if got is not None:
            assert np.isnan(got[nan]).all()
            assert np.array_equal(_bits(got[~nan]), _bits(want[~nan]))
    for bad_row in ((np.nan, 1.0, 0.0, 0.0), (1.0, np.inf, 0.0, 0.0), (1.0, 1.0, 0.0, np.nan)):   # a = NaN; b = Inf (Inf * 0 too); d = NaN
        xh0, err = _f_readout(site, R, 0, 1, bad_row, w[:5], device)
        assert np.isnan(xh0 if xh0 is not None else err).all()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_df_entry_on_the_device_is_the_reference_float32_at_forced_ties(tucker_art, device):
    """cr_sin has one read-out: rank 1, u = 1, W = 1 at (row 0, column 0) only, pitch and roll rows (0, 1, 0, 1) and x[0] = 2^60, so
    that r[0] = 2^60 exactly, every other product is zero and grad_w_y = -(2^60 df) with no rounding (tests/test_td_gradient_gpu.py
    counts flips against libm through it; here the entry must EQUAL the reference's, on inputs that all take the slow path)."""
    Wm = torch.zeros((27, F), dtype=torch.float32, device=device)
    Wm[0, 0] = 1.0
    x = torch.zeros((1, F), dtype=torch.float32, device=device)
    x[0, 0] = 2.0 ** 60
    total = bad = 0
    for name, row, w, _ in CR.tie_cases_sin(tucker_art):
        want = CR.df_entry(row[0], row[1], w, row[2])
        n = len(w)
        cp = np.zeros((3, 3, 4))
        cp[:, :, 1] = cp[:, :, 3] = 1.0
        cp[0, 0] = row
        P = np.zeros((n, 4))
        P[:, 0], P[:, 3] = w, 1.0
        g = ops.tucker_gradient(Wm, x, _t(P, device), _t(cp, device), x_index=torch.zeros(n, dtype=torch.int32, device=device),
                                return_err=False)
        g0 = -g[:, 0].cpu().numpy() / 2.0 ** 60
        got = g0.astype(np.float32)
        assert np.array_equal(g0, got.astype(np.float64))                   # the read-out is exact
        miss = int((_bits(got) != _bits(want)).sum())
        print(f"df {name}: {miss} of {n} entries differ from the reference float32")
        total, bad = total + n, bad + miss
    print(f"df: {bad} mismatches of {total} slow-path entries")
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------------------------
def _replay(fun, n_par):
    pts, vals = [], []

    def rec(p):
        v = float(fun(p))
        pts.append(p.copy())
        vals.append(v)
        return v
    powell_host.minimize_powell(rec, np.zeros(n_par))
    return np.array(pts), np.array(vals)


def _entry_table(P, cp):
    """Per point, the nine f and nine df entries: (fails-the-predicate, libm's float32 differs from the correctly rounded one) for
    cos and sin -- from the reference alone.  The correctly rounded value is only formed where the predicate fails: elsewhere the
    float32 cannot depend on the last bits of the library's value (the predicate's own guarantee, checked on the host)."""
    w = P[:, :3, None]
    a, b, c, d = (np.broadcast_to(cp[None, :, :, k], (len(P), 3, 3)) for k in range(4))
    arg = CR.argument(b, w, c)
    fc, fs = CR.slow_path_cos(a, arg, d), CR.slow_path_sin(a, b, arg)
    dc, ds = np.zeros_like(fc), np.zeros_like(fs)
    if fc.any():
        dc[fc] = _bits(CR.f_from_cos(a[fc], CR.cr_cos(arg[fc]), d[fc])) != _bits(CR.f_entry_libm(a[fc], b[fc], w.repeat(3, 2)[fc], c[fc], d[fc]))
    if fs.any():
        ds[fs] = _bits(CR.df_from_sin(a[fs], b[fs], CR.cr_sin(arg[fs]))) != _bits(CR.df_entry_libm(a[fs], b[fs], w.repeat(3, 2)[fs], c[fs]))
    return fc, fs, dc, ds


@pytest.fixture(scope="module")
def trajectories(tucker_art, golden_dir):
    """scipy's Powell -- the host stepping functions, which tests/test_powell_sm.py holds to scipy's trajectory -- replayed on the
    CPU oracles, every trial point and the value the oracle returned kept: rank 5 on the C oracle in the reference order (FX5's faces
    0 and 1, BASELINE config 3's noisy faces 0 and 1), rank 3 on oracle.tucker's numpy objective (two FX10 grid faces)."""
    from oracle import c_oracle as CO
    W = np.asarray(tucker_art["W"], np.float32)
    cp = GC.cos_block(tucker_art)
    g5 = np.load(os.path.join(golden_dir, "fx5_td_end_to_end.npz"))
    idx = synth.tucker_grid_indices(4096, seed=2)
    X5 = np.concatenate([g5["x"][:2], synth.tucker_grid_faces(tucker_art, idx, 1e-3, seed=2)[:2]]).astype(np.float32)
    P5, V5, I5 = [], [], []
    for i, x in enumerate(X5):
        p, v = _replay(lambda q: CO.tucker_objective(W, x[None], q[None], cp, reference_order=True)[0], 8)
        P5.append(p), V5.append(v), I5.append(np.full(len(p), i, np.int32))
    W3 = RF.rank_W(W, 3)
    X3 = RF.grid_faces(tucker_art, 3)[:2]
    P3, V3, I3 = [], [], []
    for i, x in enumerate(X3):
        p, v = _replay(lambda q: TK.objective(q, W3, x, cp[0], cp[1], cp[2]), 6)
        P3.append(p), V3.append(v), I3.append(np.full(len(p), i, np.int32))
    out = dict(cp=cp, W5=W, X5=X5, P5=np.concatenate(P5), V5=np.concatenate(V5), I5=np.concatenate(I5),
               W3=W3, X3=X3, P3=np.concatenate(P3), V3=np.concatenate(V3), I3=np.concatenate(I3))
    for R in (5, 3):
        fc, fs, dc, ds = _entry_table(out[f"P{R}"], cp)
        out[f"fc{R}"], out[f"fs{R}"] = fc.reshape(len(fc), -1), fs.reshape(len(fs), -1)
        out[f"out_f{R}"] = dc.reshape(len(dc), -1).any(axis=1)                        # left out of an objective comparison
        out[f"out_g{R}"] = out[f"out_f{R}"] | ds.reshape(len(ds), -1).any(axis=1)      # ... of a gradient comparison
    for k, v in out.items():
        if k[0] != "W":                                                               # (W5 is the session's own array)
            v.setflags(write=False)
    return out


def test_the_replayed_points_are_the_optimisers_domain_and_reach_the_slow_path(trajectories):
    T = trajectories
    n = len(T["P5"]) + len(T["P3"])
    w_max = max(np.abs(T["P5"][:, :3]).max(), np.abs(T["P3"][:, :3]).max())
    u_max = max(np.abs(T["P5"][:, 3:]).max(), np.abs(T["P3"][:, 3:]).max())
    n_cos, n_sin = int(T["fc5"].sum() + T["fc3"].sum()), int(T["fs5"].sum() + T["fs3"].sum())
    left = int(T["out_g5"].sum() + T["out_g3"].sum())
    print(f"replayed Powell: {len(T['P5'])} points at rank 5, {len(T['P3'])} at rank 3; max |w| {w_max:.3f}, max |u_id| {u_max:.3f}; "
          f"{n_cos} of {9 * n} f entries and {n_sin} df entries fail the fast-path predicate; {left} points left out "
          f"(libm's float32 differs from the correctly rounded one at such an entry)")
    assert w_max >= 2.6 and u_max >= 1.5
    assert n_cos >= 5
    assert left <= 1e-3 * n


def test_device_objective_on_the_replayed_points_is_the_oracles_bit_for_bit(trajectories, device):
    T = trajectories
    for R in (5, 3):
        got = ops.tucker_objective(_t(T[f"W{R}"].reshape(-1, F), device), _t(T[f"X{R}"], device), _t(T[f"P{R}"], device),
                                   _t(T["cp"], device), x_index=_t(T[f"I{R}"], device), order="reference").cpu().numpy()
        keep = ~T[f"out_f{R}"]
        miss = int((_bits(got[keep]) != _bits(T[f"V{R}"][keep])).sum())
        slow = T[f"fc{R}"].any(axis=1) & keep
        print(f"rank {R}: {miss} of {int(keep.sum())} objective values differ from the oracle's ({int((~keep).sum())} left out); "
              f"{int(slow.sum())} of them have an f entry on the slow path")
        assert (~keep).sum() <= 1e-3 * len(keep)
        assert miss == 0


def test_device_gradient_on_the_replayed_points(trajectories, device):
    """500 of the rank-5 points -- every one with an f or df entry on the slow path, the rest drawn with a fixed seed -- against the
    host restatement (whose cos / sin are the same header's: nothing is left out); 100 of them against oracle.tucker's numpy
    gradient, whose cos / sin are libm's (the exclusion rule applies)."""
    T = trajectories
    n = len(T["P5"])
    hot = np.nonzero(T["fc5"].any(axis=1) | T["fs5"].any(axis=1))[0]
    rest = np.setdiff1d(np.arange(n), hot)
    pick = np.concatenate([hot, np.random.default_rng(11).permutation(rest)])[:500]
    P, I = T["P5"][pick], T["I5"][pick]
    err, grad = ops.tucker_gradient(_t(T["W5"].reshape(-1, F), device), _t(T["X5"], device), _t(P, device), _t(T["cp"], device),
                                    x_index=_t(I, device))
    err, grad = err.cpu().numpy(), grad.cpu().numpy()
    e_h, g_h = GC.gradient_host(T["W5"], T["X5"], P, T["cp"], x_index=I)
    print(f"gradient on {len(pick)} replayed points ({len(hot)} with a slow-path entry): {int((_bits(grad) != _bits(g_h)).sum())} of "
          f"{grad.size} components and {int((_bits(err) != _bits(e_h)).sum())} values differ from the host restatement")
    assert len(hot) >= 5
    assert np.array_equal(_bits(err), _bits(e_h)) and np.array_equal(_bits(grad), _bits(g_h))
    sub = pick[:100]
    keep = ~T["out_g5"][sub]
    cp = T["cp"]
    G = np.stack([TK.compute_gradient(p, T["W5"], T["X5"][i], cp[0], cp[1], cp[2]) for p, i in zip(P[:100][keep], I[:100][keep])])
    miss = int((_bits(grad[:100][keep]) != _bits(G)).sum())
    print(f"against oracle.tucker's gradient: {miss} of {G.size} components differ on {int(keep.sum())} points ({int((~keep).sum())} left out)")
    assert (~keep).sum() <= 1e-3 * n
    assert miss == 0
    assert np.array_equal(_bits(err[:100][keep]), _bits(T["V5"][sub][keep]))
