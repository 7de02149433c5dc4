"""GPU: the cosine fit of the pose factors (K8, csrc/cosine_fit.hip) against its host form, and the training chain end to end.

The host form (nlml_cosine_fit_host / nlml_cosine_fit_objective_host, the same header compiled for the CPU) is held to the Python
oracle and to scipy in tests/test_cosine_fit_host.py; here the DEVICE build must return the host's bits: the objective on every
point the nine shipped fits visit and at the row counts where the lane mapping can go wrong (1, 2, 7, 63, 64 of 64 lanes, with a
padded stride whose padding is NaN), the fits in all five outputs for partial and several workgroups, mixed row counts, and the
machine's abnormal exits.

The chain test goes from base landmarks to a TD inference on artefacts this package wrote: K6, K7, K8, the two npz files, K3/Powell.
Its bound compares the pose error with the written cosine parameters to that with the parameters the REFERENCE's Train gives for the
same tensor's factors (FX13b): at most twice that, plus 0.02 deg -- last-bit changes of an objective move a Powell end point by about
6e-3 deg on clean grid faces (README), and the two parameter sets differ by more than last bits (other factors' last bits, another
cos).  Measured on an MI355X: 0.031234 deg against 0.031302 deg (profiles/cosine_fit.md).
"""
import numpy as np
import pytest
import torch

import cosine_fit_cases as CC
from cosine_fit_cases import same_bits
from nlml_hpe_amd import _lib, ops

pytestmark = pytest.mark.gpu


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def device_fit(device, cols, x0, ld=None, xtol=1e-4, ftol=1e-4):
    """ops.cosine_fit on [(y, w)] -> dict of numpy OUTPUTS."""
    Y, W, n = CC.pack(cols, ld)
    res = ops.cosine_fit(dev(Y, device), dev(W, device), n.tolist(), dev(np.asarray(x0, np.float64).reshape(len(cols), 4), device),
                         xtol=xtol, ftol=ftol)
    return {k: v.cpu().numpy() for k, v in res.items()}


def assert_same(got, want, what):
    for k in CC.OUTPUTS:
        if not same_bits(got[k], want[k]):
            bad = [f for f in range(len(want[k])) if not same_bits(got[k][f], want[k][f])]
            raise AssertionError(f"{what}: {k} differs at fits {bad[:8]}: device {got[k][bad[0]]}, host {want[k][bad[0]]}")


@pytest.fixture(scope="module")
def nine():
    """(columns, start, the host fits, the points scipy visits per column under the host objective)."""
    cols, g = CC.shipped_columns(), CC.shipped_guess()
    visited = {}
    for k, (name, (y, w)) in enumerate(cols.items()):
        visited[name] = CC.scipy_powell(lambda p, y=y, w=w: float(CC.host_objective(y, w, p)[0]), g[k])[1]
    return cols, g, CC.host_fit(list(cols.values()), g), visited


# ---- 1. the objective ----------------------------------------------------------------------------------------------------------------
def test_objective_on_every_point_the_nine_fits_visit(device, nine):
    cols, _, fits, visited = nine
    Y, W, n = CC.pack(list(cols.values()))
    Yd, Wd = dev(Y, device), dev(W, device)
    total = 0
    for f, (name, (y, w)) in enumerate(cols.items()):
        P = visited[name]
        got = ops.cosine_fit_objective(Yd, Wd, n.tolist(), dev(P, device), fit=f).cpu().numpy()
        want = CC.host_objective(y, w, P)
        bad = np.flatnonzero(CC.bits(got) != CC.bits(want))
        assert bad.size == 0, f"{name}: {bad.size} of {len(P)} values differ, first at {P[bad[0]]}: {got[bad[0]]!r} / {want[bad[0]]!r}"
        total += len(P)
    print(f"{total} points")
    assert total == int(fits["nfev"].sum()) and total > 15000, "every evaluation of the nine fits (19,640 under this objective)"


@pytest.mark.parametrize("n", [1, 2, 7, 63, 64])
def test_objective_row_counts_with_a_padded_stride(device, n):
    cols = [CC.random_column(n, seed=20 + n), CC.random_column(n, seed=40 + n)]
    Y, W, rows = CC.pack(cols, ld=n + 3)                       # the padding is NaN
    P = CC.random_params(257, seed=60 + n)                     # 64 workgroups and a partial one
    for f in (0, 1):
        got = ops.cosine_fit_objective(dev(Y, device), dev(W, device), rows.tolist(), dev(P, device), fit=f).cpu().numpy()
        assert same_bits(got, CC.host_objective(*cols[f], P)), (n, f)
    assert ops.cosine_fit_objective(dev(Y, device), dev(W, device), n, dev(P[:0], device)).shape == (0,)


# ---- 2. the fits ---------------------------------------------------------------------------------------------------------------------
def test_the_nine_shipped_columns_as_one_mixed_launch(device, nine):
    cols, g, want, _ = nine
    got = device_fit(device, list(cols.values()), g)
    assert_same(got, want, "nine columns")
    assert sorted(set(len(c[0]) for c in cols.values())) == [7, 9, 11]
    assert (got["status"] == CC.PW_MAXFEV).any() and (got["status"] == CC.PW_CONVERGED).any()
    # Train is this launch
    from nlml_hpe_amd import TD_Trainer
    out = TD_Trainer.Train(*CC.shipped_pairs(), backend="device")
    assert same_bits(np.concatenate(out), want["x"])
    # a start at a previous result
    again = device_fit(device, list(cols.values()), got["x"])
    assert_same(again, CC.host_fit(list(cols.values()), want["x"]), "restart at the result")


@pytest.mark.parametrize("count", [1, 3, 4, 5, 9, 257])
def test_batches_of_partial_and_several_workgroups(device, count):
    cols, x0 = CC.batch(count, seed=count)
    assert_same(device_fit(device, cols, x0, ld=13), CC.host_fit(cols, x0), f"C = {count}")


@pytest.mark.parametrize("name", ["one_row", "rows64", "nan", "inf_angle", "inf", "maxfev", "constant"])
def test_fits_off_the_happy_path(device, name):
    (y, w), x0 = CC.edge_columns()[name]
    got, want = device_fit(device, [(y, w)], x0), CC.host_fit([(y, w)], x0)
    assert_same(got, want, name)
    if name in ("nan", "inf_angle"):
        assert got["status"][0] == CC.PW_NAN and got["nfev"][0] == CC.NAN_NFEV
    if name in ("maxfev", "inf"):
        assert got["status"][0] == CC.PW_MAXFEV and got["nfev"][0] == CC.MAXFEV


def test_outputs_filled_with_garbage_and_no_fits(device):
    """The entry point itself on buffers that hold garbage: every output element of every fit is written, nothing beyond them."""
    cols, x0 = CC.batch(5, seed=77)
    Y, W, n = CC.pack(cols, ld=12)
    Cn = len(cols)
    Yd, Wd, nd, X0 = dev(Y, device), dev(W, device), dev(n, device), dev(x0, device)
    x = torch.full((Cn + 1, 4), float("nan"), dtype=torch.float64, device=device)
    fun = torch.full((Cn + 1,), float("nan"), dtype=torch.float64, device=device)
    ints = [torch.full((Cn + 1,), -12345, dtype=torch.int32, device=device) for _ in range(3)]
    L = _lib.lib()
    stream = torch.cuda.current_stream(device).cuda_stream
    rc = L.nlml_cosine_fit(Yd.data_ptr(), Wd.data_ptr(), 12, nd.data_ptr(), n.ctypes.data, Cn, X0.data_ptr(), 1e-4, 1e-4, x.data_ptr(),
                           fun.data_ptr(), *[t.data_ptr() for t in ints], stream)
    assert rc == 0, L.nlml_last_error()
    got = {"x": x[:Cn].cpu().numpy(), "fun": fun[:Cn].cpu().numpy(), "nfev": ints[0][:Cn].cpu().numpy(), "nit": ints[1][:Cn].cpu().numpy(),
           "status": ints[2][:Cn].cpu().numpy()}
    assert_same(got, CC.host_fit(cols, x0), "garbage-filled outputs")
    assert bool(torch.isnan(x[Cn]).all()) and bool(torch.isnan(fun[Cn])) and all(int(t[Cn]) == -12345 for t in ints)
    # optional outputs left out
    x2 = torch.full((Cn, 4), float("nan"), dtype=torch.float64, device=device)
    assert L.nlml_cosine_fit(Yd.data_ptr(), Wd.data_ptr(), 12, nd.data_ptr(), n.ctypes.data, Cn, X0.data_ptr(), 1e-4, 1e-4, x2.data_ptr(),
                             None, None, None, None, stream) == 0
    assert same_bits(x2.cpu().numpy(), got["x"])
    # no fits: nothing is launched, nothing is written
    assert L.nlml_cosine_fit(Yd.data_ptr(), Wd.data_ptr(), 12, nd.data_ptr(), n.ctypes.data, 0, X0.data_ptr(), 1e-4, 1e-4, x.data_ptr(),
                             fun.data_ptr(), *[t.data_ptr() for t in ints], stream) == 0
    torch.cuda.synchronize(device)
    assert same_bits(x[:Cn].cpu().numpy(), got["x"])
    empty = ops.cosine_fit(Yd[:0], Wd[:0], [], X0[:0])
    assert empty["x"].shape == (0, 4) and empty["status"].shape == (0,)


def test_tolerances_reach_the_kernel(device):
    (y, w), x0 = CC.shipped_columns()["pitch1"], CC.shipped_guess()[4]
    got = device_fit(device, [(y, w)], x0, xtol=1e-2, ftol=1e-3)
    assert_same(got, CC.host_fit([(y, w)], x0, xtol=1e-2, ftol=1e-3), "xtol 1e-2, ftol 1e-3")
    assert got["nfev"][0] < CC.host_fit([(y, w)], x0)["nfev"][0]


def test_compiled_torch_op_gives_the_same_bits(device):
    """torch.ops.nlml_hpe.cosine_fit (csrc/torch_ops.cpp) calls the entry point ops.cosine_fit calls; its Meta kernel gives the shapes."""
    cols, x0 = CC.batch(6, seed=31)
    Y, W, n = CC.pack(cols, ld=12)
    Yd, Wd, X0 = dev(Y, device), dev(W, device), dev(x0, device)
    got = torch.ops.nlml_hpe.cosine_fit(Yd, Wd, n.tolist(), X0)
    want = ops.cosine_fit(Yd, Wd, n.tolist(), X0)
    for g, k in zip(got, CC.OUTPUTS):
        assert g.dtype == want[k].dtype and same_bits(g.cpu().numpy(), want[k].cpu().numpy()), k
    meta = torch.ops.nlml_hpe.cosine_fit(Yd.to("meta"), Wd.to("meta"), n.tolist(), X0.to("meta"))
    assert [tuple(m.shape) for m in meta] == [(6, 4), (6,), (6,), (6,), (6,)]
    with pytest.raises(RuntimeError, match="outside"):
        torch.ops.nlml_hpe.cosine_fit(Yd, Wd, [13] + n.tolist()[1:], X0)


# ---- 3. a fit does not depend on its place in the batch -------------------------------------------------------------------------------
def test_the_same_column_at_positions_0_and_200(device):
    cols, x0 = CC.batch(201, seed=5)
    cols[200], x0[200] = cols[0], x0[0]
    got = device_fit(device, cols, x0)
    for k in CC.OUTPUTS:
        assert same_bits(got[k][0], got[k][200]), k
    assert not same_bits(got["x"][0], got["x"][199])
    alone = device_fit(device, cols[:1], x0[:1])
    assert all(same_bits(alone[k][0], got[k][0]) for k in CC.OUTPUTS), "nor on the size of the batch"


# ---- 4. the chain ---------------------------------------------------------------------------------------------------------------------
def test_from_base_landmarks_to_a_td_inference(device, tmp_path):
    from nlml_hpe_amd import CreateTensor as CT
    from nlml_hpe_amd import TD_Tester
    from nlml_hpe_amd import tucker_decompose as TD
    from nlml_hpe_amd import weights
    shape = (CC.CHAIN_I, 11, 9, 7, 1404)
    X, _ = CT.Compose_Tensor(CC.chain_base(), shape, CC.YAW, CC.PITCH, CC.ROLL)
    assert X.numel() * 4 == 31_135_104
    W, factors, optimized = TD.train_to_npz(X, CC.CHAIN_CONFIG, str(tmp_path), backend="device")
    art = weights.load_tucker_artefacts(str(tmp_path))
    assert art["W"].shape == (5, 3, 3, 3, 1404) and art["W"].dtype == np.float32
    for k, a in enumerate(CC.AXES):
        o = art[f"optimized_{a}"]
        assert o.dtype == np.float64 and o.shape == (3, 4) and np.isfinite(o).all() and same_bits(o, optimized[k])
    idx, deg = CC.chain_cells()
    i, j, k, l = (torch.from_numpy(idx[:, c]).to(device) for c in range(4))
    faces = X[i, j, k, l].contiguous()
    fx = CC.golden()
    ours = TD_Tester.Test_batch(art["W"], faces, 5, art["optimized_yaw"], art["optimized_pitch"], art["optimized_roll"])
    theirs = TD_Tester.Test_batch(art["W"], faces, 5, fx["b_optimized_yaw"], fx["b_optimized_pitch"], fx["b_optimized_roll"])
    e_ours, e_theirs = float(np.abs(ours - deg).mean()), float(np.abs(theirs - deg).mean())
    dist = max(np.abs(art[f"optimized_{a}"] - fx[f"b_optimized_{a}"]).max() for a in CC.AXES)
    print(f"mean absolute pose error over {len(deg)} grid cells: written parameters {e_ours:.6f} deg, the reference's {e_theirs:.6f} deg; "
          f"largest parameter difference {dist:.3e}")
    assert np.isfinite(ours).all() and np.isfinite(theirs).all()
    assert e_ours <= 2 * e_theirs + 0.02, (e_ours, e_theirs)
