"""GPU: K11, the expand-and-compare pass (csrc/tucker_residual.hip), against its host form (nlml_tucker_residual_host, the same header
in plain C++) bit for bit -- X_hat, the two sums and the per-identity residuals -- on the smallest shapes at which the kernel can go
wrong: a short last lane group, one column, one identity, a mode of one bin, the identity ranks 1, 5 and 16, every pose-rank
instance, more column groups and identities than the second launch's first round holds, offsets past 2^31 elements; then the edges
(exact integers, the expand-only form, the torch.ops form, repeatability, a NaN) and the chain through TD_main.main.

The host form itself is held to a model of the stated order and to exact arithmetic in tests/test_tucker_residual_host.py."""
import json

import numpy as np
import pytest
import torch

import tucker_cases as TC
from nlml_hpe_amd import CreateTensor as CT
from nlml_hpe_amd import TD_Tester, TD_main, ops, weights
from nlml_hpe_amd import tucker_decompose as TD

pytestmark = pytest.mark.gpu


def random_model(shape, rank, seed, with_x=True):
    rng = np.random.default_rng(seed)
    W = rng.normal(size=tuple(rank) + (shape[4],)).astype(np.float32)
    U = [rng.normal(size=(n, r)) for n, r in zip(shape[:4], rank)]
    X = rng.normal(size=shape).astype(np.float32) if with_x else None
    return X, W, U


def run_device(X, W, U, device, want_res_id=True, want_xhat=True, op=None):
    d = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=device)
    f = op or ops.tucker_residual
    out = f(d(X, torch.float32), d(W, torch.float32), *[d(u, torch.float64) for u in U], want_res_id, want_xhat)
    return [None if t is None or t.numel() == 0 else t.cpu().numpy() for t in out]


def assert_same(dev, host, what):
    for name, a, b in zip(("sums", "res_id", "xhat"), dev, host):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
            v = np.uint64 if a.dtype == np.float64 else np.uint32
            assert np.array_equal(a.view(v), b.view(v)), (what, name, np.abs(a - b).max())


# M: one column, an odd few, one past a lane group, the prototype's 156 (two full groups and a short one); I = 1; a mode of one bin
# (two here); R = 1, 5, 16; more identities (300 > 256 threads) and groups (4) than the second launch takes in one round
SHAPES = [((4, 3, 2, 5, 1), (5, 3, 2, 3)), ((4, 3, 2, 5, 3), (5, 3, 2, 3)), ((4, 3, 2, 5, 65), (5, 3, 2, 3)), ((4, 3, 2, 5, 156), (5, 3, 2, 3)),
          ((1, 4, 3, 2, 70), (2, 3, 3, 2)), ((5, 1, 3, 1, 40), (3, 1, 2, 1)), ((17, 2, 3, 2, 65), (1, 2, 3, 2)),
          ((17, 2, 3, 2, 65), (16, 2, 3, 2)), ((300, 2, 1, 2, 200), (3, 2, 1, 2)), ((600, 1, 1, 1, 64), (2, 1, 1, 1))]


@pytest.mark.parametrize("shape,rank", SHAPES)
def test_device_is_the_host_form(device, shape, rank):
    X, W, U = random_model(shape, rank, seed=sum(shape) + sum(rank))
    assert_same(run_device(X, W, U, device), TD._residual_host(X, W, U, want_res_id=True, want_xhat=True), (shape, rank))


@pytest.mark.parametrize("ry", [1, 2, 3])
def test_every_pose_rank_instance(device, ry):
    """(12, 5, 4, 3, 130) f32 = 374 KB; the nine (rp, rr) of one ry share a tensor."""
    shape = (12, 5, 4, 3, 130)
    X = np.random.default_rng(40 + ry).normal(size=shape).astype(np.float32)
    for rp in (1, 2, 3):
        for rr in (1, 2, 3):
            _, W, U = random_model(shape, (5, ry, rp, rr), seed=100 * ry + 10 * rp + rr)
            assert_same(run_device(X, W, U, device), TD._residual_host(X, W, U, want_res_id=True, want_xhat=True), (ry, rp, rr))


def test_exact_integers(device):
    shape, rank = (5, 3, 4, 2, 70), (3, 2, 3, 2)
    rng = np.random.default_rng(7)
    W = TC.exact_ints(tuple(rank) + (shape[4],), 7, amax=8)
    U = [rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], size=(n, r)) for n, r in zip(shape[:4], rank)]
    X = TC.exact_ints(shape, 8, amax=64)
    Xh = np.asarray(W, np.float64)
    for m in range(4):
        Xh = TC.expand(Xh, U[m], m)
    E = np.asarray(X, np.float64) - Xh
    sums, res_id, xhat = run_device(X, W, U, device)
    assert np.array_equal(xhat.astype(np.float64), Xh)
    assert sums[0] == np.sum(E * E) and sums[1] == np.sum(np.asarray(X, np.float64) ** 2)
    assert np.array_equal(res_id, np.sum(E * E, axis=(1, 2, 3, 4)))


def test_edges(device):
    shape, rank = (7, 3, 2, 3, 100), (4, 3, 2, 2)
    X, W, U = random_model(shape, rank, seed=3)
    host = TD._residual_host(X, W, U, want_res_id=True, want_xhat=True)
    first = run_device(X, W, U, device)
    assert_same(first, host, "all outputs")
    assert_same(run_device(X, W, U, device), first, "two calls")
    # the outputs that are not asked for change nothing in the others
    sums, res_id, xhat = run_device(X, W, U, device, want_res_id=False, want_xhat=False)
    assert res_id is None and xhat is None
    assert_same([sums, None, None], [host[0], None, None], "sums alone")
    # X == NULL: expand only
    only = run_device(None, W, U, device)
    assert only[0] is None and only[1] is None
    assert_same(only, [None, None, host[2]], "expand only")
    assert_same([None, None, ops.tucker_to_tensor(*[torch.as_tensor(a, device=device) for a in [W] + U]).cpu().numpy()],
                [None, None, host[2]], "ops.tucker_to_tensor")
    # the torch.ops form
    assert_same(run_device(X, W, U, device, op=torch.ops.nlml_hpe.tucker_residual), host, "torch.ops")
    assert_same(run_device(None, W, U, device, op=torch.ops.nlml_hpe.tucker_residual), [None, None, host[2]], "torch.ops, expand only")
    meta = torch.ops.nlml_hpe.tucker_residual(*[torch.empty(a.shape, dtype=torch.float64 if k > 1 else torch.float32, device="meta")
                                                for k, a in enumerate([X, W] + U)], True, True)
    assert [tuple(t.shape) for t in meta] == [(2,), (7,), shape]
    # a NaN in one cell reaches its identity's residual and the totals, nothing else
    Xn = X.copy()
    Xn[4, 1, 0, 2, 77] = np.nan
    sums, res_id, xhat = run_device(Xn, W, U, device)
    assert np.isnan(sums).all() and np.isnan(res_id[4])
    keep = np.arange(7) != 4
    assert np.array_equal(res_id[keep].view(np.uint64), host[1][keep].view(np.uint64))
    assert_same([None, None, xhat], [None, None, host[2]], "X_hat does not read X")
    # refusals of the wrapper: a wrong shape never reaches the kernel
    dU = [torch.as_tensor(u, device=device) for u in U]
    dW, dX = torch.as_tensor(W, device=device), torch.as_tensor(X, device=device)
    with pytest.raises(ValueError):
        ops.tucker_residual(dX[:, :2], dW, *dU)
    with pytest.raises(ValueError):
        ops.tucker_residual(dX, dW[:, :2], *dU)
    with pytest.raises(TypeError):
        ops.tucker_residual(dX, dW, dU[0].float(), *dU[1:])
    with pytest.raises(RuntimeError):
        torch.ops.nlml_hpe.tucker_residual(dX[:, :2], dW, *dU, False, False)


def model_totals(res_id):
    """The second launch's order from the per-identity sums: thread t adds its identities t, t + 256, .. from 0.0, then the halving
    tree over the 256 threads."""
    tot = np.zeros(256)
    for i, r in enumerate(res_id):
        tot[i % 256] = tot[i % 256] + r
    h = 128
    while h >= 1:
        tot[:h] = tot[:h] + tot[h:2 * h]
        h //= 2
    return tot[0]


def test_offsets_beyond_2_31_elements(device):
    """(2210, 11, 9, 7, 1404) f32 = 2,150,268,120 elements (8.6 GB): identity 2207 of the reference's grid straddles element 2^31 and
    2209 lies wholly past it; X_hat is asked for, so reads and writes both cross it.  Identities 0, 1103, 2207 and 2209 are compared
    with the host form on their own slices -- res_id[i] and X_hat[i] depend on identity i alone -- and
    sums[0] with the second launch's order applied to the device's res_id."""
    I = 2210
    base = np.random.default_rng(12).normal(size=(I, 468, 3)).astype(np.float32)
    X, _ = CT.Compose_Tensor(base, (I, 11, 9, 7, 1404), TC.YAW, TC.PITCH, TC.ROLL)
    assert X.numel() > 2 ** 31
    _, W, U = random_model((I, 11, 9, 7, 1404), (5, 3, 3, 3), seed=9, with_x=False)
    dW = torch.as_tensor(W, device=device)
    dU = [torch.as_tensor(u, device=device) for u in U]
    sums, res_id, xhat = ops.tucker_residual(X, dW, *dU, want_res_id=True, want_xhat=True)
    res_id = res_id.cpu().numpy()
    ids = [0, 1103, 2207, 2209]
    assert 2207 * 693 * 1404 < 2 ** 31 < 2208 * 693 * 1404 < 2209 * 693 * 1404
    Xs = X[ids].cpu().numpy()
    hs, hres, hx = TD._residual_host(Xs, W, [U[0][ids]] + U[1:], want_res_id=True, want_xhat=True)
    assert np.array_equal(res_id[ids].view(np.uint64), hres.view(np.uint64))
    assert np.array_equal(xhat[ids].cpu().numpy().view(np.uint32), hx.view(np.uint32))
    assert sums[0].item() == model_totals(res_id)
    # sum X^2 has no per-identity output; against a zero model X_hat is +0.0 and e = x, so that call's res_id holds each identity's q
    zsums, q_id, _ = ops.tucker_residual(X, torch.zeros_like(dW), *dU, want_res_id=True)
    q_id = q_id.cpu().numpy()
    hq = TD._residual_host(Xs, np.zeros_like(W), [U[0][ids]] + U[1:], want_res_id=True)[1]
    assert np.array_equal(q_id[ids].view(np.uint64), hq.view(np.uint64))
    assert zsums[0].item() == zsums[1].item() == sums[1].item() == model_totals(q_id)
    del X, xhat
    torch.cuda.empty_cache()


# ---- the chain -------------------------------------------------------------------------------------------------------------------
def chain(tmp):
    base = TC.base_landmarks(8, 468, seed=13)
    np.save(f"{tmp}/base8.npy", base)
    report = TD_main.main(["--base-landmarks", f"{tmp}/base8.npy", "--identities-from-file", "--out-dir", f"{tmp}/out", "--perform_validation",
                           "tr", "--val-base-landmarks", f"{tmp}/base8.npy", "--seed", "5"])
    return base, report


def test_chain_through_td_main(device, tmp_path_factory, capsys):
    """8 synthetic identities at the reference's bins through TD_main.main with validation on the same identities: pins the plumbing
    (no accuracy threshold)."""
    tmp = str(tmp_path_factory.mktemp("td_chain"))
    base, report = chain(tmp)
    out = capsys.readouterr().out
    for line in ("Reconstruction Error: ", "Shape of W: (5, 3, 3, 3, 1404)", "MAE (Yaw): ", "MAE (Pitch): ", "MAE (Roll): ", "Total MAE: "):
        assert line in out, line
    art = weights.load_tucker_artefacts(f"{tmp}/out")
    assert art["W"].shape == (5, 3, 3, 3, 1404) and art["U_id"].shape == (8, 5) and art["optimized_yaw"].shape == (3, 4)
    assert json.load(open(f"{tmp}/out/{TD_main.REPORT_NAME}")) == json.loads(json.dumps(report))
    assert report["tensor_shape"] == [8, 11, 9, 7, 1404] and len(report["sweep_errors"]) >= 1 and len(report["worst_identities"]) == 5
    # the error of the artefacts as written, on the device and on the host
    X, _ = CT.Compose_Tensor(base, (8, 11, 9, 7, 1404), TC.YAW, TC.PITCH, TC.ROLL)
    factors = [art[k] for k in ("U_id", "U_yaw", "U_pitch", "U_roll")]
    err, res_id = TD.reconstruction_error(X, art["W"], factors, backend="device", per_identity=True)
    assert report["reconstruction_error"] == err
    assert err == TD.reconstruction_error(X.cpu().numpy(), art["W"], factors, backend="numpy")
    assert [w["identity"] for w in report["worst_identities"]] == list(np.argsort(-res_id, kind="stable")[:5])
    assert 0 < err < 0.1, "a rotation tensor of 8 identities at rank 5 is fitted to a few percent"
    # the validation: the same picks, the same landmarks, the same estimator
    v = report["validation"]
    bins = [TC.YAW, TC.PITCH, TC.ROLL]
    picks = TD_main.validation_picks(8, bins, 5)
    assert v["picks"] == picks.tolist() and v["seed"] == 5
    assert v["true_deg"] == [[float(b[k]) for b, k in zip(bins, row)] for row in picks]
    x = X[torch.arange(8), picks[:, 0], picks[:, 1], picks[:, 2]]
    mine = TD_main.validation_landmarks(base, picks, bins)
    rotated = [k for k in range(8) if tuple(v["true_deg"][k]) != (0.0, 0.0, 0.0)]
    assert torch.equal(mine[rotated], x[rotated]), "the per-face call gives the grid's cell (the all-zero cell is copied, not rotated)"
    deg = TD_Tester.Test_batch(art["W"], mine, 5, art["optimized_yaw"][0:3], art["optimized_pitch"][0:3], art["optimized_roll"][0:3])
    assert v["pred_deg"] == np.round(deg, 3).tolist()
    mae = np.mean(np.abs(np.array(v["true_deg"]) - np.array(v["pred_deg"])), axis=0)
    assert [v["mae_yaw"], v["mae_pitch"], v["mae_roll"]] == mae.tolist() and v["mae_total"] == float((mae[0] + mae[1] + mae[2]) / 3)
