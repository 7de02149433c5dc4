"""GPU: the encoder-training kernels (K9, csrc/encoder_train.hip) through ops.encoder_train_steps / ops.encoder_eval_losses,
torch.ops.nlml_hpe.encoder_train_steps and EncoderTrainer.train_encoder.

Every accuracy test holds the device to tests/encoder_train_cases.py's claim: for the loss, the norm, each of the twelve gradient
tensors and each updated parameter tensor, the relative Frobenius distance from the float64 autograd result is at most 4 x torch-f32's
(floor 4 x 2^-24).  The workspace is pre-filled with NaN, so a padding row or column that leaked would show.  The measured ratios
are in profiles/encoder_train.md.
"""
import os

import numpy as np
import pytest
import torch

import encoder_train_cases as EC
from nlml_hpe_amd import _lib

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("loss", "norm")) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a["flat"], b["flat"]))


# ---- single steps: every F, batches below / at / above a tile and the full batch ----------------------------------------------------
@pytest.mark.parametrize("B", [1, 31, 32, 33, 256])
@pytest.mark.parametrize("F", [136, 1404])
def test_single_step(device, F, B):
    cs = EC.case(F, B)
    exact, t32 = EC.yardsticks(F, B, B)
    got = EC.device_train(cs, device, None, B)
    assert got["status"] == 0
    assert all(np.isfinite(v).all() for v in got["flat"]), "a NaN of the workspace leaked into the result"
    EC.check_claim(got, exact, t32, f"device F={F} B={B}")


# ---- clip ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm, clipped", [(0.1, True), (20.0, False)])
def test_clip(device, max_norm, clipped):
    F, B = 136, 33
    cs = EC.case(F, B)
    exact, t32 = EC.yardsticks(F, B, B, hyper=(("max_norm", max_norm),))
    assert (exact["norm"][0] > max_norm) == clipped
    got = EC.device_train(cs, device, None, B, max_norm=max_norm)
    EC.check_claim(got, exact, t32, f"device clip max_norm={max_norm}")
    gnorm = np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in got["grads"].values()))
    want = min(1.0, max_norm / (float(exact["norm"][0]) + 1e-6)) * float(exact["norm"][0])
    assert abs(gnorm - want) <= 1e-5 * want, "the accumulator holds the clipped gradient"


# ---- accumulation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_grad", [False, True])
def test_two_steps_on_one_batch(device, zero_grad):
    """Without zero_grad G after the second step is c2 (c1 g1 + g2) -- the reference's loop; with it, c2 g2.  max_norm 0.3 makes both
    coefficients matter (the norms are about 0.5 and 1)."""
    F, B = 136, 33
    hyper = (("max_norm", 0.3), ("zero_grad", zero_grad), ("lr", 1e-3))
    cs, _, exact, t32 = EC.settled(F, B, B, (tuple(range(B)),) * 2, hyper=hyper)
    order = tuple(range(B)) * 2
    got = EC.device_train(cs, device, order, B, **dict(hyper))
    assert got["loss"].shape == (2,)
    EC.check_claim(got, exact, t32, f"device two steps zero_grad={zero_grad}")
    other = EC.torch_loop(cs, torch.float64, [np.arange(B)] * 2, max_norm=0.3, zero_grad=not zero_grad, lr=1e-3)
    # both accumulators end on the clip sphere in nearly one direction (one batch twice), so the rule shows in the second step's norm
    # BEFORE clipping: about |c1 g1 + g2| = 0.8 against |g2| = 0.5
    assert abs(got["norm"][1] - other["norm"][1]) > 0.2 * other["norm"][1], "the two rules give different second norms"


def test_weight_decay_changes_p_and_not_g(device):
    F, B = 136, 33
    cs = EC.case(F, B)
    a = EC.device_train(cs, device, None, B, weight_decay=0.0)
    b = EC.device_train(cs, device, None, B, weight_decay=1e-2)
    assert np.array_equal(_bits(a["flat"][1]), _bits(b["flat"][1]))
    assert not np.array_equal(_bits(a["flat"][0]), _bits(b["flat"][0]))
    exact, t32 = EC.yardsticks(F, B, B, hyper=(("weight_decay", 1e-2),))
    EC.check_claim(b, exact, t32, "device weight_decay=1e-2")


# ---- an epoch with a partial last batch; twenty steps -------------------------------------------------------------------------------
def test_twenty_steps_over_ten_epochs(device):
    F, N, batch, epochs = 136, 300, 256, 10
    cs, orders = EC.case(F, N), EC.epoch_orders(N, epochs)
    exact, t32 = EC.yardsticks(F, N, batch, hyper=(("lr", 1e-3),), order=tuple(tuple(int(v) for v in o) for o in orders), check_margin="first")
    p = torch.from_numpy(cs["params"]).to(device)
    g = torch.zeros_like(p)
    losses, norms = [], []
    for o in orders:
        got = EC.device_train(cs, device, o, batch, params=p, grads=g, lr=1e-3)
        assert got["loss"].shape == (2,) and got["status"] == 0
        losses.append(got["loss"])
        norms.append(got["norm"])
    got["loss"], got["norm"] = np.concatenate(losses), np.concatenate(norms)
    assert got["loss"].shape == (20,)
    EC.check_claim(got, exact, t32, "device twenty steps", parts=("loss", "params"))   # why not the gradients: encoder_train_cases.py


# ---- bit for bit, device against device -----------------------------------------------------------------------------------------------
def test_same_call_twice_same_bits(device):
    cs = EC.case(1404, 33)
    assert _same(EC.device_train(cs, device, None, 33), EC.device_train(cs, device, None, 33, nan_workspace=False))


def test_gathered_rows_equal_contiguous_rows(device):
    F, N = 136, 300
    cs = EC.case(F, N)
    order = np.array([5, 3, 9, 250, 0, 299, 17, 3, 64, 128, 31, 32, 33, 1, 2, 7, 11, 13, 200, 100, 50, 25, 12, 6, 3, 299, 298, 297, 150, 151, 152, 153,
                      154, 155, 42], np.int32)
    a = EC.device_train(cs, device, order, 35)
    packed = dict(cs, x=np.ascontiguousarray(cs["x"][order]), labels=np.ascontiguousarray(cs["labels"][order]), N=len(order))
    b = EC.device_train(packed, device, None, 35)
    assert _same(a, b)


def test_padded_row_stride_equals_tight(device):
    F, B = 1404, 33
    cs = EC.case(F, B)
    for pad in (1, 4):   # 1: rows lose their 16-byte alignment (scalar loads); 4: they keep it
        wide = torch.full((B, F + pad), float("nan"), dtype=torch.float32, device=device)
        wide[:, :F] = torch.from_numpy(cs["x"]).to(device)
        assert _same(EC.device_train(cs, device, None, B), EC.device_train(cs, device, None, B, x=wide[:, :F]))


def test_torch_op_equals_ctypes(device):
    F, N, batch = 136, 300, 256
    cs = EC.case(F, N)
    order = EC.epoch_orders(N, 1)[0]
    a = EC.device_train(cs, device, order, batch, lr=1e-3, max_norm=0.3)
    x, lab, tabs = EC.device_inputs(cs, device)
    p = torch.from_numpy(cs["params"]).to(device)
    g = torch.zeros_like(p)
    loss, norm, status = torch.ops.nlml_hpe.encoder_train_steps(x, lab, tabs[0], tabs[1], tabs[2], p, g, torch.from_numpy(order).to(device), N,
                                                                batch, 1e-3, 1e-5, 0.3, False)
    b = {"loss": loss.cpu().numpy(), "norm": norm.cpu().numpy(), "flat": (p.cpu().numpy(), g.cpu().numpy())}
    assert int(status.cpu()[0]) == 0 and _same(a, b)


def test_validation_losses_equal_the_training_forward(device):
    from nlml_hpe_amd import ops
    F, N, batch = 136, 300, 256
    cs = EC.case(F, N)
    x, lab, tabs = EC.device_inputs(cs, device)
    p = torch.from_numpy(cs["params"]).to(device)
    ev, status = ops.encoder_eval_losses(x, lab, tabs, p, batch=batch)
    assert ev.shape == (2,) and int(status.cpu()[0]) == 0
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(cs["params"])), "the validation pass leaves the parameters alone"
    # lr = 0 and no decay: the parameters stay, so both training steps run their forward on them
    tr = EC.device_train(cs, device, None, batch, lr=0.0, weight_decay=0.0)
    assert np.array_equal(_bits(ev.cpu().numpy()), _bits(tr["loss"]))
    want, _ = EC.host_eval(cs, None, batch)
    assert np.allclose(ev.cpu().numpy(), want, rtol=1e-5)


def test_out_of_range_entries_are_clamped_and_flagged(device):
    F, N = 136, 40
    cs = EC.case(F, N)
    order = np.arange(N, dtype=np.int32)
    bad_order = order.copy()
    bad_order[3], bad_order[7] = -5, N + 1000
    a = EC.device_train(cs, device, bad_order, 32)
    clamped = order.copy()
    clamped[3], clamped[7] = 0, N - 1
    b = EC.device_train(cs, device, clamped, 32)
    assert a["status"] == _lib.ENCODER_TRAIN_CLAMPED_ORDER and b["status"] == 0 and _same(a, b)
    lab = cs["labels"].copy()
    lab[35, 0], lab[2, 2] = 99, -1
    c = EC.device_train(dict(cs, labels=lab), device, None, 32)
    lab2 = cs["labels"].copy()
    lab2[35, 0], lab2[2, 2] = cs["tables"][0].shape[0] - 1, 0
    d = EC.device_train(dict(cs, labels=lab2), device, None, 32)
    assert c["status"] == _lib.ENCODER_TRAIN_CLAMPED_LABEL and _same(c, d)


# ---- the chain: base landmarks -> K6 -> K7 / K8 -> K9 -> Encoder.pth -> the packed K2 model -------------------------------------------
def test_from_base_landmarks_to_a_runnable_model(device, tmp_path, monkeypatch, repo_root):
    """Eight synthetic identities, six for training and two for validation, on a 5 x 3 x 3 grid of bins (270 training rows: batches of
    256 and 14, three epochs, lr 0.1).  The settings were chosen with the float64 replica: its epoch means fall 0.848 -> 0.593, and
    its closest ReLU pre-activation stays 0.19 of relu_margin's sixteen deviations from zero, about three deviations (asserted below
    at 0.1), so no mask can flip legitimately and the final parameters can be held to the 4x rule."""
    import shutil

    import cosine_fit_cases as CC
    import NLML_HPE_Model_Builder as MB
    from nlml_hpe_amd import CreateTensor as CT
    from nlml_hpe_amd import EncoderTrainer as ET
    from nlml_hpe_amd import tucker_decompose as TD
    from nlml_hpe_amd import weights
    from nlml_hpe_amd.model import load_model

    yaw, pitch, roll = np.arange(-20, 21, 10), np.arange(-10, 11, 10), np.arange(-10, 11, 10)
    config = {"tensor_decom_ranks": {"R_identity": 5, "R_yaw": 3, "R_pitch": 3, "R_roll": 3, "R_features": 1404},
              "yaw_bins": {"min_bin": -20, "max_bin": 21, "interval": 10}, "pitch_bins": {"min_bin": -10, "max_bin": 11, "interval": 10},
              "roll_bins": {"min_bin": -10, "max_bin": 11, "interval": 10}}
    base = CC.chain_base()
    X, _ = CT.Compose_Tensor(base[:6], (6, 5, 3, 3, 1404), yaw, pitch, roll)
    Xv, _ = CT.Compose_Tensor(base[6:], (2, 5, 3, 3, 1404), yaw, pitch, roll)
    features = tmp_path / "outputs" / "features"
    TD.train_to_npz(X, config, str(features), backend="device")
    hyper = dict(num_epochs=3, learning_rate=0.1, seed=0, config=None, verbose=False)
    out = tmp_path / "models" / "Encoder.pth"
    best, hist = ET.train_encoder(X, Xv, str(features / "Factor_Matrices.npz"), out_path=str(out), **hyper)
    assert [len(s) for s in hist["step_loss"]] == [2, 2, 2] and np.isfinite(hist["val_loss"]).all()
    assert hist["train_loss"][-1] < hist["train_loss"][0], "the last epoch's mean training loss is below the first's"

    # the written file through the unchanged loaders, the model builder without synthetic weights, and a forward
    for name in weights.HEAD_NAMES:
        shutil.copy(os.path.join(repo_root, "models", f"{name}_network.pth"), tmp_path / "models")
    shutil.copytree(os.path.join(repo_root, "configs"), tmp_path / "configs")
    enc = weights.load_encoder_state_dict(str(tmp_path / "models"))
    heads = weights.load_head_state_dicts(str(tmp_path / "models"))
    assert weights.validate_shapes(enc, heads) == 1404 and weights.pack_blob(enc, heads).size > 0
    assert all(np.array_equal(_bits(enc[k].numpy()), _bits(best[k])) for k in EC.KEYS)
    monkeypatch.chdir(tmp_path)
    packed = MB.model_builder([])
    assert os.path.getsize(packed) > 0
    pose = load_model("models", device).from_landmarks(torch.from_numpy(np.ascontiguousarray(base)).to(device))
    assert pose.shape == (8, 3) and bool(torch.isfinite(pose).all())

    # the same run on the host form, and both against the reference's loop in float64 and float32
    host, hist_h = ET.train_encoder(X, Xv, str(features / "Factor_Matrices.npz"), out_path=None, backend="host", **hyper)
    assert hist_h["best_epoch"] == hist["best_epoch"]
    x, lab = ET.tensor_rows(X.cpu().numpy())
    cs = {"x": x, "labels": lab, "tables": ET._tables(str(features / "Factor_Matrices.npz")), "sd": ET.initial_state_dict(1404, 0)}
    b = [piece for o in ET.epoch_orders(x.shape[0], 3, 0) for piece in EC.batches_of(o, 256)]
    close = set()
    exact = EC.torch_loop(cs, torch.float64, b, lr=0.1, check_margin=True, violators=close, margin_floor=0.1)
    assert not close, "a ReLU pre-activation of the float64 run within 1.6 deviations of zero"
    t32 = EC.torch_loop(cs, torch.float32, b, lr=0.1)
    assert (exact["loss"][4] + exact["loss"][5]) < 0.8 * (exact["loss"][0] + exact["loss"][1]), "the replica's margin"
    for who, sd, h in (("device", best, hist), ("host", host, hist_h)):
        assert h["best_epoch"] == 3
        got = {"loss": np.concatenate(h["step_loss"]), "params": sd}
        EC.check_claim(got, exact, t32, f"chain {who}", parts=("loss", "params"))
