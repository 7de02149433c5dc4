"""CPU: the host forms of the encoder-training entry points (nlml_encoder_train_steps_host, nlml_encoder_eval_losses_host:
csrc/encoder_train_ref.h in plain C++), the argument contract of all four forms, and the stand-alone sanitizer program.

The accuracy tests hold the host form to the claim of tests/encoder_train_cases.py (4 x torch-f32's distance from the float64
autograd result, floor 4 x 2^-24) on the cases the GPU tests run on the device.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import encoder_train_cases as EC
from nlml_hpe_amd import _lib

BADARG = -1
FAKE = 0x1000            # a non-null, 16-byte aligned address no refused call may touch


def _err():
    return (_lib.lib().nlml_last_error() or b"").decode()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- accuracy -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 31, 32, 33, 256])
@pytest.mark.parametrize("F", [136, 1404])
def test_single_step(F, B):
    cs = EC.case(F, B)
    exact, t32 = EC.yardsticks(F, B, B)
    got = EC.host_train(cs, None, B)
    assert got["status"] == 0
    EC.check_claim(got, exact, t32, f"host F={F} B={B}")


@pytest.mark.parametrize("max_norm, clipped", [(0.1, True), (20.0, False)])
def test_clip(max_norm, clipped):
    F, B = 136, 33
    cs = EC.case(F, B)
    exact, t32 = EC.yardsticks(F, B, B, hyper=(("max_norm", max_norm),))
    assert (exact["norm"][0] > max_norm) == clipped
    got = EC.host_train(cs, None, B, max_norm=max_norm)
    EC.check_claim(got, exact, t32, f"host clip max_norm={max_norm}")


@pytest.mark.parametrize("zero_grad", [False, True])
def test_two_steps_on_one_batch(zero_grad):
    F, B = 136, 33
    hyper = (("max_norm", 0.3), ("zero_grad", zero_grad), ("lr", 1e-3))
    cs, _, exact, t32 = EC.settled(F, B, B, (tuple(range(B)),) * 2, hyper=hyper)
    order = tuple(range(B)) * 2
    assert exact["norm"][0] > 0.3 and exact["norm"][1] > 0.3, "both clip coefficients are below 1"
    got = EC.host_train(cs, order, B, **dict(hyper))
    assert got["loss"].shape == (2,)
    EC.check_claim(got, exact, t32, f"host two steps zero_grad={zero_grad}")
    other = EC.torch_loop(cs, torch.float64, [np.arange(B)] * 2, max_norm=0.3, zero_grad=not zero_grad, lr=1e-3)
    # both accumulators end on the clip sphere in nearly one direction (one batch twice), so the rule shows in the second step's norm
    # BEFORE clipping: about |c1 g1 + g2| = 0.8 against |g2| = 0.5
    assert abs(got["norm"][1] - other["norm"][1]) > 0.2 * other["norm"][1], "the two rules give different second norms"


def test_weight_decay_changes_p_and_not_g():
    F, B = 136, 33
    cs = EC.case(F, B)
    a = EC.host_train(cs, None, B, weight_decay=0.0)
    b = EC.host_train(cs, None, B, weight_decay=1e-2)
    assert np.array_equal(_bits(a["flat"][1]), _bits(b["flat"][1]))
    assert not np.array_equal(_bits(a["flat"][0]), _bits(b["flat"][0]))
    exact, t32 = EC.yardsticks(F, B, B, hyper=(("weight_decay", 1e-2),))
    EC.check_claim(b, exact, t32, "host weight_decay=1e-2")


def test_twenty_steps_over_ten_epochs():
    F, N, batch, epochs = 136, 300, 256, 10
    cs, orders = EC.case(F, N), EC.epoch_orders(N, epochs)
    exact, t32 = EC.yardsticks(F, N, batch, hyper=(("lr", 1e-3),), order=tuple(tuple(int(v) for v in o) for o in orders), check_margin="first")
    p, g = cs["params"].copy(), np.zeros_like(cs["params"])
    losses, norms = [], []
    for o in orders:
        got = EC.host_train(cs, o, batch, params=p, grads=g, lr=1e-3)
        assert got["loss"].shape == (2,) and got["status"] == 0
        losses.append(got["loss"])
        norms.append(got["norm"])
    got["loss"], got["norm"] = np.concatenate(losses), np.concatenate(norms)
    EC.check_claim(got, exact, t32, "host twenty steps", parts=("loss", "params"))   # why not the gradients: encoder_train_cases.py


def test_gather_padding_and_validation():
    F, N = 136, 300
    cs = EC.case(F, N)
    order = np.array([5, 3, 9, 250, 0, 299, 17, 3, 64, 128, 31, 32, 33, 1, 2, 7], np.int32)
    a = EC.host_train(cs, order, 16)
    packed = dict(cs, x=np.ascontiguousarray(cs["x"][order]), labels=np.ascontiguousarray(cs["labels"][order]))
    b = EC.host_train(packed, None, 16)
    wide = np.full((len(order), F + 3), np.nan, np.float32)
    wide[:, :F] = packed["x"]
    c = EC.host_train(packed, None, 16, x=wide[:, :F])
    for other in (b, c):
        assert np.array_equal(_bits(a["loss"]), _bits(other["loss"])) and all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a["flat"], other["flat"]))
    ev, status = EC.host_eval(cs, None, 256)
    tr = EC.host_train(cs, None, 256, lr=0.0, weight_decay=0.0)
    assert status == 0 and ev.shape == (2,) and np.array_equal(_bits(ev), _bits(tr["loss"]))


def test_out_of_range_entries_are_clamped_and_flagged():
    F, N = 136, 40
    cs = EC.case(F, N)
    order = np.arange(N, dtype=np.int32)
    bad = order.copy()
    bad[3], bad[37] = -5, N + 1000
    good = order.copy()
    good[3], good[37] = 0, N - 1
    a, b = EC.host_train(cs, bad, 32), EC.host_train(cs, good, 32)
    assert a["status"] == _lib.ENCODER_TRAIN_CLAMPED_ORDER and b["status"] == 0
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a["flat"], b["flat"]))
    lab = cs["labels"].copy()
    lab[35, 0], lab[2, 2] = 99, -1
    lab2 = cs["labels"].copy()
    lab2[35, 0], lab2[2, 2] = cs["tables"][0].shape[0] - 1, 0
    c, d = EC.host_train(cs, bad, 32, labels=lab), EC.host_train(cs, good, 32, labels=lab2)
    assert c["status"] == (_lib.ENCODER_TRAIN_CLAMPED_ORDER | _lib.ENCODER_TRAIN_CLAMPED_LABEL)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(c["flat"], d["flat"]))
    ev, status = EC.host_eval(dict(cs, labels=lab), None, 32)
    assert status == _lib.ENCODER_TRAIN_CLAMPED_LABEL and np.isfinite(ev).all()


# ---- the argument contract: every refusal, in the header's order, before any GPU call ----------------------------------------------
def _call(form, **over):
    """One of the four entry points on FAKE buffers with one argument set replaced; no refused call touches a buffer."""
    a = dict(x=FAKE, ldx=1404, N=10, labels=FAKE, ld_lab=3, t_yaw=FAKE, n_yaw=11, t_pitch=FAKE, n_pitch=9, t_roll=FAKE, n_roll=7, params=FAKE,
             grads=FAKE, F=1404, batch=256, order=FAKE, n=10, lr=1e-4, wd=1e-5, max_norm=20.0, zero_grad=0, loss=FAKE, norm=FAKE, status=FAKE,
             ws=FAKE, ws_bytes=1 << 30)
    a.update(over)
    L = _lib.lib()
    data = [a["x"], a["ldx"], a["N"], a["labels"], a["ld_lab"], a["t_yaw"], a["n_yaw"], a["t_pitch"], a["n_pitch"], a["t_roll"], a["n_roll"]]
    run = [a["F"], a["batch"], a["order"], a["n"]]
    hyper = [a["lr"], a["wd"], a["max_norm"], a["zero_grad"]]
    if form == "train":
        return L.nlml_encoder_train_steps(*data, a["params"], a["grads"], *run, *hyper, a["loss"], a["norm"], a["status"], a["ws"], a["ws_bytes"], None)
    if form == "eval":
        return L.nlml_encoder_eval_losses(*data, a["params"], *run, a["loss"], a["status"], a["ws"], a["ws_bytes"], None)
    if form == "train_host":
        return L.nlml_encoder_train_steps_host(*data, a["params"], a["grads"], *run, *hyper, a["loss"], a["norm"], a["status"])
    return L.nlml_encoder_eval_losses_host(*data, a["params"], *run, a["loss"], a["status"])


FORMS = ("train", "eval", "train_host", "eval_host")
# (the bad argument, a word of its message), in the documented order; each case also carries EVERY LATER case's bad argument, so the
# message shows which check came first
REFUSALS = [(dict(F=137), "F = 137"), (dict(batch=257), "batch"), (dict(n=-1), "negative n"), (dict(x=None), "null buffer"),
            (dict(N=0), "N = 0"), (dict(ld_lab=2), "ld_lab"), (dict(n_pitch=0), "table 1"), (dict(ldx=1403), "ldx"),
            (dict(N=2 ** 31 - 1, ldx=2 ** 40), "64-bit")]
TRAIN_ONLY = [(dict(lr=float("nan")), "finite")]
DEVICE_ONLY = [(dict(ws_bytes=64), "workspace of 64 bytes"), (dict(params=FAKE + 4), "16-byte"), (dict(loss=FAKE + 2), "4-byte")]


@pytest.mark.parametrize("form", FORMS)
def test_refusals_in_the_documented_order(form):
    chain = list(REFUSALS) + (TRAIN_ONLY if form.startswith("train") else []) + (DEVICE_ONLY if not form.endswith("host") else [])
    for k, (bad, word) in enumerate(chain):
        over = {}
        for later, _ in reversed(chain[k:]):   # the case's own argument last: it wins where two cases use one argument
            over.update(later)
        assert _call(form, **over) == BADARG, (form, bad)
        assert word in _err(), f"{form} with {over}: expected the refusal about {word!r} first, got {_err()!r}"


@pytest.mark.parametrize("form", FORMS)
def test_batch_bounds_and_empty_call(form):
    assert _call(form, batch=0) == BADARG and "batch" in _err()
    assert _call(form, F=136, ldx=136, n=0, x=None, params=None, ws=None, ws_bytes=0) == 0, "n == 0 returns at once, whatever else is passed"
    assert _call(form, n=0, N=-3, ldx=0) == 0


def test_workspace_bytes():
    L = _lib.lib()
    assert L.nlml_encoder_train_workspace_bytes(100, 256) == 0 and L.nlml_encoder_train_workspace_bytes(1404, 0) == 0
    assert L.nlml_encoder_train_workspace_bytes(1404, 257) == 0
    small, big = L.nlml_encoder_train_workspace_bytes(1404, 1), L.nlml_encoder_train_workspace_bytes(1404, 256)
    assert 0 < small < big <= 8 << 20
    assert _call("train", ws_bytes=big - 1) == BADARG and "workspace" in _err(), "one byte short is refused"


# ---- the stand-alone program under AddressSanitizer + UBSan ------------------------------------------------------------------------------
def test_host_form_under_asan_ubsan(tmp_path, repo_root):
    exe = tmp_path / "encoder_train_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(exe),
           os.path.join(repo_root, "tools", "encoder_train_host.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "encoder train host ok" in res.stdout
    assert "heads train host ok" in res.stdout, "the K10 case (two networks in an exact-size workspace) runs the shared host functions too"


# ---- the trainer on the host backend -------------------------------------------------------------------------------------------------
def _small_sets():
    cs = EC.case(136, 300)
    return (cs["x"][:200], cs["labels"][:200]), (cs["x"][200:], cs["labels"][200:]), dict(zip(("U_yaw", "U_pitch", "U_roll"), cs["tables"]))


def test_trainer_on_the_host_backend(tmp_path):
    """Two epochs of 200 rows in batches of 128 (a partial second batch), StepLR after the first epoch, the snapshot of the best
    validation total written under the reference's keys and read back by the unchanged loader."""
    from nlml_hpe_amd import EncoderTrainer as ET
    from nlml_hpe_amd import weights
    train, val, factors = _small_sets()
    out = tmp_path / "models" / "Encoder.pth"
    best, hist = ET.train_encoder(train, val, factors, batch_size=128, num_epochs=2, learning_rate=0.05, scheduler_step_size=1, seed=3,
                                  backend="host", config=None, out_path=str(out), verbose=False)
    assert hist["lr"] == [0.05, 0.05 * 0.9] and [len(s) for s in hist["step_loss"]] == [2, 2]
    assert hist["best_epoch"] == int(np.argmin(hist["val_total"])) + 1 == 2 and hist["train_loss"][1] < hist["train_loss"][0]
    sd = weights.load_encoder_state_dict(str(tmp_path / "models"))
    assert list(sd) == EC.KEYS and all(np.array_equal(_bits(sd[k].numpy()), _bits(best[k])) for k in EC.KEYS)
    # the same run by hand: the initial weights, the orders and the rates are the module's own functions
    p, g = ET.flatten_state_dict(ET.initial_state_dict(136, 3)), None
    g = np.zeros_like(p)
    cs = dict(EC.case(136, 300), x=np.ascontiguousarray(train[0]), labels=np.ascontiguousarray(train[1]))
    for epoch, order in enumerate(ET.epoch_orders(200, 2, 3)):
        got = EC.host_train(cs, order, 128, params=p, grads=g, lr=ET.learning_rate_of_epoch(0.05, epoch, 1))
        assert np.array_equal(_bits(got["loss"]), _bits(hist["step_loss"][epoch]))
    assert np.array_equal(_bits(p), _bits(ET.flatten_state_dict(best)))


def test_trainer_reads_the_reference_dataset_files_and_raises_on_bad_input(tmp_path):
    import torch
    from nlml_hpe_amd import EncoderTrainer as ET
    train, val, factors = _small_sets()
    for name, (x, lab) in (("train", train), ("val", val)):
        torch.save((torch.from_numpy(x), torch.from_numpy(lab.astype(np.int64))), tmp_path / f"{name}_dataset.pth")
    kw = dict(batch_size=256, num_epochs=1, seed=1, backend="host", config=None, out_path=None, verbose=False)
    a, _ = ET.train_encoder(str(tmp_path / "train_dataset.pth"), str(tmp_path / "val_dataset.pth"), factors, **kw)
    b, _ = ET.train_encoder(train, val, factors, **kw)
    assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in EC.KEYS)
    bad = train[1].copy()
    bad[5, 1] = 40
    with pytest.raises(ValueError, match="outside its range"):
        ET.train_encoder((train[0], bad), val, factors, **kw)
    with pytest.raises(FloatingPointError, match="step 0"):
        ET.train_encoder(train, val, factors, **dict(kw, learning_rate=1e30, num_epochs=2))   # the first update overflows
    x, lab = ET.tensor_rows(np.zeros((2, 3, 2, 2, 136), np.float32))
    assert x.shape == (24, 136) and lab[13].tolist() == [0, 0, 1, 1] and lab[23].tolist() == [2, 1, 1, 1]
