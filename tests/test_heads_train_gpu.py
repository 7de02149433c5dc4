"""K10 on the device (csrc/heads_train.hip): every word of a step against the host form (csrc/heads_train_ref.h, which the CPU tests
hold to the C oracle's GEMM order, to a numpy model of the other orders and to torch) and against the oracle on the device's own
inputs to each launch; the independence of the networks that share the launches; the step count carried across calls; the
evaluation pass, the clamped orders, the torch op; and the chain Trained_data.npz -> train_heads -> Model_Builder -> a forward."""
import os
import shutil

import numpy as np
import pytest
import torch

import heads_train_cases as HC
from nlml_hpe_amd import MLPHeadsTrainer as MT
from nlml_hpe_amd import _lib, ops, weights

pytestmark = pytest.mark.gpu

# (R, rows of the three networks -- B differs per network inside every launch, padded x)
#   256 / 33 / 1     the full batch, two tiles of rows, wgrad K = 1 with fifteen empty bias runs
#   15 / 16 / 17     the second super-chunk and wave 1 appear in the wgrad
#   129 / 255 / 2    spw = 2 with one row on wave 4; a last bias run of 15 rows
#   R = 1, 5         layer 0 with one and five k of its only super-chunk; R = 3 and ldx = 4: x rows that are no 16-byte vectors apart
BITS = [(3, (256, 33, 1), False), (3, (15, 16, 17), False), (3, (129, 255, 2), False), (1, (256, 33, 1), False), (5, (256, 33, 1), False),
        (3, (256, 33, 1), True)]


def _nets(R, rows, padded=False, seed=0, state=None, step0=0, orders=None):
    tab, P = HC.table(R), HC.initial_params(R, seed)
    rows = rows if rows is not None else [len(o) for o in orders]
    nets = []
    for i, (name, n) in enumerate(zip(HC.NAMES, rows)):
        x, y = tab[name]
        if padded:
            wide = np.full((x.shape[0], R + 1), np.nan, np.float32)
            wide[:, :R] = x
            x = wide[:, :R]
        order = orders[i] if orders is not None else HC.synth.rng(seed, 60 + i).permutation(x.shape[0])[:n].astype(np.int32)
        nets.append(HC.new_net(x, y, P[i], order=order, step0=step0, state=state, seed=seed + i))
    return nets


@pytest.mark.parametrize("R,rows,padded", BITS)
def test_one_step_is_the_host_forms_words_and_the_oracles_order(device, R, rows, padded):
    batch = 256
    for max_norm, state, step0 in ((1.0, None, 0), (HC.NO_CLIP, "warm", 6)):
        host = _nets(R, rows, padded, state=state, step0=step0)
        dev = [HC.copy_net(n) for n in host]
        before = [n["params"].copy() for n in host]
        ws_h = HC.host_train(host, R, batch, max_norm=max_norm)
        ws_d, _, _ = HC.device_train(dev, R, batch, device, max_norm=max_norm)
        what = f"R = {R}, rows {rows}, max_norm {max_norm:g}"
        HC.assert_nets_equal(dev, host, what)
        assert all(int(n["status"][0]) == 0 for n in dev)
        # the whole workspace, word for word: rows, A_1..A_5, delta_1..delta_5, the f64 partials -- and the padding, which both leave NaN
        assert np.array_equal(ws_d.view(np.uint32), ws_h.view(np.uint32)), \
            f"{what}: {int((ws_d.view(np.uint32) != ws_h.view(np.uint32)).sum())} words of the workspace differ from the host form's"
        assert (HC.padding_words(ws_d, R, batch, rows) == HC.FILL).all(), f"{what}: a padding word was written"
        if max_norm == HC.NO_CLIP:   # c = 1: the stored gradient is the wgrad launches' own
            for i, B in enumerate(rows):
                assert float(dev[i]["norm"][0]) < 1e20
                obs = HC.workspace_views(ws_d, R, batch, i, B)
                HC.check_launches(obs, dev[i]["x"], dev[i]["y"], before[i], dev[i]["grads"], R, B, order=dev[i]["order"], what=f"{what}, network {i}")
                assert HC.same_words(HC.model_partials(HC.views(dev[i]["grads"], R), R), obs["partials"])


def test_a_network_alone_and_beside_two_others(device):
    R, batch = 3, 32
    three = _nets(R, (128, 64, 128))           # four steps; network 1 is exhausted after step 2
    alone = [HC.copy_net(three[1])]
    solo0 = [HC.copy_net(three[0])]
    ws3, dnets, _ = HC.device_train(three, R, batch, device)
    HC.device_train(alone, R, batch, device)
    HC.device_train(solo0, R, batch, device)
    HC.assert_nets_equal([three[1]], alone, "network 1 of three against itself alone (steps 3-4 must not touch it)")
    HC.assert_nets_equal([three[0]], solo0, "network 0 of three against itself alone")
    assert three[1]["loss"].shape == (2,) and three[0]["loss"].shape == (4,)
    # its later call continues with t = 3: the host form from the same state with step0 = 2
    later = HC.copy_net(three[1])
    later["step0"] = 2
    host = [HC.copy_net(later)]
    HC.host_train(host, R, batch)
    cont = [later]
    HC.device_train(cont, R, batch, device)
    HC.assert_nets_equal(cont, host, "network 1's next call (step0 = 2)")
    wrong = [HC.copy_net(three[1])]
    HC.host_train(wrong, R, batch)              # step0 = 0: another bias correction
    assert not HC.same_words(wrong[0]["params"], host[0]["params"]), "step0 must matter here"


def test_four_steps_across_two_calls_carry_the_step_count(device):
    R, batch = 3, 33
    orders = [HC.synth.rng(3, 70 + i).permutation(600)[:n].astype(np.int32) for i, n in enumerate((132, 99, 100))]
    whole = _nets(R, None, orders=orders)
    HC.host_train(whole, R, batch)             # 4 / 3 / 4 steps in one host call
    first = _nets(R, None, orders=[o[:66] for o in orders])
    second_orders = [o[66:] for o in orders]
    # a stale workspace: a call with the full batch of 256 leaves a larger step's rows, activations and partials in it
    big = _nets(R, (256, 256, 256))
    stale = torch.full((_lib.lib().nlml_heads_train_workspace_bytes(R, 256, 3) // 4,), float("nan"), dtype=torch.float32, device=device)
    HC.device_train(big, R, 256, device, ws=stale)
    HC.device_train(first, R, batch, device)
    second = []
    for net, o in zip(first, second_orders):
        nxt = HC.copy_net(net)
        nxt["order"], nxt["n"], nxt["step0"] = np.ascontiguousarray(o), len(o), 2
        second.append(nxt)
    again = [HC.copy_net(n) for n in second]
    HC.device_train(second, R, batch, device)
    HC.device_train(again, R, batch, device, ws=stale)
    HC.assert_nets_equal(again, second, "a stale workspace against a NaN-filled one")
    for i in range(3):
        for k in ("params", "grads", "m", "v"):
            assert HC.same_words(second[i][k], whole[i][k]), f"network {i}: {k} after 2 + 2 steps differs from the host form's four"
        assert HC.same_words(np.concatenate([first[i]["loss"], second[i]["loss"]]), whole[i]["loss"])
        assert HC.same_words(np.concatenate([first[i]["norm"], second[i]["norm"]]), whole[i]["norm"])


def test_evaluation_clamped_orders_and_the_torch_op(device):
    R, batch = 3, 64
    nets = _nets(R, (64, 40, 7))
    ev = [HC.copy_net(n) for n in nets]
    ev_h = [HC.copy_net(n) for n in nets]
    ws_e = HC.device_eval(ev, R, batch, device)
    HC.host_eval(ev_h, R, batch)
    HC.device_train(nets, R, batch, device)
    for i in range(3):
        assert HC.same_words(ev[i]["loss"], nets[i]["loss"]), "the evaluation pass's loss is the training forward's"
        assert HC.same_words(ev[i]["loss"], ev_h[i]["loss"]) and int(ev[i]["status"][0]) == 0
    assert (HC.padding_words(ws_e, R, batch, (64, 40, 7), train=False) == HC.FILL).all(), "the evaluation pass wrote beyond rows and A_1..A_5"
    # order entries outside [0, N) are clamped and flagged; the result is the clamped order's
    N = [n["x"].shape[0] for n in nets]
    bad = _nets(R, (64, 40, 7))
    bad[0]["order"][[3, 17]] = [-5, N[0] + 10]
    bad[2]["order"][0] = 2 ** 31 - 1
    good = [HC.copy_net(n) for n in bad]
    for n_, N_ in zip(good, N):
        n_["order"] = np.clip(n_["order"], 0, N_ - 1).astype(np.int32)
    host = [HC.copy_net(n) for n in bad]
    HC.device_train(bad, R, batch, device)
    HC.device_train(good, R, batch, device)
    HC.host_train(host, R, batch)
    assert [int(n["status"][0]) for n in bad] == [1, 0, 1] and [int(n["status"][0]) for n in host] == [1, 0, 1]
    HC.assert_nets_equal(bad, good, "clamped orders", keys=("params", "grads", "m", "v", "loss", "norm"))
    # torch.ops.nlml_hpe.heads_train_steps is ops.heads_train_steps
    a, b = _nets(R, (64, 40, 7), state="warm", step0=3), _nets(R, (64, 40, 7), state="warm", step0=3)
    HC.device_train(a, R, batch, device, lr=1e-3)
    d = HC.device_nets(b, device)
    loss, norm, status = torch.ops.nlml_hpe.heads_train_steps([n["x"] for n in d], [n["y"] for n in d], [n["params"] for n in d],
                                                              [n["grads"] for n in d], [n["m"] for n in d], [n["v"] for n in d],
                                                              [n["order"] for n in d], [n["n"] for n in d], [n["step0"] for n in d], batch,
                                                              1e-3, 1e-5, 1.0)
    assert status.cpu().tolist() == [0, 0, 0]
    for i in range(3):
        for k in ("params", "grads", "m", "v"):
            assert HC.same_words(d[i][k].cpu().numpy(), a[i][k]), f"torch op: network {i}: {k}"
        assert HC.same_words(loss[i].cpu().numpy(), a[i]["loss"]) and HC.same_words(norm[i].cpu().numpy(), a[i]["norm"])


def test_gradient_path_on_the_device(device):
    """Item 5 of the CPU tests (test_heads_train_host.py) once on the device: B = 33, the clip on."""
    R, B = 3, 33
    x, y, params, _, _ = HC.gradient_case(R, B)
    net = [HC.new_net(x, y, params)]
    HC.device_train(net, R, 256, device, max_norm=1.0)
    sd = HC.views(params, R)
    exact, t32 = HC.torch_step(sd, x, y, torch.float64, 1.0), HC.torch_step(sd, x, y, torch.float32, 1.0)
    got = {"loss": float(net[0]["loss"][0]), "norm": float(net[0]["norm"][0]), "grads": HC.views(net[0]["grads"], R)}
    HC.check_claim(got, exact, t32, "device, B = 33, clip on")


def _small_tables():
    # 375 / 300 / 225 rows: 300 / 240 / 180 of them train, 3 / 2 / 2 steps at batch 128
    tab = HC.table(3, rows=(375, 300, 225))
    return {n: tab[n] for n in HC.NAMES}


def test_the_loop_on_the_device_is_the_host_forms(device):
    kw = dict(tables=_small_tables(), out_dir=None, epochs=3, batch_size=128, scheduler_step_size=1, verbose=False, config=None)
    sd_d, h_d = MT.train_heads(None, backend="device", device=device, **kw)
    sd_h, h_h = MT.train_heads(None, backend="host", **kw)
    for name in HC.NAMES:
        assert [len(s) for s in h_d[name]["step_loss"]] == [{"yaw": 3, "pitch": 2, "roll": 2}[name]] * 3
        assert HC.same_words(np.concatenate(h_d[name]["step_loss"]), np.concatenate(h_h[name]["step_loss"]))
        assert h_d[name]["val_loss"] == h_h[name]["val_loss"] and h_d[name]["best_epoch"] == h_h[name]["best_epoch"]
        for k in HC.KEYS:
            assert HC.same_words(sd_d[name][k], sd_h[name][k]), f"{name}: {k}"


def test_the_chain_from_trained_data_to_a_forward(device, repo_root, tmp_path, monkeypatch):
    import NLML_HPE_Model_Builder as MB
    from nlml_hpe_amd.entrypoints import load_config
    from nlml_hpe_amd.model import load_model
    from nlml_hpe_amd import synth

    models = tmp_path / "models"
    sds, hist = MT.train_heads(os.path.join(repo_root, "outputs", "features", "Trained_data.npz"),
                               os.path.join(repo_root, "configs", "config_MlpHeads.yaml"), out_dir=str(models), epochs=5, device=device, verbose=False)
    heads = weights.load_head_state_dicts(str(models))
    enc = synth.encoder_state_dict(1404, 0)
    assert weights.validate_shapes(enc, heads) == 1404
    for name in HC.NAMES:
        assert all(HC.same_words(heads[name][k].numpy(), sds[name][k]) for k in HC.KEYS)
        assert np.isfinite(hist[name]["val_loss"]).all() and hist[name]["saved_epoch"] == hist[name]["best_epoch"]
        print(f"{name}: train {hist[name]['train_loss']}, val {hist[name]['val_loss']}")
    # the trained heads' float64 forward on the validation rows reproduces the reported validation loss (keep="last" run: the live weights)
    cfg = load_config(os.path.join(repo_root, "configs", "config_MlpHeads.yaml"))
    sds_l, hist_l = MT.train_heads(os.path.join(repo_root, "outputs", "features", "Trained_data.npz"), cfg, out_dir=None, epochs=5, keep="last",
                                   device=device, verbose=False)
    from nlml_hpe_amd.artefacts import heads_training_table
    td = np.load(os.path.join(repo_root, "outputs", "features", "Trained_data.npz"))
    tab = heads_training_table(cfg, {n: td[f"optimized_{n}"] for n in HC.NAMES}, device=device)
    for name in HC.NAMES:
        assert hist_l[name]["val_loss"] == hist[name]["val_loss"] and hist_l[name]["saved_epoch"] == 5
        val = hist_l["split"][name][1]
        xv, yv = tab[name][0].cpu().numpy().astype(np.float32)[val], tab[name][1].astype(np.float32)[val]
        losses = {}
        for dtype in (torch.float64, torch.float32):
            ps = {k: torch.tensor(sds_l[name][k], dtype=dtype) for k in HC.KEYS}
            with torch.no_grad():
                losses[dtype] = np.mean([float(torch.nn.MSELoss()(HC.torch_forward(ps, torch.tensor(xv[s:s + 256], dtype=dtype)),
                                                                  torch.tensor(yv[s:s + 256], dtype=dtype))) for s in range(0, len(yv), 256)])
        d_g = abs(hist_l[name]["val_loss"][-1] - losses[torch.float64]) / losses[torch.float64]
        d_t = abs(losses[torch.float32] - losses[torch.float64]) / losses[torch.float64]
        print(f"{name}: reported validation loss {hist_l[name]['val_loss'][-1]:.6e}, float64 {losses[torch.float64]:.6e}: {d_g:.2e} (torch-f32 {d_t:.2e})")
        assert d_g <= max(HC.MARGIN * d_t, HC.FLOOR), f"{name}: the reported validation loss is {d_g:.3e} from the float64 forward's"
    # the model builder on those heads with a synthetic encoder, and a forward
    shutil.copytree(os.path.join(repo_root, "configs"), tmp_path / "configs")
    shutil.copytree(os.path.join(repo_root, "outputs", "features"), tmp_path / "outputs" / "features")
    monkeypatch.chdir(tmp_path)
    packed = MB.model_builder(["--synthetic-encoder-seed", "0"])
    assert os.path.getsize(packed) > 0
    raw = synth.raw_landmarks(8, seed=1)
    pose = load_model("models", device, encoder_state_dict=enc).from_landmarks(torch.from_numpy(raw).to(device))
    assert pose.shape == (8, 3) and bool(torch.isfinite(pose).all())
