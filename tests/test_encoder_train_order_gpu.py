"""GPU: the encoder-training kernels (K9, csrc/encoder_train.hip) held to the C oracle's order model BIT FOR BIT, launch by launch.

A call of one step leaves that step's resolved rows, A_1..A_6, delta_1..delta_6 and the f64 norm partials in the caller's workspace,
so every one of the fourteen launches is compared with the model of tests/encoder_train_order_cases.py fed the DEVICE's own inputs to
that launch (uint32 / uint64 words; -0 is not +0).  ocml's tanhf is the one thing not reproduced: A_5 is held to 5 ulp of float64
tanh of the model's Z_4.  The model itself is held to the host form, to float64 and to its deliberately wrong variants in
tests/test_encoder_train_order_host.py.  The measured counts (all 0) and the tanhf ulp maximum are in profiles/encoder_train.md.
"""
import numpy as np
import pytest
import torch

import encoder_train_cases as EC
import encoder_train_order_cases as OC
from nlml_hpe_amd import _lib
from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu

CLIP = dict(lr=0.0, weight_decay=0.0, max_norm=0.1, zero_grad=False)
CLIP_UPDATE = dict(lr=1e-2, weight_decay=1e-2, max_norm=0.1, zero_grad=False)


def _one_step(cs, dev, B, batch, hyper, order=None, p=None, g=None, ws=None, **kw):
    """One step of B rows (slots 0..B-1 of `order`) on a NaN-filled workspace -> dict(before, after, ws_bytes, loss, norm, status)."""
    if p is None:
        p, g = OC.fresh(cs, dev)
    before = OC.state(p, g)
    order = np.arange(B, dtype=np.int32) if order is None else order
    assert len(order) == B
    loss, norm, status, ws = OC.device_call(cs, dev, order, batch, p, g, hyper, ws=ws, **kw)
    assert loss.shape == (1,) and norm.shape == (1,)
    return {"before": before, "after": OC.state(p, g), "ws": OC.ws_bytes_of(ws), "loss": loss[0], "norm": norm[0], "status": status,
            "device": (p, g)}


def _pin(cs, run, rows, batch, hyper, what, **kw):
    bad, info = OC.pin_step(cs, rows, run["before"], run["after"], run["ws"], batch, run["loss"], run["norm"], hyper, **kw)
    print(f"{what}: tanhf within {info['tanh_ulp']} ulp of float64 tanh, c = {info['c']!r}")
    OC.assert_pinned(bad, what)
    return info


def _same_outputs(a, b):
    return (OC.mismatches(a["loss"], b["loss"]) == 0 and OC.mismatches(a["norm"], b["norm"]) == 0
            and all(OC.mismatches(x, y) == 0 for x, y in zip(a["after"], b["after"])))


# ---- one step, every launch --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F, B", OC.SHAPES)
def test_single_step_launch_by_launch(device, F, B):
    cs = EC.case(F, B)
    run = _one_step(cs, device, B, B, OC.NO_CLIP)
    assert run["status"] == 0
    info = _pin(cs, run, np.arange(B, dtype=np.int32), B, OC.NO_CLIP, f"K9 pin F={F} B={B}")
    assert info["c"] == 1.0 and OC.mismatches(run["after"][0], run["before"][0]) == 0, "lr = 0 and c = 1 keep the parameters"


def test_workspace_of_a_larger_batch_gives_the_same_bits(device):
    """B = 33 in the workspace of batch = 33 and of batch = 256: every offset differs, no bit may."""
    F, B = 136, 33
    cs = EC.case(F, B)
    tight, wide = _one_step(cs, device, B, B, OC.NO_CLIP), _one_step(cs, device, B, 256, OC.NO_CLIP)
    _pin(cs, wide, np.arange(B, dtype=np.int32), 256, OC.NO_CLIP, "K9 pin F=136 B=33 in the workspace of batch 256")
    assert _same_outputs(tight, wide)
    a, b = OC.workspace_views(tight["ws"], F, B, B), OC.workspace_views(wide["ws"], F, 256, B)
    assert OC.mismatches(a["rows"], b["rows"]) == 0 and OC.mismatches(a["partials"], b["partials"]) == 0
    assert all(OC.mismatches(x, y) == 0 for k in ("act", "delta") for x, y in zip(a[k], b[k]))


# ---- clip and update ---------------------------------------------------------------------------------------------------------------------
def test_clip_and_update_word_for_word(device):
    """G_pre comes from the c = 1 run and c from the model's norm of it: G_out = float(c) G_pre, p_out = the model's update."""
    F, B = 136, 33
    cs = EC.case(F, B)
    rows = np.arange(B, dtype=np.int32)
    g_pre = _one_step(cs, device, B, B, OC.NO_CLIP)["after"][1]
    nm = CO.et_norm(F, G=g_pre, max_norm=CLIP["max_norm"])
    c32 = np.float32(nm["c"])
    assert c32 < 1.0, "the step clips"
    for hyper, what in ((CLIP, "clip"), (CLIP_UPDATE, "clip, lr and weight decay")):
        run = _one_step(cs, device, B, B, hyper)
        assert OC.mismatches(run["norm"], np.float32(nm["norm"])) == 0
        assert OC.mismatches(run["after"][1], (c32 * g_pre).astype(np.float32)) == 0, f"{what}: G_out = float(c) G_pre"
        p_want, g_want = CO.et_update(cs["params"], g_pre, c32, hyper["lr"], hyper["weight_decay"])
        assert OC.mismatches(run["after"][0], p_want) == 0 and OC.mismatches(run["after"][1], g_want) == 0, f"{what}: the model's update"
        _pin(cs, run, rows, B, hyper, f"K9 pin F=136 B=33 {what}", accuracy=False)
    assert OC.mismatches(run["after"][0], cs["params"]) > 0, "lr = 1e-2 moves the parameters"


# ---- a chain of steps --------------------------------------------------------------------------------------------------------------------
def test_four_steps_pinned_one_by_one_then_as_one_call(device):
    F, B, hyper = 136, 33, dict(lr=1e-2, weight_decay=1e-2, max_norm=0.3, zero_grad=False)
    cs = EC.case(F, 4 * B)
    order = EC.epoch_orders(4 * B, 1)[0]
    p, g = OC.fresh(cs, device)
    losses, norms = [], []
    for s in range(4):   # no zero_grad: step s accumulates onto the clipped G of step s - 1, and starts from the DEVICE's state
        rows = order[s * B:(s + 1) * B]
        run = _one_step(cs, device, B, B, hyper, order=rows, p=p, g=g)
        info = _pin(cs, run, rows, B, hyper, f"K9 pin chain step {s}", accuracy=False)
        assert info["c"] < 1.0, "every step of the chain clips"
        losses.append(run["loss"])
        norms.append(run["norm"])
    single = {"loss": np.array(losses), "norm": np.array(norms), "after": run["after"]}
    p2, g2 = OC.fresh(cs, device)
    loss, norm, status, _ = OC.device_call(cs, device, order, B, p2, g2, hyper)
    assert status == 0 and _same_outputs(single, {"loss": loss, "norm": norm, "after": OC.state(p2, g2)})


def test_partial_last_batch_over_the_stale_rows_of_the_step_before(device):
    """40 rows, then 7 on the same workspace: rows 7..39 of every tensor still hold the larger step's values."""
    F, hyper = 136, dict(lr=1e-2, weight_decay=1e-2, max_norm=0.3, zero_grad=False)
    cs = EC.case(F, 47)
    order = EC.epoch_orders(47, 1)[0]
    p, g = OC.fresh(cs, device)
    first = _one_step(cs, device, 40, 40, hyper, order=order[:40], p=p, g=g)
    _pin(cs, first, order[:40], 40, hyper, "K9 pin B=40", accuracy=False)
    second = _one_step(cs, device, 7, 7, hyper, order=order[40:], p=p, g=g)
    _pin(cs, second, order[40:], 7, hyper, "K9 pin B=7 after B=40", accuracy=False)
    p2, g2 = OC.fresh(cs, device)
    loss, norm, status, ws = OC.device_call(cs, device, order, 40, p2, g2, hyper)
    both = {"loss": loss, "norm": norm, "after": OC.state(p2, g2)}
    assert status == 0 and _same_outputs({"loss": np.array([first["loss"], second["loss"]]), "norm": np.array([first["norm"], second["norm"]]),
                                          "after": second["after"]}, both)
    a, b = OC.workspace_views(second["ws"], F, 7, 7), OC.workspace_views(OC.ws_bytes_of(ws), F, 40, 7)
    assert OC.mismatches(a["rows"], b["rows"]) == 0 and OC.mismatches(a["partials"], b["partials"]) == 0
    assert all(OC.mismatches(x, y) == 0 for k in ("act", "delta") for x, y in zip(a[k], b[k]))
    stale = OC.workspace_views(OC.ws_bytes_of(ws), F, 40, 40)
    assert all(np.isfinite(t[7:]).all() for k in ("act", "delta") for t in stale[k]), "the larger step's rows are still there"


# ---- small things ------------------------------------------------------------------------------------------------------------------------
def test_x_and_a_table_off_16_byte_alignment_give_the_aligned_bits(device):
    """The ABI asks 4-byte alignment of x, the tables and the labels.  x: a view one, two and three floats into a larger tensor with
    ldx % 4 == 0 (so only the base pointer loses the 16 bytes); a table: one float into a larger buffer."""
    F, B, ldx = 136, 33, 140
    cs = EC.case(F, B)
    want = _one_step(cs, device, B, B, CLIP_UPDATE)
    for off in (0, 1, 2, 3):
        buf = torch.full((B * ldx + 4,), float("nan"), dtype=torch.float32, device=device)
        x = buf[off:off + B * ldx].view(B, ldx)[:, :F]
        x.copy_(torch.from_numpy(cs["x"]).to(device))
        assert x.data_ptr() % 16 == 4 * off and x.stride(0) % 4 == 0
        tabs = [torch.from_numpy(t).to(device) for t in cs["tables"]]
        if off:
            k = off - 1
            tb = torch.full((tabs[k].numel() + 1,), float("nan"), dtype=torch.float32, device=device)
            tb[1:] = tabs[k].reshape(-1)
            tabs[k] = tb[1:].view(-1, 3)
            assert tabs[k].data_ptr() % 16 == 4 and tabs[k].is_contiguous()
        got = _one_step(cs, device, B, B, CLIP_UPDATE, x=x, tabs=tabs)
        assert got["status"] == 0 and _same_outputs(want, got), f"x {4 * off} bytes off 16-byte alignment"
        assert OC.mismatches(want["ws"], got["ws"]) == 0, "the whole workspace, padding included"


def test_order_entry_out_of_range_in_one_step_only_is_flagged(device):
    F, B = 136, 33
    cs = EC.case(F, 2 * B)
    order = np.arange(2 * B, dtype=np.int32)
    runs = {}
    for name, at, bad, clamped in (("first step only", 5, -3, 0), ("second step only", B + 5, 2 * B + 1000, 2 * B - 1)):
        for which, value in (("bad", bad), ("clamped", clamped)):
            o = order.copy()
            o[at] = value
            p, g = OC.fresh(cs, device)
            loss, norm, status, _ = OC.device_call(cs, device, o, B, p, g, CLIP_UPDATE)
            runs[name, which] = {"loss": loss, "norm": norm, "after": OC.state(p, g), "status": status}
        assert runs[name, "bad"]["status"] == _lib.ENCODER_TRAIN_CLAMPED_ORDER, f"{name}: the bit is set after the last step"
        assert runs[name, "clamped"]["status"] == 0 and _same_outputs(runs[name, "bad"], runs[name, "clamped"])


def test_eval_losses_give_the_model_loss_bits(device):
    from nlml_hpe_amd import ops
    F, N, batch = 136, 40, 33      # the second batch has 7 rows; the workspace holds its forward afterwards
    cs = EC.case(F, N)
    x, lab, tabs = EC.device_inputs(cs, device)
    p = torch.from_numpy(cs["params"]).to(device)
    ws = OC.nan_workspace(F, batch, device)
    ev, status = ops.encoder_eval_losses(x, lab, tabs, p, batch=batch, workspace=ws)
    ev = ev.cpu().numpy()
    assert ev.shape == (2,) and int(status.cpu()[0]) == 0
    rows = np.arange(batch, N, dtype=np.int32)
    wsb = OC.ws_bytes_of(ws)
    obs = OC.workspace_views(wsb, F, batch, len(rows))
    assert OC.mismatches(obs["rows"], rows) == 0
    assert OC.mismatches(ev[1], CO.et_loss(obs["act"][5], OC.targets(cs, rows))["loss"]) == 0
    lay = OC.layout(F, batch)
    assert (wsb[lay["delta"][0]:lay["bytes"]].view(np.uint32) == OC.FILL).all(), "the validation pass writes no delta"
    # the first batch: the training step's forward on the same rows (lr = 0 keeps the parameters), pinned above launch by launch
    run = _one_step(cs, device, batch, batch, OC.NO_CLIP)
    assert OC.mismatches(ev[0], run["loss"]) == 0
    first = OC.workspace_views(run["ws"], F, batch, batch)
    assert OC.mismatches(run["loss"], CO.et_loss(first["act"][5], OC.targets(cs, np.arange(batch)))["loss"]) == 0
