"""Shared cases and yardsticks of the encoder-training tests (K9: csrc/encoder_train.hip, csrc/encoder_train_ref.h).

YARDSTICKS, both the reference's own loop (NLML_HPE_EncoderTrainer.py:400-454: three MSELoss means, backward WITHOUT zero_grad,
clip_grad_norm_, SGD with weight decay) written with torch on the CPU, sharing no code with the library:
  exact    the loop in float64 autograd
  torch32  the same loop in float32: the reference's arithmetic
THE CLAIM, for the loss, the norm, each of the twelve gradient tensors and each updated parameter tensor: the relative Frobenius
distance from `exact` is at most MARGIN = 4 x torch32's distance from it on the same inputs (two legitimate f32 summation orders
differ by a small factor on a single draw; the margin is the cosine fit's), with a floor of 4 x 2^-24 (a few roundings per element)
where torch32 happens to land exactly.

INPUTS.  A ReLU mask must not be able to flip legitimately, so no pre-activation of a ReLU layer may lie within f32 rounding of zero
in the float64 run.  z = sum_k a_k w_k + b is a chain of K + 1 roundings, each at most 2^-24 of a partial sum; the partial sums of
any order are of the size of R = sqrt(sum (a_k w_k)^2 + b^2) and the roundings add like a random walk, so an f32 value differs from z
by about sqrt(K + 1) 2^-24 R.  A row is used only where every ReLU pre-activation has |z| > 16 sqrt(K + 1) 2^-24 R (`relu_margin`:
sixteen such deviations) -- at the start, and in the two-step runs at both steps (`settled`, which replaces the rows the float64 run
finds too close and runs again).  The worst-case bound (K + 1) 2^-24 sum |a_k w_k| is not used: at K = 1404 it is a hundred
deviations wide.
The twenty-step run checks its rows at the start only, and is held to the claim on the PARAMETERS and the losses, as its issue
states it: 3,000 row visits times 1,920 pre-activations put about forty of them inside any such margin at some step, whatever rows
are drawn (replacing rows moves the trajectory by far more than the margin, so every attempt is a fresh draw), so there the masks of
two f32 runs CAN legitimately differ in an entry.  A flipped entry moves one row of one gradient by about 1e-3 of its size, which is
far beyond 4 x torch-f32's distance on the gradients, and moves the parameters by lr times that, which is below the floor.
"""
import functools
import os

import numpy as np
import torch

from nlml_hpe_amd import _lib, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 4.0
FLOOR = 4.0 * 2.0 ** -24
WIDTHS = (1024, 512, 256, 128, 64, 9)
KEYS = [f"encoder.{2 * i}.{k}" for i in range(6) for k in ("weight", "bias")]
LD_LAB = 4                         # labels carry a fourth column (the identity), as the reference's do
_STREAM_ROWS, _STREAM_LABELS = 40, 41


def tables():
    fm = np.load(os.path.join(REPO, "outputs", "features", "Factor_Matrices.npz"))
    return [np.ascontiguousarray(fm[k], dtype=np.float32) for k in ("U_yaw", "U_pitch", "U_roll")]


def flat(sd) -> np.ndarray:
    return np.concatenate([np.asarray(sd[k], np.float32).ravel() for k in KEYS])


def views(buf, F):
    out, off, fan_in = {}, 0, F
    for i, w in enumerate(WIDTHS):
        out[f"encoder.{2 * i}.weight"] = buf[off:off + w * fan_in].reshape(w, fan_in)
        off += w * fan_in
        out[f"encoder.{2 * i}.bias"] = buf[off:off + w]
        off += w
        fan_in = w
    assert off == buf.shape[0]
    return out


def relu_margin(sd, x) -> np.ndarray:
    """Per row of x: min over the ReLU layers' pre-activations of |z| / (16 sqrt(K + 1) 2^-24 R), in float64."""
    h = torch.from_numpy(np.asarray(x, np.float64))
    worst = torch.full((h.shape[0],), float("inf"), dtype=torch.float64)
    for i in range(4):
        W = torch.from_numpy(np.asarray(sd[f"encoder.{2 * i}.weight"], np.float64))
        b = torch.from_numpy(np.asarray(sd[f"encoder.{2 * i}.bias"], np.float64))
        z = h @ W.T + b
        R = torch.sqrt((h * h) @ (W * W).T + b * b)
        worst = torch.minimum(worst, (z.abs() / (16.0 * np.sqrt(W.shape[1] + 1.0) * 2.0 ** -24 * R)).min(dim=1).values)
        h = torch.relu(z)
    return worst.numpy()


@functools.lru_cache(maxsize=None)
def case(F: int, N: int, seed: int = 0, rows=None):
    """N dataset rows with labels, the tables and a synth.encoder_state_dict start (mixed signs: non-trivial masks, tanh' not ~1).
    rows: the candidate rows to use, a tuple (`settled`); None: the first N that pass relu_margin."""
    sd = synth.encoder_state_dict(F, seed=seed)
    cand = synth.features(4 * N + 64, F, seed=100 + seed)
    ok = np.flatnonzero(relu_margin(sd, cand) > 1.0)
    assert ok.size >= N, f"only {ok.size} of {cand.shape[0]} candidate rows keep every ReLU pre-activation away from zero"
    used = ok[:N] if rows is None else np.array(rows, np.int64)
    x = np.ascontiguousarray(cand[used])
    tabs = tables()
    g = synth.rng(seed, _STREAM_LABELS)
    labels = np.stack([g.integers(0, t.shape[0], size=N) for t in tabs] + [np.arange(N)], axis=1).astype(np.int32)
    assert labels.shape[1] == LD_LAB
    return {"F": F, "N": N, "x": x, "labels": labels, "tables": tabs, "sd": sd, "params": flat(sd), "cand": used, "pool": ok[N:]}


def batches_of(order, batch):
    order = np.asarray(order)
    return [order[s:s + batch] for s in range(0, len(order), batch)]


def torch_loop(cs, dtype, batches, lr=1e-4, weight_decay=1e-5, max_norm=20.0, zero_grad=False, check_margin=False, violators=None,
               margin_floor=1.0):
    """The reference's loop over `batches` (index arrays; check_margin: every visited row passes relu_margin at that step ("first": at the first), or, with a
    set `violators`, the rows whose margin is at most margin_floor are added to it) -> dict(loss [steps], norm [steps], grads {key: array}, params {key: array})."""
    ps = {k: torch.tensor(np.asarray(cs["sd"][k]), dtype=dtype, requires_grad=True) for k in KEYS}
    opt = torch.optim.SGD(list(ps.values()), lr=lr, weight_decay=weight_decay)
    crit = torch.nn.MSELoss()
    tabs = [torch.tensor(t, dtype=dtype) for t in cs["tables"]]
    losses, norms = [], []
    for step, idx in enumerate(batches):
        if zero_grad:
            opt.zero_grad()
        if check_margin and (check_margin != "first" or step == 0):
            m = relu_margin({k: v.detach().numpy() for k, v in ps.items()}, cs["x"][idx])
            if violators is not None:
                violators.update(int(i) for i in np.asarray(idx)[m <= margin_floor])
            else:
                assert m.min() > 1.0, f"a ReLU pre-activation within f32 rounding of zero (margin ratio {m.min():.3f})"
        h = torch.tensor(cs["x"][idx], dtype=dtype)
        for i in range(6):
            h = torch.nn.functional.linear(h, ps[f"encoder.{2 * i}.weight"], ps[f"encoder.{2 * i}.bias"])
            h = torch.relu(h) if i < 4 else (torch.tanh(h) if i == 4 else h)
        lab = cs["labels"][idx]
        loss = sum(crit(h[:, 3 * t:3 * t + 3], tabs[t][lab[:, t]]) for t in range(3))
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(ps.values()), max_norm=max_norm)))
        opt.step()
        losses.append(float(loss.detach()))
    return {"loss": np.array(losses), "norm": np.array(norms), "grads": {k: v.grad.detach().numpy().copy() for k, v in ps.items()},
            "params": {k: v.detach().numpy().copy() for k, v in ps.items()}}


@functools.lru_cache(maxsize=None)
def yardsticks(F, N, batch, hyper=(), order=None, seed=0, check_margin=True):
    """(exact, torch32) for the case's rows in `order` (a tuple, or a tuple of tuples: one per epoch; None: 0..N-1) cut into batches;
    hyper: (name, value) pairs."""
    cs = case(F, N, seed)
    epochs = [np.arange(N)] if order is None else ([np.array(o) for o in order] if isinstance(order[0], tuple) else [np.array(order)])
    b = [piece for o in epochs for piece in batches_of(o, batch)]
    kw = dict(hyper)
    return torch_loop(cs, torch.float64, b, check_margin=check_margin, **kw), torch_loop(cs, torch.float32, b, **kw)


@functools.lru_cache(maxsize=None)
def settled(F, N, batch, epochs, hyper=(), seed=0):
    """A case whose rows stay clear of every ReLU's zero through the whole float64 run -> (case, orders, exact, torch32).  epochs: a
    number of shuffled epochs (epoch_orders) or the orders themselves, a tuple of tuples.  Rows the run finds too close are replaced
    by unused candidates and the run is repeated."""
    orders = epoch_orders(N, epochs, seed) if isinstance(epochs, int) else [np.array(o, np.int32) for o in epochs]
    b = [piece for o in orders for piece in batches_of(o, batch)]
    rows, spare = None, 0
    for _ in range(16):
        cs = case(F, N, seed, rows)
        bad = set()
        exact = torch_loop(cs, torch.float64, b, check_margin=True, violators=bad, **dict(hyper))
        if not bad:
            return cs, orders, exact, torch_loop(cs, torch.float32, b, **dict(hyper))
        rows = [int(v) for v in cs["cand"]]
        for i in sorted(bad):   # the row at position i (its label and its place in every order stay) becomes the next spare candidate
            rows[i] = int(cs["pool"][spare])
            spare += 1
        rows = tuple(rows)
    raise AssertionError("no set of rows stays clear of the ReLU zeros")


def distance(got, exact) -> float:
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    den = np.linalg.norm(exact.ravel())
    return float(np.linalg.norm((got - exact).ravel()) / den) if den > 0 else float(np.linalg.norm(got.ravel()))


def check_claim(got, exact, t32, what, report=None, parts=("loss", "norm", "grads", "params")):
    """got: dict(loss, norm, grads, params) like torch_loop's.  Asserts the claim for every quantity of `parts`; -> the measured ratios."""
    rows = [(k, got[k], exact[k], t32[k]) for k in ("loss", "norm") if k in parts]
    for part in [k for k in ("grads", "params") if k in parts]:
        rows += [(f"{part}[{k}]", got[part][k], exact[part][k], t32[part][k]) for k in KEYS]
    ratios, bad = {}, []
    for name, g, e, t in rows:
        d_g, d_t = distance(g, e), distance(t, e)
        ratios[name] = (d_g, d_t)
        if not d_g <= max(MARGIN * d_t, FLOOR):
            bad.append(f"{name}: {d_g:.3e} vs torch-f32 {d_t:.3e} (x{d_g / max(d_t, 1e-300):.2f})")
    worst = max(ratios.items(), key=lambda kv: kv[1][0] / max(kv[1][1], FLOOR / MARGIN))
    print(f"{what}: worst {worst[0]} {worst[1][0]:.3e} vs torch-f32 {worst[1][1]:.3e} "
          f"(x{worst[1][0] / max(worst[1][1], FLOOR / MARGIN):.2f} of the allowance base)")
    if report is not None:
        report[what] = ratios
    assert not bad, f"{what}: beyond {MARGIN} x torch-f32's distance from the float64 result: " + "; ".join(bad)
    return ratios


# ---- the library's host form through ctypes ----------------------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data if a is not None else None


def data_args(x, labels, tabs):
    assert x.strides[1] == 4 and labels.flags.c_contiguous
    return [_ptr(x), x.strides[0] // 4, x.shape[0], _ptr(labels), labels.shape[1]] + [v for t in tabs for v in (_ptr(t), t.shape[0])]


def host_train(cs, order, batch, params=None, grads=None, lr=1e-4, weight_decay=1e-5, max_norm=20.0, zero_grad=False, x=None, labels=None,
               F=None):
    """nlml_encoder_train_steps_host -> dict like torch_loop's, plus status; params / grads (flat f32) are updated in place when given."""
    F = cs["F"] if F is None else F
    x = cs["x"] if x is None else x
    labels = cs["labels"] if labels is None else labels
    params = cs["params"].copy() if params is None else params
    grads = np.zeros_like(params) if grads is None else grads
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    n = x.shape[0] if order is None else order.shape[0]
    steps = (n + batch - 1) // batch
    loss, norm, status = np.full(steps, np.nan, np.float32), np.full(steps, np.nan, np.float32), np.full(1, -1, np.int32)
    rc = _lib.lib().nlml_encoder_train_steps_host(*data_args(x, labels, cs["tables"]), _ptr(params), _ptr(grads), F, batch, _ptr(order), n,
                                                  lr, weight_decay, max_norm, int(zero_grad), _ptr(loss), _ptr(norm), _ptr(status))
    _lib.check(rc, "nlml_encoder_train_steps_host")
    return {"loss": loss, "norm": norm, "status": int(status[0]), "grads": views(grads, F), "params": views(params, F), "flat": (params, grads)}


def host_eval(cs, order, batch, params=None):
    params = cs["params"] if params is None else params
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    n = cs["N"] if order is None else order.shape[0]
    loss, status = np.full((n + batch - 1) // batch, np.nan, np.float32), np.full(1, -1, np.int32)
    rc = _lib.lib().nlml_encoder_eval_losses_host(*data_args(cs["x"], cs["labels"], cs["tables"]), _ptr(params), cs["F"], batch, _ptr(order), n,
                                                  _ptr(loss), _ptr(status))
    _lib.check(rc, "nlml_encoder_eval_losses_host")
    return loss, int(status[0])


# ---- the device form ---------------------------------------------------------------------------------------------------------------
def device_inputs(cs, dev):
    return (torch.from_numpy(cs["x"]).to(dev), torch.from_numpy(cs["labels"]).to(dev), [torch.from_numpy(t).to(dev) for t in cs["tables"]])


def device_train(cs, dev, order, batch, params=None, grads=None, nan_workspace=True, x=None, **hyper):
    """ops.encoder_train_steps on a NaN-filled workspace -> dict like torch_loop's (numpy), plus status and the device buffers."""
    from nlml_hpe_amd import ops
    xd, lab, tabs = device_inputs(cs, dev)
    xd = xd if x is None else x
    p = torch.from_numpy(cs["params"]).to(dev) if params is None else params
    g = torch.zeros_like(p) if grads is None else grads
    od = None if order is None else torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(dev)
    ws = None
    if nan_workspace:
        ws = torch.full((_lib.lib().nlml_encoder_train_workspace_bytes(cs["F"], batch) // 4,), float("nan"), dtype=torch.float32, device=dev)
    loss, norm, status = ops.encoder_train_steps(xd, lab, tabs, p, g, order=od, batch=batch, workspace=ws, **hyper)
    ph, gh = p.cpu().numpy(), g.cpu().numpy()
    return {"loss": loss.cpu().numpy(), "norm": norm.cpu().numpy(), "status": int(status.cpu()[0]), "grads": views(gh, cs["F"]),
            "params": views(ph, cs["F"]), "flat": (ph, gh), "device": (p, g)}


def epoch_orders(N, epochs, seed=0):
    g = synth.rng(seed, _STREAM_ROWS)
    return [g.permutation(N).astype(np.int32) for _ in range(epochs)]
