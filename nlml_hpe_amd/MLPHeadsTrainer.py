"""Training of the yaw, pitch and roll heads (the reference's NLML_HPE_MLPHeadsTrainer.py), on the device.

The reference's ``train_MlpHeads`` (:132-251) trains three independent networks -- Linear(R,128) ReLU Linear(128,256) ReLU
Linear(256,128) ReLU Linear(128,64) ReLU Linear(64,1), R = the pose rank -- to map a row of the cosine table
a cos(b w + c) + d (one column per fitted curve of Trained_data.npz) back onto its angle w in radians: an 80/20 split, batches of
256 shuffled per epoch, zero_grad / MSELoss / backward / clip_grad_norm_(1.0) / Adam(lr 5e-3, weight_decay 1e-5), StepLR(10, 0.9)
stepped per epoch, 50 epochs, a validation pass per epoch.  Here an epoch is ONE training call of K10 for all three networks
(ops.heads_train_steps, csrc/heads_train.hip: every launch is shared by the three), ONE evaluation call (ops.heads_eval_losses) and
ONE synchronisation, to read the epoch's losses, decide the snapshots and print the reference's line.

WHICH EPOCH IS SAVED.  The reference keeps ``best_model_state = network.state_dict()`` (:119), which ALIASES the live tensors: the
file it really writes holds the LAST epoch's weights under the best epoch's printed number.  ``keep="best"`` (the default) saves the
weights of the epoch with the lowest validation loss, the stated intent; ``keep="last"`` saves what the reference's file holds.

The table comes from artefacts.heads_training_table (nlml_cosine_table, on the device) cast to float32 as the reference casts it.
The split, the epochs' permutations and the Kaiming-uniform initial weights (bound sqrt(6 / fan_in), zero biases, :59-66) come from
synth's Philox generator, as EncoderTrainer's do, so a run is reproducible from its seed on any machine; the bits of sklearn's
train_test_split(random_state=42) and of torch's generator are NOT reproduced.

``backend="host"`` runs the same operation order on the CPU (nlml_heads_train_steps_host; csrc/heads_train_ref.h) and returns the
device's bits for the same table.
"""
from __future__ import annotations

import math
import os

import numpy as np

from . import _lib, synth
from .weights import HEAD_NAMES

HEADS_WIDTHS = _lib.HEADS_WIDTHS
_STREAM_INIT = 7        # Philox stream ids next to synth's (0..4) and EncoderTrainer's (5, 6); the three networks draw in turn
_STREAM_SPLIT = 8
_STREAM_ORDER = 9
# the reference's settings: configs/config_MlpHeads.yaml there, and the rest from its code (:76,87,101,239)
DEFAULTS = {"epochs": 50, "batch_size": 256, "lr": 5e-3}
WEIGHT_DECAY = 1e-5
MAX_NORM = 1.0
STEP_SIZE = 10
GAMMA = 0.9
TEST_SIZE = 0.2


def param_count(R: int) -> int:
    total, fan_in = 0, int(R)
    for w in HEADS_WIDTHS:
        total += w * fan_in + w
        fan_in = w
    return total


def state_dict_views(buf, R: int) -> dict:
    """The state dict `model.{0,2,4,6,8}.{weight,bias}` as views of a params buffer W0,b0,...,W4,b4 (numpy or torch)."""
    sd, off, fan_in = {}, 0, int(R)
    for i, w in enumerate(HEADS_WIDTHS):
        sd[f"model.{2 * i}.weight"] = buf[off:off + w * fan_in].reshape(w, fan_in)
        off += w * fan_in
        sd[f"model.{2 * i}.bias"] = buf[off:off + w]
        off += w
        fan_in = w
    return sd


def flatten_state_dict(sd: dict) -> np.ndarray:
    return np.concatenate([np.asarray(sd[f"model.{2 * i}.{k}"], np.float32).ravel() for i in range(len(HEADS_WIDTHS)) for k in ("weight", "bias")])


def initial_state_dicts(ranks, seed: int = 0) -> dict:
    """kaiming_uniform_(nonlinearity='relu') weights, U(-sqrt(6 / fan_in), sqrt(6 / fan_in)) f32 [out,in], and zero biases for the
    three networks (ranks: their input widths, yaw, pitch, roll), drawn in turn from one Philox stream."""
    g = synth.rng(seed, _STREAM_INIT)
    out = {}
    for name, R in zip(HEAD_NAMES, ranks):
        sd, fan_in = {}, int(R)
        for i, width in enumerate(HEADS_WIDTHS):
            bound = math.sqrt(6.0 / fan_in)
            sd[f"model.{2 * i}.weight"] = synth._uniform_f32(g, (width, fan_in), -bound, bound)
            sd[f"model.{2 * i}.bias"] = np.zeros((width,), np.float32)
            fan_in = width
        out[name] = sd
    return out


def split_rows(rows, seed: int = 0, test_size: float = TEST_SIZE) -> dict:
    """train_test_split's sizes (ceil(test_size n) validation rows, the rest training rows) on one Philox permutation per network
    -> {name: (train i64[], val i64[])}; rows: the three row counts."""
    g = synth.rng(seed, _STREAM_SPLIT)
    out = {}
    for name, n in zip(HEAD_NAMES, rows):
        perm = g.permutation(int(n))
        n_val = int(math.ceil(test_size * int(n)))
        out[name] = (perm[n_val:], perm[:n_val])
    return out


def epoch_orders(n_train, epochs: int, seed: int = 0, shuffle: bool = True) -> dict:
    """{name: [i32[n_train] per epoch]}: the visiting orders (DataLoader(shuffle=True)), one Philox stream per network."""
    out = {}
    for h, (name, n) in enumerate(zip(HEAD_NAMES, n_train)):
        g = synth.rng(seed, _STREAM_ORDER + h)
        out[name] = [g.permutation(int(n)).astype(np.int32) if shuffle else np.arange(int(n), dtype=np.int32) for _ in range(epochs)]
    return out


def learning_rate_of_epoch(lr0: float, epoch: int, step_size: int = STEP_SIZE, gamma: float = GAMMA) -> float:
    """StepLR(step_size, gamma), stepped once after every epoch: the rate epoch `epoch` (from 0) trains with."""
    return float(lr0) * float(gamma) ** (epoch // int(step_size))


def _settings(config, overrides):
    cfg = {}
    if isinstance(config, (str, os.PathLike)):
        from .entrypoints import load_config
        cfg = load_config(config)
    elif config is not None:
        cfg = dict(config)
    hp = {}
    for key, default in DEFAULTS.items():
        v = overrides.get(key)
        hp[key] = type(default)(v if v is not None else cfg.get(key, default))
    return cfg, hp


def _host_table(cfg, optimized):
    """The table without a GPU: numpy's cos in float64 (the device's nlml_cosine_table may differ from it in a last bit)."""
    from .artefacts import angle_grid
    out = {}
    for name in HEAD_NAMES:
        b = cfg[f"{name}_bins"]
        ang = angle_grid(b["min_bin"], b["max_bin"], b["interval"])
        p = np.asarray(optimized[name], np.float64)
        out[name] = (p[:, 0] * np.cos(p[:, 1] * ang.astype(np.float64)[:, None] + p[:, 2]) + p[:, 3], ang)
    return out


class _HostBackend:
    """nlml_heads_*_host on numpy arrays."""

    def __init__(self, sets, params, R, device):
        self.R, self.sets = R, sets
        self.params = [p.copy() for p in params]
        self.state = [[np.zeros_like(p) for _ in range(3)] for p in params]   # grads, m, v
        self.best = [p.copy() for p in params]

    def _call(self, which, orders, batch, lr, step0):
        """One host call for the three networks on their training (orders given) or validation rows -> (loss, norm, status)."""
        arr = (_lib.HeadsNet * 3)()
        loss, norm, status = [], [], np.zeros(3, np.int32)
        for i, name in enumerate(HEAD_NAMES):
            x, y = self.sets[name][which]
            n = x.shape[0] if orders is None else len(orders[i])
            steps = (n + batch - 1) // batch
            loss.append(np.zeros(steps, np.float32))
            norm.append(np.zeros(steps, np.float32))
            a = arr[i]
            a.x, a.ldx, a.N, a.y = x.ctypes.data, x.shape[1], x.shape[0], y.ctypes.data
            a.params = self.params[i].ctypes.data
            a.grads, a.m, a.v = (s.ctypes.data for s in self.state[i])
            a.order, a.n, a.step0 = (orders[i].ctypes.data if orders is not None else None), n, step0[i]
            a.loss_out, a.norm_out, a.status = loss[i].ctypes.data, norm[i].ctypes.data, status[i:].ctypes.data
        L = _lib.lib()
        if orders is not None:
            _lib.check(L.nlml_heads_train_steps_host(arr, 3, self.R, batch, lr, WEIGHT_DECAY, MAX_NORM, None, 0), "nlml_heads_train_steps_host")
        else:
            _lib.check(L.nlml_heads_eval_losses_host(arr, 3, self.R, batch, None, 0), "nlml_heads_eval_losses_host")
        return loss, norm, int(status.max())

    def epoch(self, orders, batch, lr, step0):
        loss, norm, status = self._call("train", [np.ascontiguousarray(o, np.int32) for o in orders], batch, lr, step0)
        vloss, _, vstatus = self._call("val", None, batch, lr, step0)
        return loss, norm, vloss, status | vstatus

    def snapshot(self, i):
        self.best[i][:] = self.params[i]

    def host(self, i, best):
        return (self.best if best else self.params)[i].copy()


class _DeviceBackend:
    """K10 on the GPU: everything stays there; an epoch's losses come back in one copy."""

    def __init__(self, sets, params, R, device):
        import torch

        from . import ops
        self.torch, self.ops, self.R = torch, ops, R
        self.dev = torch.device(device) if device is not None else torch.device("cuda")
        self.sets = {name: {w: tuple(torch.as_tensor(a).to(self.dev) for a in xy) for w, xy in s.items()} for name, s in sets.items()}
        self.params = [torch.from_numpy(p).to(self.dev) for p in params]
        self.state = [[torch.zeros_like(p) for _ in range(3)] for p in self.params]
        self.best = [p.clone() for p in self.params]
        self.ws = None

    def epoch(self, orders, batch, lr, step0):
        torch, ops = self.torch, self.ops
        if self.ws is None:
            self.ws = torch.empty((_lib.lib().nlml_heads_train_workspace_bytes(self.R, batch, 3),), dtype=torch.uint8, device=self.dev)
        # one host-to-device copy for the three orders
        od = torch.from_numpy(np.concatenate(orders)).to(self.dev)
        cuts = np.cumsum([0] + [len(o) for o in orders])
        tnets, vnets = [], []
        for i, name in enumerate(HEAD_NAMES):
            (x, y), (xv, yv) = self.sets[name]["train"], self.sets[name]["val"]
            g, m, v = self.state[i]
            tnets.append(dict(x=x, y=y, params=self.params[i], grads=g, m=m, v=v, order=od[cuts[i]:cuts[i + 1]], step0=step0[i]))
            vnets.append(dict(x=xv, y=yv, params=self.params[i]))
        loss, norm, status = ops.heads_train_steps(tnets, batch=batch, lr=lr, weight_decay=WEIGHT_DECAY, max_norm=MAX_NORM, workspace=self.ws)
        vloss, vstatus = ops.heads_eval_losses(vnets, batch=batch, workspace=self.ws)
        # the epoch's one synchronisation: every figure of it in one device-to-host copy
        packed = torch.cat(loss + norm + vloss + [status.to(torch.float32), vstatus.to(torch.float32)]).cpu().numpy()
        out, at = [], 0
        for group in (loss, norm, vloss):
            piece = []
            for t in group:
                piece.append(packed[at:at + t.shape[0]])
                at += t.shape[0]
            out.append(piece)
        return out[0], out[1], out[2], int(packed[at:].max())

    def snapshot(self, i):
        self.best[i].copy_(self.params[i])   # device to device

    def host(self, i, best):
        return (self.best if best else self.params)[i].cpu().numpy()


def train_heads(trained_data="outputs/features/Trained_data.npz", config="configs/config_MlpHeads.yaml", *, out_dir="models", keep="best",
                backend="device", seed=0, epochs=None, batch_size=None, lr=None, shuffle=True, scheduler_step_size=STEP_SIZE, tables=None, initial=None,
                device=None, verbose=True):
    """Train the three heads as the reference's train_MlpHeads does and write {out_dir}/{yaw,pitch,roll}_network.pth
    -> ({name: state dict}, history).

    trained_data  Trained_data.npz (a path or a mapping with optimized_yaw, optimized_pitch, optimized_roll f64[R,4])
    config        configs/config_MlpHeads.yaml (a path or a mapping): the bin grids and epochs, batch_size, lr
    out_dir       where the three files go (None: nowhere)
    keep          "best": each network's weights at its lowest validation loss (the reference's stated intent);
                  "last": the last epoch's, which is what the reference's file really holds (its best_model_state aliases the
                  live tensors, NLML_HPE_MLPHeadsTrainer.py:119)
    backend       "device": K10 on the GPU;  "host": the same operation order on the CPU, the same bits for the same table
    seed          of the split, the epochs' permutations and the initial weights (synth's Philox generator; sklearn's and torch's
                  generator bits are not reproduced)
    epochs, batch_size, lr   None: the key of `config`, else the reference's 50, 256, 5e-3
    scheduler_step_size   of StepLR (the reference's 10; its gamma is 0.9)
    tables        {name: (U [n,R], angles [n])} instead of the table of `trained_data` (cast to float32 either way)
    initial       {name: state dict} instead of the Kaiming-uniform draw

    history: per network name dict(train_loss [epochs] the mean step loss, val_loss [epochs] the mean batch loss, step_loss /
    step_norm [epochs][steps], best_epoch (from 1), best_val_loss, saved_epoch), plus "lr" [epochs] and "split" {name: (train, val)}.
    A non-finite loss raises FloatingPointError naming the network, the epoch and the step."""
    if backend not in ("device", "host"):
        raise ValueError(f"backend: expected 'device' or 'host', got {backend!r}")
    if keep not in ("best", "last"):
        raise ValueError(f"keep: expected 'best' or 'last', got {keep!r}")
    cfg, hp = _settings(config, dict(epochs=epochs, batch_size=batch_size, lr=lr))
    batch = hp["batch_size"]
    if not 1 <= batch <= _lib.ENCODER_TRAIN_BATCH_MAX:
        raise ValueError(f"batch_size = {batch} outside [1, {_lib.ENCODER_TRAIN_BATCH_MAX}]")
    if tables is None:
        td = np.load(trained_data) if isinstance(trained_data, (str, os.PathLike)) else trained_data
        optimized = {name: np.asarray(td[f"optimized_{name}"], np.float64) for name in HEAD_NAMES}
        if backend == "device":
            from .artefacts import heads_training_table
            tables = {k: (U.cpu().numpy(), ang) for k, (U, ang) in heads_training_table(cfg, optimized, device=device or "cuda").items()}
        else:
            tables = _host_table(cfg, optimized)
    tables = {name: (np.ascontiguousarray(tables[name][0], dtype=np.float32), np.ascontiguousarray(tables[name][1], dtype=np.float32))
              for name in HEAD_NAMES}                                     # torch.tensor(.., dtype=torch.float32), :220-221
    ranks = [tables[name][0].shape[1] for name in HEAD_NAMES]
    R = ranks[0]
    if any(r != R for r in ranks) or not 1 <= R <= _lib.HEADS_TRAIN_R_MAX:
        raise ValueError(f"the tables have {ranks} columns: expected the same pose rank in [1, {_lib.HEADS_TRAIN_R_MAX}] for all three")
    for name in HEAD_NAMES:
        U, ang = tables[name]
        if U.ndim != 2 or ang.shape != (U.shape[0],) or U.shape[0] < 2:
            raise ValueError(f"{name}: expected a table [n,R] with n >= 2 angles, got {U.shape}, {ang.shape}")
    split = split_rows([tables[name][0].shape[0] for name in HEAD_NAMES], seed)
    sets = {name: {w: (np.ascontiguousarray(tables[name][0][idx]), np.ascontiguousarray(tables[name][1][idx]))
                   for w, idx in zip(("train", "val"), split[name])} for name in HEAD_NAMES}
    sds = initial if initial is not None else initial_state_dicts(ranks, seed)
    be = (_DeviceBackend if backend == "device" else _HostBackend)(sets, [flatten_state_dict(sds[name]) for name in HEAD_NAMES], R, device)
    n_train = [len(split[name][0]) for name in HEAD_NAMES]
    orders = epoch_orders(n_train, hp["epochs"], seed, shuffle)
    hist = {name: {"train_loss": [], "val_loss": [], "step_loss": [], "step_norm": [], "best_epoch": None, "best_val_loss": float("inf"),
                   "saved_epoch": None} for name in HEAD_NAMES}
    hist["lr"], hist["split"] = [], split
    step0 = [0, 0, 0]
    for epoch in range(hp["epochs"]):
        lr_e = learning_rate_of_epoch(hp["lr"], epoch, scheduler_step_size)
        loss, norm, vloss, status = be.epoch([orders[name][epoch] for name in HEAD_NAMES], batch, lr_e, step0)
        if status:
            raise ValueError(f"epoch {epoch + 1}: a row index lies outside its table (status {status})")
        hist["lr"].append(lr_e)
        for i, name in enumerate(HEAD_NAMES):
            for what, arr in (("training", loss[i]), ("validation", vloss[i])):
                bad = np.flatnonzero(~np.isfinite(arr))
                if bad.size:
                    raise FloatingPointError(f"{name}, epoch {epoch + 1}: the {what} loss of step {int(bad[0])} is {arr[bad[0]]}")
            step0[i] += len(loss[i])
            h = hist[name]
            train_mean = float(sum(float(v) for v in loss[i])) / len(loss[i])    # the reference sums the steps' .item()s (:103,115)
            val_total = float(sum(float(v) for v in vloss[i]))
            h["train_loss"].append(train_mean)
            h["val_loss"].append(val_total / len(vloss[i]))
            h["step_loss"].append(np.array(loss[i]))
            h["step_norm"].append(np.array(norm[i]))
            if verbose:
                print(f"{name}: Epoch {epoch + 1}/{hp['epochs']} - Train Loss: {train_mean:.4f}, Val Loss: {val_total / len(vloss[i]):.4f}")
            if val_total < h["best_val_loss"] * len(vloss[i]):
                h["best_val_loss"], h["best_epoch"] = val_total / len(vloss[i]), epoch + 1
                be.snapshot(i)
    out = {}
    for i, name in enumerate(HEAD_NAMES):
        saved_best = keep == "best" and hist[name]["best_epoch"] is not None
        hist[name]["saved_epoch"] = hist[name]["best_epoch"] if saved_best else hp["epochs"]
        out[name] = {k: np.array(v) for k, v in state_dict_views(be.host(i, saved_best), R).items()}
    if out_dir is not None:
        import torch
        os.makedirs(out_dir, exist_ok=True)
        for name in HEAD_NAMES:
            torch.save({k: torch.from_numpy(v.copy()) for k, v in out[name].items()}, os.path.join(out_dir, f"{name}_network.pth"))
            if verbose:
                print(f"Best Model Saved for {name} at Epoch {hist[name]['best_epoch']}"
                      + ("" if keep == "best" else f" (the file holds epoch {hp['epochs']}, as the reference's does)"))
    return out, hist
