"""Training of the landmark encoder (the reference's NLML_HPE_EncoderTrainer.py), on the device.

The reference's ``train_encoder`` (:294-539) trains the encoder K2 runs -- Linear(F,1024) ReLU .. Linear(128,64) Tanh Linear(64,9)
-- to map a landmark row onto the rows of the Tucker pose factors that belong to its (yaw, pitch, roll) bins: SGD on the sum of
three MSELoss means, gradients accumulated WITHOUT zero_grad and clipped in place by clip_grad_norm_(20), StepLR(gamma 0.9) once
per epoch, a validation pass after every epoch, the parameters of the best validation total saved as models/Encoder.pth.  Here a
whole epoch of steps is ONE call of K9 (ops.encoder_train_steps, csrc/encoder_train.hip) and the validation pass another
(ops.encoder_eval_losses); the host synchronises once per epoch, to read the epoch's losses, decide the snapshot (a device-to-device
copy) and print the reference's two lines.

Both of the trainer's inputs are produced on the device by the links before it: the training rows are the rotation tensor of
CreateTensor.Compose_Tensor (K6) viewed as rows, one per cell (identity, yaw bin, pitch bin, roll bin) with the cell's bins as its
labels, and the targets are the rows of U_yaw, U_pitch, U_roll from tucker_decompose (K7).  The reference's own dataset files
(data/train_dataset.pth: torch.save((data, labels))) are read too.

``backend="host"`` runs the same operation order on the CPU (nlml_encoder_train_steps_host; csrc/encoder_train_ref.h): close to the
device's result, not its bits (the two tanh differ).

The initial weights (the reference's ``nn.init.uniform_(w, 1e-5, 1e-3)``, zero biases, :46-54) and the epochs' permutations
(DataLoader(shuffle=True)) come from synth's Philox generator, so a run is reproducible from its seed on any machine; the bits of
torch's own generator are not reproduced.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib, synth

ENCODER_WIDTHS = synth.ENCODER_WIDTHS
_STREAM_INIT = 5       # Philox stream ids next to synth's own (0..4)
_STREAM_ORDER = 6
# the reference's settings: configs/config_EncoderTrainer.yaml there, and max_norm / gamma from its code (:388,442)
DEFAULTS = {"batch_size": 256, "num_epochs": 100, "learning_rate": 1e-4, "weight_decay": 1e-5, "scheduler_step_size": 10}
MAX_NORM = 20.0
GAMMA = 0.9


def initial_state_dict(input_size: int = synth.F_REFERENCE, seed: int = 0) -> dict:
    """The reference's initialisation under its state-dict keys: weights U(1e-5, 1e-3) f32 [out,in], biases 0."""
    g = synth.rng(seed, _STREAM_INIT)
    sd, fan_in = {}, int(input_size)
    for i, width in enumerate(ENCODER_WIDTHS):
        sd[f"encoder.{2 * i}.weight"] = synth._uniform_f32(g, (width, fan_in), 1e-5, 1e-3)
        sd[f"encoder.{2 * i}.bias"] = np.zeros((width,), np.float32)
        fan_in = width
    return sd


def epoch_orders(n_rows: int, epochs: int, seed: int = 0, shuffle: bool = True) -> list:
    """The visiting order of every epoch, i32[n_rows] each: one permutation after the other from one Philox stream."""
    g = synth.rng(seed, _STREAM_ORDER)
    return [g.permutation(n_rows).astype(np.int32) if shuffle else np.arange(n_rows, dtype=np.int32) for _ in range(epochs)]


def learning_rate_of_epoch(lr0: float, epoch: int, step_size: int, gamma: float = GAMMA) -> float:
    """StepLR(step_size, gamma), stepped once after every epoch: the rate epoch `epoch` (from 0) trains with."""
    return float(lr0) * float(gamma) ** (epoch // int(step_size))


def flatten_state_dict(sd: dict) -> np.ndarray:
    """W0,b0,...,W5,b5 as one f32 vector: the layout of K9's params buffer."""
    return np.concatenate([np.asarray(sd[f"encoder.{2 * i}.{k}"], np.float32).ravel() for i in range(6) for k in ("weight", "bias")])


def state_dict_views(buf, input_size: int) -> dict:
    """The state dict as views of a params buffer in flatten_state_dict's layout (numpy or torch)."""
    sd, off, fan_in = {}, 0, int(input_size)
    for i, width in enumerate(ENCODER_WIDTHS):
        sd[f"encoder.{2 * i}.weight"] = buf[off:off + width * fan_in].reshape(width, fan_in)
        off += width * fan_in
        sd[f"encoder.{2 * i}.bias"] = buf[off:off + width]
        off += width
        fan_in = width
    return sd


def tensor_rows(tensor):
    """A composed rotation tensor [I,ny,np,nr,F] (torch or numpy) -> (x [I ny np nr, F] a view, labels i32 [rows,4] numpy): row
    r = ((i ny + y) np + p) nr + q carries the labels (y, p, q, i)."""
    if len(tensor.shape) != 5:
        raise ValueError(f"expected a tensor [I,ny,np,nr,F], got {tuple(tensor.shape)}")
    I, ny, npi, nr, F = (int(s) for s in tensor.shape)
    r = np.arange(I * ny * npi * nr, dtype=np.int64)
    labels = np.stack([(r // (npi * nr)) % ny, (r // nr) % npi, r % nr, r // (ny * npi * nr)], axis=1).astype(np.int32)
    return tensor.reshape(I * ny * npi * nr, F), labels


def load_dataset(path: str):
    """The reference's dataset file (save_dataset, :272-275): torch.save((data, labels)), data [N,F] float, labels [N,>=3] integer."""
    import torch
    data, labels = torch.load(path, map_location="cpu", weights_only=True)
    return data, labels


def _as_dataset(ds, what):
    """A dataset in any accepted form -> (x, labels): a path, a composed tensor, or the pair itself."""
    if isinstance(ds, (str, os.PathLike)):
        ds = load_dataset(os.fspath(ds))
    if isinstance(ds, (tuple, list)):
        if len(ds) != 2:
            raise ValueError(f"{what}: expected (x [N,F], labels [N,>=3])")
        return ds[0], ds[1]
    return tensor_rows(ds)


def _settings(config, overrides):
    """The five hyper-parameters: an explicit value, else the key of `config` (a mapping, or a path: a missing file holds no keys), else
    the reference's default."""
    cfg = {}
    if isinstance(config, (str, os.PathLike)):
        if os.path.exists(config):
            from .entrypoints import load_config
            cfg = load_config(config)
    elif config is not None:
        cfg = dict(config)
    out = {}
    for key, default in DEFAULTS.items():
        v = overrides.get(key)
        out[key] = type(default)(v if v is not None else cfg.get(key, default))
    return out


def _tables(factors):
    fm = np.load(factors) if isinstance(factors, (str, os.PathLike)) else factors
    tabs = [np.ascontiguousarray(np.asarray(fm[k]), dtype=np.float32) for k in ("U_yaw", "U_pitch", "U_roll")]   # float32(U[idx]), :408-410
    for k, t in zip(("U_yaw", "U_pitch", "U_roll"), tabs):
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError(f"{k}: expected [bins,3] (the encoder's latent is 3 x (1,3)), got {t.shape}")
    return tabs


class _HostBackend:
    """nlml_encoder_*_host on numpy arrays."""

    def __init__(self, train, val, tabs, params, device):
        self.sets = {}
        for name, (x, lab) in (("train", train), ("val", val)):
            x = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float32)
            lab = np.ascontiguousarray(lab.detach().cpu().numpy() if hasattr(lab, "detach") else lab).astype(np.int32)
            self.sets[name] = (x, lab)
        self.tabs = tabs
        self.params = params.copy()
        self.grads = np.zeros_like(self.params)
        self.best = self.params.copy()

    def _data(self, name):
        x, lab = self.sets[name]
        return [x.ctypes.data, x.shape[1], x.shape[0], lab.ctypes.data, lab.shape[1]] + [v for t in self.tabs for v in (t.ctypes.data, t.shape[0])]

    def epoch(self, order, batch, lr, wd, max_norm, zero_grad):
        x, _ = self.sets["train"]
        xv, _ = self.sets["val"]
        n, nv = len(order), xv.shape[0]
        loss, norm = np.zeros((n + batch - 1) // batch, np.float32), np.zeros((n + batch - 1) // batch, np.float32)
        vloss = np.zeros((nv + batch - 1) // batch, np.float32)
        status, vstatus = np.zeros(1, np.int32), np.zeros(1, np.int32)
        L = _lib.lib()
        _lib.check(L.nlml_encoder_train_steps_host(*self._data("train"), self.params.ctypes.data, self.grads.ctypes.data, x.shape[1], batch,
                                                   order.ctypes.data, n, lr, wd, max_norm, int(zero_grad), loss.ctypes.data, norm.ctypes.data,
                                                   status.ctypes.data), "nlml_encoder_train_steps_host")
        _lib.check(L.nlml_encoder_eval_losses_host(*self._data("val"), self.params.ctypes.data, x.shape[1], batch, None, nv, vloss.ctypes.data,
                                                   vstatus.ctypes.data), "nlml_encoder_eval_losses_host")
        return loss, norm, vloss, int(status[0]) | int(vstatus[0])

    def snapshot(self):
        self.best[:] = self.params

    def best_host(self):
        return self.best


class _DeviceBackend:
    """K9 on the GPU: everything stays there; an epoch's losses come back in one copy."""

    def __init__(self, train, val, tabs, params, device):
        import torch

        from . import ops
        self.torch, self.ops = torch, ops
        dev = torch.device(device) if device is not None else (train[0].device if hasattr(train[0], "is_cuda") and train[0].is_cuda
                                                                else torch.device("cuda"))
        self.dev = dev
        self.sets = {}
        for name, (x, lab) in (("train", train), ("val", val)):
            x = torch.as_tensor(x).to(dev, torch.float32)
            if x.stride(1) != 1:
                x = x.contiguous()
            self.sets[name] = (x, torch.as_tensor(lab).to(dev, torch.int32).contiguous())
        self.tabs = [torch.from_numpy(t).to(dev) for t in tabs]
        self.params = torch.from_numpy(params).to(dev)
        self.grads = torch.zeros_like(self.params)
        self.best = self.params.clone()
        self.ws = None

    def epoch(self, order, batch, lr, wd, max_norm, zero_grad):
        torch, ops = self.torch, self.ops
        x, lab = self.sets["train"]
        xv, labv = self.sets["val"]
        if self.ws is None:
            self.ws = torch.empty((_lib.lib().nlml_encoder_train_workspace_bytes(x.shape[1], batch),), dtype=torch.uint8, device=self.dev)
        loss, norm, status = ops.encoder_train_steps(x, lab, self.tabs, self.params, self.grads, order=torch.from_numpy(order).to(self.dev),
                                                     batch=batch, lr=lr, weight_decay=wd, max_norm=max_norm, zero_grad=zero_grad,
                                                     workspace=self.ws)
        vloss, vstatus = ops.encoder_eval_losses(xv, labv, self.tabs, self.params, batch=batch, workspace=self.ws)
        # the epoch's one synchronisation: every figure of it in one device-to-host copy
        packed = torch.cat([loss, norm, vloss, status.to(torch.float32), vstatus.to(torch.float32)]).cpu().numpy()
        s, v = loss.shape[0], vloss.shape[0]
        return packed[:s], packed[s:2 * s], packed[2 * s:2 * s + v], int(packed[2 * s + v]) | int(packed[2 * s + v + 1])

    def snapshot(self):
        self.best.copy_(self.params)   # device to device

    def best_host(self):
        return self.best.cpu().numpy()


def train_encoder(train="data/train_dataset.pth", val="data/val_dataset.pth", factors="outputs/features/Factor_Matrices.npz", *,
                  batch_size=None, num_epochs=None, learning_rate=None, weight_decay=None, scheduler_step_size=None, max_norm=MAX_NORM,
                  shuffle=True, zero_grad=False, seed=0, backend="device", device=None, config="configs/config_EncoderTrainer.yaml",
                  out_path="models/Encoder.pth", verbose=True):
    """Train the encoder as the reference's train_encoder does and write models/Encoder.pth -> (best state dict, history).

    train, val   a dataset each: (x f32[N,F], labels int[N,>=3]) (torch, on the device or not, or numpy), a composed rotation tensor
                 [I,ny,np,nr,F] (its rows are labelled by their cell), or the path of a reference dataset file
    factors      Factor_Matrices.npz (a path or a mapping with U_yaw, U_pitch, U_roll): the targets' tables
    batch_size, num_epochs, learning_rate, weight_decay, scheduler_step_size
                 None: the key of `config` (a path or a mapping; its training keys are optional), else the reference's default
                 (256, 100, 1e-4, 1e-5, 10)
    max_norm     of clip_grad_norm_ (the reference's 20);  shuffle: the reference's DataLoader(shuffle=True)
    zero_grad    False: the reference's loop, whose gradient accumulates across steps;  True: plain SGD
    seed         of the initial weights and the epochs' permutations (synth's Philox generator)
    backend      "device": K9 on the GPU;  "host": the same operation order on the CPU
    out_path     where the best state dict goes (None: nowhere)

    history: dict(train_loss [epochs] the mean step loss, val_loss [epochs] the mean batch loss, val_total [epochs], lr [epochs],
    step_loss / step_norm [epochs][steps], best_epoch (from 1), best_val_total, best_train_loss).
    A non-finite loss raises FloatingPointError naming the epoch and the step; a label or row index out of range raises ValueError."""
    if backend not in ("device", "host"):
        raise ValueError(f"backend: expected 'device' or 'host', got {backend!r}")
    hp = _settings(config, dict(batch_size=batch_size, num_epochs=num_epochs, learning_rate=learning_rate, weight_decay=weight_decay,
                           scheduler_step_size=scheduler_step_size))
    train, val = _as_dataset(train, "train"), _as_dataset(val, "val")
    F = int(train[0].shape[1])
    if F not in (136, synth.F_REFERENCE) or int(val[0].shape[1]) != F:
        raise ValueError(f"the datasets' rows have {F} and {int(val[0].shape[1])} features: expected 136 or 1404, the same for both")
    for name, (x, lab) in (("train", train), ("val", val)):
        if len(lab.shape) != 2 or lab.shape[0] != x.shape[0] or lab.shape[1] < 3 or x.shape[0] < 1:
            raise ValueError(f"{name}: expected x [N,F] with labels [N,>=3], got {tuple(x.shape)}, {tuple(lab.shape)}")
    batch = hp["batch_size"]
    if not 1 <= batch <= _lib.ENCODER_TRAIN_BATCH_MAX:
        raise ValueError(f"batch_size = {batch} outside [1, {_lib.ENCODER_TRAIN_BATCH_MAX}]")
    tabs = _tables(factors)
    be = (_DeviceBackend if backend == "device" else _HostBackend)(train, val, tabs, flatten_state_dict(initial_state_dict(F, seed)), device)
    n_train = int(train[0].shape[0])
    orders = epoch_orders(n_train, hp["num_epochs"], seed, shuffle)
    hist = {"train_loss": [], "val_loss": [], "val_total": [], "lr": [], "step_loss": [], "step_norm": [], "best_epoch": None,
            "best_val_total": float("inf"), "best_train_loss": float("inf")}
    for epoch in range(hp["num_epochs"]):
        lr = learning_rate_of_epoch(hp["learning_rate"], epoch, hp["scheduler_step_size"])
        loss, norm, vloss, status = be.epoch(orders[epoch], batch, lr, hp["weight_decay"], float(max_norm), bool(zero_grad))
        if status:
            raise ValueError(f"epoch {epoch + 1}: a row index or a label lies outside its range (status {status}: "
                             f"{_lib.ENCODER_TRAIN_CLAMPED_ORDER} = order, {_lib.ENCODER_TRAIN_CLAMPED_LABEL} = label)")
        for what, arr in (("training", loss), ("validation", vloss)):
            bad = np.flatnonzero(~np.isfinite(arr))
            if bad.size:
                raise FloatingPointError(f"epoch {epoch + 1}: the {what} loss of step {int(bad[0])} is {arr[bad[0]]}")
        train_mean = float(sum(float(v) for v in loss)) / len(loss)            # the reference sums the steps' .item()s (:453-459)
        val_total = float(sum(float(v) for v in vloss))
        hist["train_loss"].append(train_mean)
        hist["val_total"].append(val_total)
        hist["val_loss"].append(val_total / len(vloss))
        hist["lr"].append(lr)
        hist["step_loss"].append(np.array(loss))
        hist["step_norm"].append(np.array(norm))
        if verbose:
            print(f"Training - Epoch [{epoch + 1}/{hp['num_epochs']}] ------ Total Loss: {train_mean:.4f}")
            print(f"Validation - Epoch [{epoch + 1}/{hp['num_epochs']}] ------ Total Loss: {val_total / len(vloss):.4f} \n")
        if val_total <= hist["best_val_total"]:
            hist["best_val_total"], hist["best_train_loss"], hist["best_epoch"] = val_total, train_mean, epoch + 1
            be.snapshot()
    best = {k: np.array(v) for k, v in state_dict_views(be.best_host(), F).items()}
    if out_path is not None and hist["best_epoch"] is not None:
        import torch
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        torch.save({k: torch.from_numpy(v.copy()) for k, v in best.items()}, out_path)
        if verbose:
            print(f"Best Model Saved at Epoch {hist['best_epoch']} with train loss = {hist['best_train_loss']:.4f} "
                  f"and val loss = {hist['best_val_total'] / len(vloss):.4f}")
    return best, hist
