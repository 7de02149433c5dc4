#!/usr/bin/env python3
"""Train the landmark encoder and write models/Encoder.pth -- MI355X counterpart of the reference's NLML_HPE_EncoderTrainer.py
(train_encoder(), :294): the training loop runs on the GPU as K9 (nlml_hpe_amd/EncoderTrainer.py, csrc/encoder_train.hip).

    python NLML_HPE_EncoderTrainer.py                                  # data/train_dataset.pth, data/val_dataset.pth (the reference's files)
    python NLML_HPE_EncoderTrainer.py --from-base-landmarks train.npy val.npy
                                                                       # f32[I,468,3] each: both rotation tensors are composed first (K6)

The targets come from outputs/features/Factor_Matrices.npz (TD_main's output; nlml_hpe_amd.tucker_decompose.train_to_npz writes it),
the bins and the optional training keys (batch_size, num_epochs, learning_rate, weight_decay, scheduler_step_size) from
configs/config_EncoderTrainer.yaml; the command line overrides them.
"""
from __future__ import annotations

import argparse

import numpy as np

from nlml_hpe_amd import EncoderTrainer
from nlml_hpe_amd.entrypoints import load_config, load_landmarks


def _bins(spec):
    return np.arange(spec["min_bin"], spec["max_bin"], spec["interval"])


def train_encoder(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--from-base-landmarks", nargs=2, metavar=("TRAIN", "VAL"),
                    help="base landmarks f32[I,468,3] (.npy / .npz) of the training and the validation identities")
    ap.add_argument("--trainset", default="data/train_dataset.pth")
    ap.add_argument("--valset", default="data/val_dataset.pth")
    ap.add_argument("--factors", default="outputs/features/Factor_Matrices.npz")
    ap.add_argument("--config", default="configs/config_EncoderTrainer.yaml")
    ap.add_argument("--out", default="models/Encoder.pth")
    ap.add_argument("--batch-size", type=int)
    ap.add_argument("--epochs", type=int)
    ap.add_argument("--lr", type=float)
    ap.add_argument("--weight-decay", type=float)
    ap.add_argument("--scheduler-step-size", type=int)
    ap.add_argument("--zero-grad", action="store_true", help="plain SGD instead of the reference's accumulating gradient")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--backend", choices=["device", "host"], default="device")
    args = ap.parse_args(argv)

    train, val = args.trainset, args.valset
    if args.from_base_landmarks:
        from nlml_hpe_amd import CreateTensor
        cfg = load_config(args.config)
        yaw, pitch, roll = (_bins(cfg[k]) for k in ("yaw_bins", "pitch_bins", "roll_bins"))
        sets = []
        for path in args.from_base_landmarks:
            base = load_landmarks(path)
            shape = (base.shape[0], len(yaw), len(pitch), len(roll), 1404)
            sets.append(CreateTensor.Compose_Tensor(base, shape, yaw, pitch, roll)[0])
        train, val = sets
    best, hist = EncoderTrainer.train_encoder(train, val, args.factors, batch_size=args.batch_size, num_epochs=args.epochs,
                                              learning_rate=args.lr, weight_decay=args.weight_decay,
                                              scheduler_step_size=args.scheduler_step_size, zero_grad=args.zero_grad, seed=args.seed,
                                              backend=args.backend, config=args.config, out_path=args.out)
    return best, hist


if __name__ == "__main__":
    train_encoder()
