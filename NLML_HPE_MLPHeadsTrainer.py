#!/usr/bin/env python3
"""Train the yaw, pitch and roll heads and write models/{yaw,pitch,roll}_network.pth -- MI355X counterpart of the reference's
NLML_HPE_MLPHeadsTrainer.py (train_MlpHeads(), :132): the three training loops run on the GPU as K10, every launch shared by the
three networks (nlml_hpe_amd/MLPHeadsTrainer.py, csrc/heads_train.hip).

    python NLML_HPE_MLPHeadsTrainer.py                         # outputs/features/Trained_data.npz -> models/*_network.pth
    python NLML_HPE_MLPHeadsTrainer.py --out-dir runs/heads --epochs 10 --keep last

The cosine curves come from outputs/features/Trained_data.npz (nlml_hpe_amd.tucker_decompose.train_to_npz writes it), the bin grids
and epochs, batch_size, lr from configs/config_MlpHeads.yaml; the command line overrides them.  --keep best (default) saves each
network at its lowest validation loss; --keep last saves the last epoch, which is what the reference's file really holds.
"""
from __future__ import annotations

import argparse

from nlml_hpe_amd import MLPHeadsTrainer


def train_MlpHeads(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trained-data", default="outputs/features/Trained_data.npz")
    ap.add_argument("--config", default="configs/config_MlpHeads.yaml")
    ap.add_argument("--out-dir", default="models")
    ap.add_argument("--epochs", type=int)
    ap.add_argument("--batch-size", type=int)
    ap.add_argument("--lr", type=float)
    ap.add_argument("--backend", choices=["device", "host"], default="device")
    ap.add_argument("--keep", choices=["best", "last"], default="best")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    return MLPHeadsTrainer.train_heads(args.trained_data, args.config, out_dir=args.out_dir, keep=args.keep, backend=args.backend,
                                       seed=args.seed, epochs=args.epochs, batch_size=args.batch_size, lr=args.lr)


if __name__ == "__main__":
    train_MlpHeads()
