#!/usr/bin/env python3
"""Compose the rotation training tensor, Tucker-decompose it, fit the pose factors' cosines and write the two artefacts of the TD
path -- MI355X counterpart of the reference's TD_main.py, the entry point its README runs first (nlml_hpe_amd/TD_main.py; K6, K7, K8
and K11 on the GPU).

    python TD_main.py --base-landmarks base.npy                                   # -> outputs/features/{Factor_Matrices,Trained_data}.npz
    python TD_main.py --base-landmarks base.npy --perform_validation tr --val-base-landmarks val.npy --print-singular-values
    python TD_main.py --base-landmarks base.npy --identities-from-file --backend numpy --out-dir runs/td

The identities come from a landmark file (f32[I,468,3], pose (0, 0, 0)) instead of the reference's image folders; shape, ranks and
bins from configs/config_TD_main.yaml.  Prints the reference's lines (Reconstruction Error, Shape of W, the four MAE lines) and writes
<out-dir>/TD_main_report.json.  The reconstruction error is |X - X_hat| / |X| of the files as written, measured in one GPU pass.
"""
from nlml_hpe_amd import TD_main

if __name__ == "__main__":
    TD_main.main()
