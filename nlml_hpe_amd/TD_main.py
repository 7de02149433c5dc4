"""The training entry point behind the root TD_main.py -- the reference's TD_main.py:105-262 and its validation block (:347-433).

  1. compose the rotation training tensor from the identities' base landmarks (K6, CreateTensor.Compose_Tensor)
  2. decompose it, fit the pose factors' cosines and write Factor_Matrices.npz and Trained_data.npz (K7, K8,
     tucker_decompose.train_to_npz)
  3. print the reconstruction error |X - X_hat| / |X| of the artefacts AS WRITTEN -- the f32 W and the f32 factors read back from the
     two files -- measured in one pass over the tensor (K11, tucker_decompose.reconstruction_error)
  4. validate if asked: one random grid cell per validation identity, its landmarks from the per-face K6 call, one Test_batch over
     all of them, the reference's four MAE lines
  5. write <out-dir>/TD_main_report.json

What differs from the reference: the identities come from a landmark file (--base-landmarks, f32[I,468,3]) instead of image folders,
the validation picks are seeded (the reference's random.choice is not), and the matplotlib monitoring block (:270-333) is not built.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import time

import numpy as np

from . import entrypoints, tucker_decompose
from . import IntrinsicRotation as IR

REPORT_NAME = "TD_main_report.json"
MATRIX_NAMES = ("U_id", "yaw", "pitch", "roll")       # the reference's labels of the four unfoldings (:188)


def _parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base-landmarks", required=True, metavar="FILE",
                    help=".npy / .npz ('landmarks') f32[I,468,3]: every identity's landmarks at pose (0, 0, 0); replaces the image "
                         "folders of the reference's train_set_path")
    ap.add_argument("--use_rotation_features", type=int, default=1,
                    help="1 (default): the tensor is the base landmarks rotated to every bin; 0 is refused as Compose_Tensor refuses it")
    ap.add_argument("--perform_validation", choices=["tr", "fl"], help="tr: validate after training; fl (or absent): do not")
    ap.add_argument("--config", default="configs/config_TD_main.yaml")
    ap.add_argument("--out-dir", default="outputs/features")
    ap.add_argument("--tensor-file", metavar="NPY",
                    help="the reference's tensor cache: loaded if it exists, else the composed tensor is saved there; without the "
                         "option nothing is cached")
    ap.add_argument("--print-singular-values", action="store_true",
                    help="print every singular value of the four unfoldings with its energy (the reference's print_singular_values)")
    ap.add_argument("--backend", choices=["device", "numpy"], default="device",
                    help="device: K6, K7, K8 and K11 on the GPU; numpy: their host forms (no GPU involved).  The two validation "
                         "kernels -- the per-face rotation and the Powell estimator behind Test_batch -- run on the device whatever "
                         "the backend")
    ap.add_argument("--seed", type=int, default=0, help="seed of the validation picks")
    ap.add_argument("--val-base-landmarks", metavar="FILE", help="f32[V,468,3]: the validation identities (needed with --perform_validation tr)")
    ap.add_argument("--identities-from-file", action="store_true",
                    help="take the identity count from --base-landmarks; without it a config I_identity that differs is an error")
    return ap


def _bins(config):
    return [tucker_decompose._bins(config[k]) for k in ("yaw_bins", "pitch_bins", "roll_bins")]


def _tables(bins):
    """The matrix tables of the grid in the reference's expressions: yaw about y, pitch about x, roll about z -> three f64[n,3,3]."""
    return [np.ascontiguousarray(IR.rotation_matrices(axis, vals), np.float64) for axis, vals in zip(("y", "x", "z"), bins)]


def compose(base, tensor_shape, bins, use_rotation_features=1, backend="device"):
    """Step 1 -> the tensor f32[I,ny,np,nr,1404]: a device tensor (K6) or, backend "numpy", a host array from K6's host form, which
    returns the device's bits."""
    from . import CreateTensor

    if backend == "device" or use_rotation_features != 1:      # the refusal of use_rotation_features=0 is Compose_Tensor's
        return CreateTensor.Compose_Tensor(base, tensor_shape, *bins, None, use_rotation_features)[0]
    from . import _lib
    base = np.ascontiguousarray(base, np.float32)
    shape = (base.shape[0],) + tuple(len(b) for b in bins) + (1404,)
    if tuple(int(s) for s in tensor_shape) != shape:
        raise ValueError(f"tensor_shape {tuple(tensor_shape)} disagrees with the inputs: {shape[0]} identities and "
                         f"{shape[1]} x {shape[2]} x {shape[3]} bins of 1404 features give {shape}")
    zero = [CreateTensor._zero_bin(list(b), n) for b, n in zip(bins, ("yaw", "pitch", "roll"))]
    t = _tables(bins)
    out = np.zeros(shape, np.float32)
    _lib.check(_lib.lib().nlml_compose_rotation_tensor_host(base.ctypes.data, shape[0], t[0].ctypes.data, shape[1], t[1].ctypes.data,
                                                            shape[2], t[2].ctypes.data, shape[3], _lib.ROT_INTRINSIC, *zero,
                                                            out.ctypes.data, None), "nlml_compose_rotation_tensor_host")
    return out


def validation_picks(count, bins, seed):
    """One grid cell (yaw bin, pitch bin, roll bin) per validation identity from random.Random(seed), identity after identity, yaw
    then pitch then roll -> i64[count,3]."""
    rng = random.Random(seed)
    return np.array([[rng.randrange(len(b)) for b in bins] for _ in range(count)], np.int64).reshape(count, 3)


def validation_landmarks(val_base, picks, bins):
    """The picked cells' landmarks f32[V,1404] on the device: the per-face K6 call with the cell's three matrices in the intrinsic
    application order (pitch, yaw, roll), taken from the grid's own tables."""
    import torch

    from . import ops
    ty, tp, tr = _tables(bins)
    rot = np.ascontiguousarray(np.stack([tp[picks[:, 1]], ty[picks[:, 0]], tr[picks[:, 2]]], axis=1))
    lm = IR._landmarks(val_base, 3).to(IR._dev())
    out = ops.rotate_landmarks(lm, torch.from_numpy(rot).to(lm.device))
    return out.reshape(out.shape[0], -1)


def validate(val_base, artefacts, bins, seed):
    """Step 4 -> the report's validation entry; prints the reference's four MAE lines (:430-433)."""
    from . import TD_Tester

    picks = validation_picks(val_base.shape[0], bins, seed)
    x = validation_landmarks(val_base, picks, bins)
    W = artefacts["W"]
    deg = TD_Tester.Test_batch(W, x, W.shape[0], artefacts["optimized_yaw"][0:3], artefacts["optimized_pitch"][0:3],
                               artefacts["optimized_roll"][0:3])
    pred = np.round(deg, 3)                                                       # round(est, 3), :412
    true = np.stack([np.asarray(b, np.float64)[picks[:, k]] for k, b in enumerate(bins)], axis=1)
    mae = np.mean(np.abs(true - pred), axis=0)
    total = float((mae[0] + mae[1] + mae[2]) / 3)
    print(f"MAE (Yaw): {mae[0]}")
    print(f"MAE (Pitch): {mae[1]}")
    print(f"MAE (Roll): {mae[2]}")
    print(f"Total MAE: {total}")
    return {"seed": seed, "picks": picks.tolist(), "true_deg": true.tolist(), "pred_deg": pred.tolist(),
            "mae_yaw": float(mae[0]), "mae_pitch": float(mae[1]), "mae_roll": float(mae[2]), "mae_total": total}


def main(argv=None):
    args = _parser().parse_args(argv)
    config = entrypoints.load_config(args.config)
    validation = args.perform_validation == "tr"
    if validation and not args.val_base_landmarks:
        raise ValueError("--perform_validation tr needs --val-base-landmarks FILE (f32[V,468,3])")
    base = entrypoints.load_landmarks(args.base_landmarks)
    ts = config["tensor_shape"]
    if base.shape[0] != ts["I_identity"] and not args.identities_from_file:
        raise ValueError(f"{args.config} sets I_identity = {ts['I_identity']} but {args.base_landmarks} holds {base.shape[0]} "
                         "identities; make them agree or pass --identities-from-file")
    bins = _bins(config)
    tensor_shape = (base.shape[0], ts["I_yaw"], ts["I_pitch"], ts["I_roll"], ts["I_features"])

    # ---- step 1 ----
    start = time.time()
    if args.tensor_file and os.path.exists(args.tensor_file):
        if args.use_rotation_features != 1:
            compose(base, tensor_shape, bins, args.use_rotation_features, args.backend)
        tensor = np.load(args.tensor_file)
        if tuple(tensor.shape) != tensor_shape or tensor.dtype != np.float32:
            raise ValueError(f"{args.tensor_file} holds {tensor.dtype}{tuple(tensor.shape)}; the inputs give float32{tensor_shape}")
        print("Tensor loaded from disk.")
    else:
        tensor = compose(base, tensor_shape, bins, args.use_rotation_features, args.backend)
        if args.tensor_file:
            os.makedirs(os.path.dirname(os.path.abspath(args.tensor_file)), exist_ok=True)
            np.save(args.tensor_file, tucker_decompose._to_numpy(tensor))
            print(f"Tensor saved to {args.tensor_file}.")
    print(f"Time taken: {time.time() - start} seconds")
    if args.backend == "device" and not hasattr(tensor, "detach"):
        tensor = tucker_decompose._DeviceBackend(tensor).X

    report = {"tensor_shape": list(tensor_shape), "ranks": dict(config["tensor_decom_ranks"]), "backend": args.backend}
    if args.print_singular_values:
        values, energies = tucker_decompose.singular_values(tensor, backend=args.backend)
        for name, s, e in zip(MATRIX_NAMES, values, energies):
            for i in range(len(s)):
                print(f"Singular value {i + 1} of {name}: {s[i]}, Energy: {e[i]:.2f}%")
            print("\n")
        report["singular_values"] = {n: s.tolist() for n, s in zip(MATRIX_NAMES, values)}
        report["energies"] = {n: e.tolist() for n, e in zip(MATRIX_NAMES, energies)}

    # ---- step 2 ----
    start = time.time()
    _, _, _, errors = tucker_decompose.train_to_npz(tensor, config, args.out_dir, backend=args.backend, return_errors=True)
    print("Tensor successfully decomposed.")
    print("Training successfully completed!")
    print(f"Time taken: {time.time() - start} seconds")
    report["sweep_errors"] = [float(e) for e in errors]

    # ---- step 3: the error of what the files hold ----
    from . import weights
    start = time.time()
    art = weights.load_tucker_artefacts(args.out_dir)
    factors = [art[k] for k in ("U_id", "U_yaw", "U_pitch", "U_roll")]
    err, res_id = tucker_decompose.reconstruction_error(tensor, art["W"], factors, backend=args.backend, per_identity=True)
    print(f"Reconstruction Error: {err}")
    print(f"Time taken: {time.time() - start} seconds")
    print("Shape of W:", tuple(art["W"].shape))
    worst = np.argsort(-res_id, kind="stable")[:5]
    report["reconstruction_error"] = err
    report["worst_identities"] = [{"identity": int(i), "sum_squared_residual": float(res_id[i])} for i in worst]

    # ---- step 4 ----
    if validation:
        start = time.time()
        val_base = entrypoints.load_landmarks(args.val_base_landmarks)
        report["validation"] = validate(val_base, art, bins, args.seed)
        print(f"Time taken: {(time.time() - start) / val_base.shape[0]} seconds per validation identity")

    # ---- step 5 ----
    path = os.path.join(args.out_dir, REPORT_NAME)
    with open(path, "w") as f:
        json.dump(report, f, indent=1)
    print(f"Report written to {path}.")
    return report
