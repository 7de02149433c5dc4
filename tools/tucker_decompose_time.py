"""K7 timing: the Tucker decomposition's primitives and driver at the reference's shape, each against its own bound.

    python tools/tucker_decompose_time.py [--identities 1620] [--reps 20] [--warmup 3] [--numpy-seconds 40]
                                          [--out profiles/tucker_decompose.md]

The tensor is composed on the device by nlml_compose_rotation_tensor from synthetic landmarks: (1620, 11, 9, 7, 1404) f32 = 6.3 GB.
Every kernel is timed on its own: warm-up launches, then `reps` measurements, each a pair of device events around one call of the
ops.* wrapper (workspace allocation from torch's caching allocator included -- no device allocation after warm-up); the median is
reported with min and max.  Bounds:
  K7a         its upper-triangle floating-point operations I (I + 1) K over the 78.6 TFLOP/s f64 matrix peak
  K7b/K7c/K7d bytes read + written once over 6.3 TB/s, the achievable HBM rate (K6 writes the same tensor at 4.6 TB/s)
The eigen-solves (torch.linalg.eigh, f64, on the device) are timed separately, the whole tucker() call by wall clock around a
synchronised call, and backend="numpy" on this host's CPU at growing identity counts until one run exceeds the time budget; its
figure for the full shape is an EXTRAPOLATION (linear in the identity count) and labelled so.
Writes the markdown table and prints the same numbers as one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlml_hpe_amd import CreateTensor as CT  # noqa: E402
from nlml_hpe_amd import ops, synth  # noqa: E402
from nlml_hpe_amd import tucker_decompose as TD  # noqa: E402

F64_MATRIX_FLOPS = 78.6e12
HBM_ACHIEVABLE = 6.3e12
YAW, PITCH, ROLL = np.arange(-50, 51, 10), np.arange(-40, 41, 10), np.arange(-30, 31, 10)
RANK = [5, 3, 3, 3, 1404]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--identities", type=int, default=1620)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--numpy-seconds", type=float, default=40.0)
    ap.add_argument("--out", default=os.path.join("profiles", "tucker_decompose.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    I = args.identities
    base = synth.raw_landmarks(I, seed=1)
    X, _ = CT.Compose_Tensor(base, (I, 11, 9, 7, 1404), YAW, PITCH, ROLL)
    A = X.reshape(I, -1)
    K = A.shape[1]
    xbytes = X.numel() * 4

    _, U = TD.tucker(X, RANK, n_iter_max=0)
    # the driver keeps its projected tensors in f64 (out_dtype), so those forms are the ones timed
    f64 = torch.float64
    P = ops.project_pose(X, U[1], U[2], U[3], out_dtype=f64)
    Z = ops.project_identity(A, U[0], out_dtype=f64).reshape(5, 11, 9, 7, 1404)
    T = ops.project_pose(Z, None, U[2], U[3], out_dtype=f64)
    G_id = ops.mode_gram(A)

    # name -> (call, bound in seconds, what the bound is, work)
    flops = lambda i, k: i * (i + 1) * k                                      # noqa: E731  upper triangle, 2 flop per product
    cases = {
        "K7a mode_gram, X": (lambda: ops.mode_gram(A), flops(I, K) / F64_MATRIX_FLOPS, "f64 matrix peak", f"[{I}, {K:,}], {flops(I, K) / 1e12:.2f} TFLOP"),
        "K7a mode_gram, projected (f64 in)": (lambda: ops.mode_gram(P.reshape(I, -1)), flops(I, 27 * 1404) / F64_MATRIX_FLOPS, "f64 matrix peak",
                                     f"[{I}, {27 * 1404:,}], {flops(I, 27 * 1404) / 1e12:.3f} TFLOP"),
        "K7b pose_grams, X": (lambda: ops.pose_grams(X), xbytes / HBM_ACHIEVABLE, "HBM", f"{xbytes / 1e9:.2f} GB read"),
        "K7c project_identity, X (f64 out)": (lambda: ops.project_identity(A, U[0], out_dtype=f64), (xbytes + Z.numel() * 8) / HBM_ACHIEVABLE, "HBM",
                                              f"{xbytes / 1e9:.2f} GB read, {Z.numel() * 8 / 1e6:.0f} MB written"),
        "K7d project_pose, X, 3 factors (f64 out)": (lambda: ops.project_pose(X, U[1], U[2], U[3], out_dtype=f64),
                                                     (xbytes + P.numel() * 8) / HBM_ACHIEVABLE, "HBM",
                                                     f"{xbytes / 1e9:.2f} GB read, {P.numel() * 8 / 1e6:.0f} MB written"),
        "K7d project_pose, X, 3 factors (f32 out)": (lambda: ops.project_pose(X, U[1], U[2], U[3]), (xbytes + P.numel() * 4) / HBM_ACHIEVABLE, "HBM",
                                                     f"{xbytes / 1e9:.2f} GB read, {P.numel() * 4 / 1e6:.0f} MB written"),
        "K7d project_pose, Z, 2 factors (f64)": (lambda: ops.project_pose(Z, None, U[2], U[3], out_dtype=f64),
                                                 (Z.numel() + T.numel()) * 8 / HBM_ACHIEVABLE, "HBM", f"{Z.numel() * 8 / 1e6:.0f} MB read"),
        "K7b pose_grams, projected Z (f64 in)": (lambda: ops.pose_grams(T, which=(True, False, False)), T.numel() * 8 / HBM_ACHIEVABLE, "HBM",
                                                 f"{T.numel() * 8 / 1e6:.1f} MB read"),
    }
    res = {"identities": I, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev), "kernels": {}}
    for name, (fn, bound, what, work) in cases.items():
        r = timed(fn, args.reps, args.warmup)
        r.update(bound_ms=round(bound * 1e3, 4), bound=what, work=work, of_bound=round(bound * 1e3 / r["ms"], 3))
        res["kernels"][name] = r
    res["eigh"] = {f"{n} x {n}": timed(lambda G=G: torch.linalg.eigh(G), args.reps, args.warmup)
                   for n, G in ((I, G_id), (11, torch.eye(11, dtype=torch.float64, device=dev)))}

    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        W, _, errs = TD.tucker(X, RANK, return_errors=True)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    res["tucker_device"] = {"s": round(min(walls), 4), "s_all": [round(w, 4) for w in walls], "sweeps": len(errs), "error": errs[-1]}

    del P, T, G_id
    n, runs = 8, []
    while n <= I:
        Xh = X[:n].cpu().numpy()
        t0 = time.perf_counter()
        _, _, e = TD.tucker(Xh, RANK, backend="numpy", return_errors=True)
        runs.append({"identities": n, "s": round(time.perf_counter() - t0, 3), "sweeps": len(e)})
        if runs[-1]["s"] > args.numpy_seconds / 3:
            break
        n *= 2
    last = runs[-1]
    res["tucker_numpy"] = {"runs": runs, "extrapolated_s_full": round(last["s"] * I / last["identities"], 1)}
    print(json.dumps(res), flush=True)

    lines = ["# K7: the Tucker decomposition on the device, each kernel against its bound", "",
             f"`python tools/tucker_decompose_time.py --identities {I} --reps {args.reps} --warmup {args.warmup}` on {res['device']}: tensor",
             f"({I}, 11, 9, 7, 1404) f32 = {xbytes / 1e9:.2f} GB composed on the device; per kernel {args.warmup} warm-up calls, then the median of",
             f"{args.reps} measurements, each a pair of device events around one call.  Bounds: f64 matrix peak 78.6 TFLOP/s over the",
             "upper-triangle operations (K7a); bytes read + written once over 6.3 TB/s achievable HBM (K7b, K7c, K7d).", "",
             "| kernel | work | ms (min .. max) | bound, ms | bound / measured |", "|---|---|---|---|---|"]
    for name, r in res["kernels"].items():
        lines.append(f"| {name} | {r['work']} | {r['ms']} ({r['ms_min']} .. {r['ms_max']}) | {r['bound_ms']} ({r['bound']}) | {r['of_bound']:.1%} |")
    lines += ["", "Eigen-solves (`torch.linalg.eigh`, f64, on the device): " +
              "; ".join(f"{k}: {v['ms']} ms ({v['ms_min']} .. {v['ms_max']})" for k, v in res["eigh"].items()) + ".", "",
              f"The whole `tucker(X, [5, 3, 3, 3, 1404])` call (HOSVD + {res['tucker_device']['sweeps']} HOOI sweeps until the default tol, "
              f"relative error {res['tucker_device']['error']:.6f}): **{res['tucker_device']['s']} s** wall clock (three calls: {res['tucker_device']['s_all']}).", "",
              "`backend=\"numpy\"` on this host's CPUs (f64, the same driver): " +
              ", ".join(f"{r['identities']} identities {r['s']} s" for r in runs) +
              f".  EXTRAPOLATED linearly from the last run to {I} identities: {res['tucker_numpy']['extrapolated_s_full']} s "
              "(not run at the full shape: its f64 copy of the tensor alone is 12.6 GB).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
