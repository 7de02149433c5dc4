"""K11 timing: the expand-and-compare pass at the reference's shape against K7c, which reads the same tensor.

    python tools/tucker_residual_time.py [--identities 1620] [--reps 20] [--warmup 3] [--json PATH]
                                         [--td-main]

The tensor is composed on the device from synthetic landmarks: (1620, 11, 9, 7, 1404) f32 = 6.3 GB.  K11 (sums only), K7c
(nlml_project_identity, f64 out) and K11's other forms are timed ALTERNATELY in one process: after the warm-up calls every round
measures each of them once, a pair of device events around one call of the ops.* wrapper (workspace and output allocation from
torch's caching allocator included -- no device allocation after warm-up); the medians are reported with min and max.  The bound of
the forms that only read X is its bytes over 6.3 TB/s; the forms that write X_hat move twice the bytes.
--td-main also runs nlml_hpe_amd.TD_main.main end to end on those identities (landmarks and outputs in a temporary directory) and
reports its wall clock beside the decomposition's alone.
Prints one JSON line (and writes it to --json)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlml_hpe_amd import CreateTensor as CT  # noqa: E402
from nlml_hpe_amd import TD_main, ops, synth  # noqa: E402
from nlml_hpe_amd import tucker_decompose as TD  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
YAW, PITCH, ROLL = np.arange(-50, 51, 10), np.arange(-40, 41, 10), np.arange(-30, 31, 10)
RANK = [5, 3, 3, 3, 1404]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--identities", type=int, default=1620)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json")
    ap.add_argument("--td-main", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    I = args.identities
    base = synth.raw_landmarks(I, seed=1)
    X, _ = CT.Compose_Tensor(base, (I, 11, 9, 7, 1404), YAW, PITCH, ROLL)
    A = X.reshape(I, -1)
    xbytes = X.numel() * 4
    W, U, errs = TD.tucker(X, RANK, return_errors=True)
    sums = ops.tucker_residual(X, W, *U)[0].cpu().numpy()

    cases = {
        "K11 tucker_residual, sums": (lambda: ops.tucker_residual(X, W, *U), xbytes),
        "K7c project_identity, X (f64 out)": (lambda: ops.project_identity(A, U[0], out_dtype=torch.float64), xbytes + 5 * A.shape[1] * 8),
        "K11 tucker_residual, sums + res_id": (lambda: ops.tucker_residual(X, W, *U, want_res_id=True), xbytes),
        "K11 tucker_residual, sums + X_hat": (lambda: ops.tucker_residual(X, W, *U, want_xhat=True), 2 * xbytes),
        "K11 tucker_to_tensor (expand only)": (lambda: ops.tucker_to_tensor(W, *U), xbytes),
    }
    for fn, _ in cases.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in cases}
    for _ in range(args.reps):
        for name, (fn, _) in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    res = {"identities": I, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(dev), "tensor_gb": round(xbytes / 1e9, 3),
           "norms_error": errs[-1], "residual_error": float(np.sqrt(sums[0] / sums[1])), "kernels": {}}
    for name, (_, nbytes) in cases.items():
        med = float(np.median(ms[name]))
        res["kernels"][name] = {"ms": round(med, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                                "bound_ms": round(nbytes / HBM_ACHIEVABLE * 1e3, 4), "of_achievable_hbm": round(nbytes / HBM_ACHIEVABLE * 1e3 / med, 3),
                                "tb_per_s": round(nbytes / med / 1e9, 3)}
    k = res["kernels"]
    res["k11_over_k7c"] = round(k["K11 tucker_residual, sums"]["ms"] / k["K7c project_identity, X (f64 out)"]["ms"], 3)

    walls = []
    for error in ("norms", "residual"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, e = TD.tucker(X, RANK, return_errors=True, error=error)
        torch.cuda.synchronize()
        walls.append({"error": error, "s": round(time.perf_counter() - t0, 4), "sweeps": len(e), "last": e[-1]})
    res["tucker_device"] = walls

    if args.td_main:
        del X, A
        torch.cuda.empty_cache()
        with tempfile.TemporaryDirectory() as tmp:
            np.save(os.path.join(tmp, "base.npy"), np.asarray(base, np.float32))
            argv = ["--base-landmarks", os.path.join(tmp, "base.npy"), "--identities-from-file", "--out-dir", os.path.join(tmp, "out")]
            runs = []
            for more in ([], ["--perform_validation", "tr", "--val-base-landmarks", os.path.join(tmp, "base.npy")]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                report = TD_main.main(argv + more)
                torch.cuda.synchronize()
                runs.append({"validation": bool(more), "s": round(time.perf_counter() - t0, 3), "reconstruction_error": report["reconstruction_error"]})
            res["td_main"] = runs
    line = json.dumps(res)
    print(line, flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
