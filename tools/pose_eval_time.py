"""K5 timing: metrics.evaluate (one native pass, two launches, one device-to-host copy) against the ATen path the test entry point
runs on the same device tensors (metrics.compute_errors + compute_interval_mae on the kept rows), at 65,536 and 1,048,576 faces.

    python tools/pose_eval_time.py [reps]

Device events around each form, after warm-up; the kernels alone (ops.pose_eval, no copy) are timed the same way.  The ATen path is
given its inputs already rounded and filtered (the numpy part of the host path is not counted), so its time is a lower bound.
Prints one JSON line per size."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlml_hpe_amd import metrics, ops  # noqa: E402
from nlml_hpe_amd.entrypoints import load_config  # noqa: E402

LO, HI = (-50.0, -40.0, -30.0), (51.0, 41.0, 31.0)
HBM_BYTES_PER_S = 8.0e12            # MI355X HBM3E peak
BYTES_PER_FACE = 12 + 1 + 24        # f32 pose, u8 valid, f64 GT


def _time(fn, reps: int, warm: int = 5) -> float:
    """median ms per call over `reps` event-timed calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main() -> None:
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    cfg = load_config("configs/config_NLML_HPE_Test.yaml")
    intervals = [[tuple(x) for x in cfg[k]] for k in ("yaw_intervals", "pitch_intervals", "roll_intervals")]
    flat = [(a, lo, hi) for a, ivs in enumerate(intervals) for lo, hi in ivs]
    for B in (65_536, 1_048_576):
        rng = np.random.default_rng(B)
        gt = rng.uniform((-52.0, -41.5, -31.0), (53.0, 42.5, 32.0), size=(B, 3))
        pose = np.radians(gt + rng.normal(0.0, 3.0, size=(B, 3))).astype(np.float32)
        valid = rng.random(B) >= 0.03
        dg, dp, dv = (torch.from_numpy(x).to(dev) for x in (gt, pose, valid))
        pred = np.round(np.degrees(pose.astype(np.float64)), 3)
        keep = ((gt >= np.array(LO)) & (gt <= np.array(HI))).all(axis=1) & valid
        gk, pk = torch.from_numpy(gt[keep]).to(dev), torch.from_numpy(pred[keep]).to(dev)

        t_kernels = _time(lambda: ops.pose_eval(dp, dg, dv, LO, HI, flat, 3), reps)
        t_eval = _time(lambda: metrics.evaluate(dp, dv, dg, LO, HI, intervals, verbose=False), reps)
        t_aten = _time(lambda: (metrics.compute_errors(gk, pk, verbose=False), metrics.compute_interval_mae(gk, pk, *intervals)), reps)
        bound_us = B * BYTES_PER_FACE / HBM_BYTES_PER_S * 1e6
        print(json.dumps({"faces": B, "kept": int(keep.sum()), "kernels_us": round(t_kernels * 1e3, 1),
                          "evaluate_us": round(t_eval * 1e3, 1), "aten_us": round(t_aten * 1e3, 1),
                          "speedup_evaluate_vs_aten": round(t_aten / t_eval, 1), "bytes_per_face": BYTES_PER_FACE,
                          "hbm_bound_us": round(bound_us, 2), "f64_sincos_per_face": 6, "f64_acos_per_face": 3}), flush=True)


if __name__ == "__main__":
    main()
