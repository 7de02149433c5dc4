"""K6 timing: the rotation training tensor at the reference's full shape, with nlml_normalize_ipd (K1) as the yardstick in the same run.

    python tools/rotation_tensor_time.py [--identities 1620] [--faces 65536] [--reps 20] [--inner 5] [--ref-ms-per-cell 0.119]
                                         [--out profiles/rotation_tensor.md]

nlml_compose_rotation_tensor writes the reference's (1620, 11, 9, 7, 1404) f32 tensor -- 6.30 GB, beyond every cache -- from 9 MB of
landmarks; nlml_rotate_landmarks rotates 65,536 faces, one pose each; nlml_normalize_ipd normalises 65,536 faces.  All through the C
ABI into buffers allocated once.  After warm-up the three are timed ALTERNATELY in one process, each measurement a pair of device
events around `inner` back-to-back launches, so clock and thermal drift fall on all alike; the median per launch is reported with the
algorithmic bytes per second and the fraction of the 8 TB/s HBM peak.  Nobody has measured this kernel before, so there is no pass
mark: K1's fraction of the peak from the same run is the yardstick.  --ref-ms-per-cell is the reference's CPU time per tensor cell
as tests/golden/make_golden_rotation.py prints it for its 54 cells (measured on the build machine's CPU, not on this one); the table
extrapolates it to the full grid and says so.  Writes the markdown table and prints the same numbers as one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlml_hpe_amd import IntrinsicRotation as IR  # noqa: E402
from nlml_hpe_amd import _lib, synth  # noqa: E402

HBM_BYTES_PER_S = 8.0e12            # MI355X HBM3E peak
ROW = 1404 * 4                      # one face of f32 features
YAW, PITCH, ROLL = np.arange(-50, 51, 10), np.arange(-40, 41, 10), np.arange(-30, 31, 10)     # the reference's grid, 11 x 9 x 7


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--identities", type=int, default=1620)
    ap.add_argument("--faces", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-ms-per-cell", type=float, default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "rotation_tensor.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    I, B = args.identities, args.faces
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    raw = torch.from_numpy(synth.raw_landmarks(B, seed=1)).to(dev)
    base = raw[:I].contiguous() if I <= B else torch.from_numpy(synth.raw_landmarks(I, seed=1)).to(dev)
    tabs = [torch.from_numpy(IR.rotation_matrices(ax, v)).to(dev) for ax, v in (("y", YAW), ("x", PITCH), ("z", ROLL))]
    ny, np_, nr = (t.shape[0] for t in tabs)
    cells = I * ny * np_ * nr
    tensor = torch.empty((cells, 1404), dtype=torch.float32, device=dev)
    poses = synth.rng(12, 3).uniform(-60.0, 60.0, (B, 3))
    rot = torch.from_numpy(IR.pose_matrices(poses, "intrinsic")).to(dev)
    out = torch.empty((B, 1404), dtype=torch.float32, device=dev)
    valid = torch.empty((B,), dtype=torch.uint8, device=dev)

    def ipd():
        _lib.check(L.nlml_normalize_ipd(raw.data_ptr(), B, 1, out.data_ptr(), valid.data_ptr(), stream), "nlml_normalize_ipd")

    def compose():
        _lib.check(L.nlml_compose_rotation_tensor(base.data_ptr(), I, tabs[0].data_ptr(), ny, tabs[1].data_ptr(), np_, tabs[2].data_ptr(), nr,
                                                  _lib.ROT_INTRINSIC, 5, 4, 3, tensor.data_ptr(), None, stream), "nlml_compose_rotation_tensor")

    def faces():
        _lib.check(L.nlml_rotate_landmarks(raw.data_ptr(), rot.data_ptr(), out.data_ptr(), None, B, stream), "nlml_rotate_landmarks")

    # name -> (call, rows, bytes read + written per launch)
    kernels = {"normalize_ipd": (ipd, B, 2 * B * ROW),
               "compose_rotation_tensor": (compose, cells, cells * ROW + I * ROW),
               "rotate_landmarks": (faces, B, 2 * B * ROW + B * 27 * 8)}
    for _ in range(args.warmup):
        for fn, _, _ in kernels.values():
            for _ in range(args.inner):
                fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in kernels}
    for _ in range(args.reps):
        for name, (fn, _, _) in kernels.items():            # alternately
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / args.inner)
    res = {"identities": I, "grid": [int(ny), int(np_), int(nr)], "cells": cells, "faces": B, "reps": args.reps, "inner": args.inner,
           "device": torch.cuda.get_device_name(dev)}
    for name, (_, rows, nbytes) in kernels.items():
        t = float(np.median(ms[name])) * 1e-3
        res[name] = {"ms": round(t * 1e3, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4), "rows": rows,
                     "GB": round(nbytes / 1e9, 3), "GB_per_s": round(nbytes / t / 1e9, 1), "hbm_peak_fraction": round(nbytes / t / HBM_BYTES_PER_S, 3)}
    k1 = res["normalize_ipd"]["hbm_peak_fraction"]
    res["compose_over_k1_fraction"] = round(res["compose_rotation_tensor"]["hbm_peak_fraction"] / k1, 3)
    res["faces_over_k1_fraction"] = round(res["rotate_landmarks"]["hbm_peak_fraction"] / k1, 3)
    if args.ref_ms_per_cell is not None:
        res["reference_ms_per_cell"] = args.ref_ms_per_cell
        res["reference_s_extrapolated"] = round(args.ref_ms_per_cell * cells / 1e3, 1)
    print(json.dumps(res), flush=True)

    lines = ["# K6: the rotation training tensor against the IPD kernel", "",
             f"`python tools/rotation_tensor_time.py --identities {I} --faces {B} --reps {args.reps} --inner {args.inner}` on {res['device']}: the three",
             f"kernels timed alternately in one process, device events around {args.inner} back-to-back launches, median of {args.reps}.",
             "Bytes are algorithmic (read + written once); HBM peak taken as 8 TB/s.", "",
             "| kernel | work | ms per launch (min .. max) | GB moved | GB/s | of HBM peak |", "|---|---|---|---|---|---|"]
    work = {"normalize_ipd": f"{B:,} faces (K1, the yardstick)", "compose_rotation_tensor": f"({I}, {ny}, {np_}, {nr}, 1404) = {cells:,} cells",
            "rotate_landmarks": f"{B:,} faces, one pose each"}
    for name in kernels:
        r = res[name]
        lines.append(f"| `nlml_{name}` | {work[name]} | {r['ms']} ({r['ms_min']} .. {r['ms_max']}) | {r['GB']} | {r['GB_per_s']:,} | {r['hbm_peak_fraction']:.1%} |")
    lines += ["", f"Fraction of the peak relative to K1's in the same run: tensor **{res['compose_over_k1_fraction']}**, per-face mode "
              f"**{res['faces_over_k1_fraction']}**.", ""]
    if args.ref_ms_per_cell is not None:
        lines += [f"The reference's side: its own `Compose_Tensor` loop took {args.ref_ms_per_cell} ms per cell on the build machine's CPU for the 54 cells of",
                  f"FX12 (printed by `tests/golden/make_golden_rotation.py`); EXTRAPOLATED to {cells:,} cells that is {res['reference_s_extrapolated']} s.  It was",
                  "not run at the full shape.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
