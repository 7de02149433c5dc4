"""K1c timing: nlml_normalize_centroid against nlml_normalize_ipd (the yardstick: same bytes per face, same box, same run).

    python tools/time_centroid.py [--faces 65536] [--reps 30] [--inner 10] [--out profiles/k1c_centroid.md]

Both kernels through the C ABI into buffers allocated once, on 65,536 faces (368 MB in, 368 MB out: beyond every cache).  After
warm-up the two are timed ALTERNATELY in one process -- ipd, centroid, ipd, ... -- each measurement a pair of device events around
`inner` back-to-back launches, so clock and thermal drift fall on both alike; the median per launch is reported.  Writes faces/s,
TB/s of algorithmic traffic (11,232 B per face for both), the fraction of the 8 TB/s HBM peak and the ratio of the two as a
markdown table, and prints the same numbers as one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlml_hpe_amd import _lib, synth  # noqa: E402

HBM_BYTES_PER_S = 8.0e12            # MI355X HBM3E peak
BYTES_PER_FACE = 2 * 1404 * 4       # f32 landmarks read, f32 features written


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "k1c_centroid.md"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B = args.faces
    L = _lib.lib()
    raw = torch.from_numpy(synth.raw_landmarks(B, seed=1)).to(dev)
    out = torch.empty((B, 1404), dtype=torch.float32, device=dev)
    valid = torch.empty((B,), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def ipd():
        _lib.check(L.nlml_normalize_ipd(raw.data_ptr(), B, 1, out.data_ptr(), valid.data_ptr(), stream), "nlml_normalize_ipd")

    def centroid():
        _lib.check(L.nlml_normalize_centroid(raw.data_ptr(), B, out.data_ptr(), valid.data_ptr(), None, stream), "nlml_normalize_centroid")

    kernels = {"normalize_ipd": ipd, "normalize_centroid": centroid}
    for _ in range(args.warmup):
        for fn in kernels.values():
            for _ in range(args.inner):
                fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in kernels}
    for _ in range(args.reps):
        for name, fn in kernels.items():            # alternately
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / args.inner)
    res = {"faces": B, "reps": args.reps, "inner": args.inner, "bytes_per_face": BYTES_PER_FACE, "device": torch.cuda.get_device_name(dev)}
    for name, v in ms.items():
        t = float(np.median(v)) * 1e-3
        res[name] = {"us": round(t * 1e6, 2), "us_min": round(min(v) * 1e3, 2), "us_max": round(max(v) * 1e3, 2),
                     "faces_per_s": round(B / t), "TB_per_s": round(B * BYTES_PER_FACE / t / 1e12, 3),
                     "hbm_peak_fraction": round(B * BYTES_PER_FACE / t / HBM_BYTES_PER_S, 3)}
    res["centroid_over_ipd_time"] = round(res["normalize_centroid"]["us"] / res["normalize_ipd"]["us"], 3)
    print(json.dumps(res), flush=True)

    lines = ["# K1c: centroid normalisation against the IPD kernel", "",
             f"`python tools/time_centroid.py --faces {B} --reps {args.reps} --inner {args.inner}` on {res['device']}: both kernels timed",
             f"alternately in one process, device events around {args.inner} back-to-back launches, median of {args.reps}.",
             f"{BYTES_PER_FACE:,} algorithmic bytes per face for both; HBM peak taken as 8 TB/s.", "",
             "| kernel | us per launch (min .. max) | faces/s | TB/s | of HBM peak |", "|---|---|---|---|---|"]
    for name in kernels:
        r = res[name]
        lines.append(f"| `nlml_{name}` | {r['us']} ({r['us_min']} .. {r['us_max']}) | {r['faces_per_s']:,} | {r['TB_per_s']} | {r['hbm_peak_fraction']:.1%} |")
    lines += ["", f"Time ratio centroid / ipd: **{res['centroid_over_ipd_time']}**", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
