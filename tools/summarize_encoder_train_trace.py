#!/usr/bin/env python3
"""Per-launch times of a K9 epoch from a rocprofv3 --kernel-trace CSV: the launches of one kernel are told apart by their grid size
(one size per layer), so the table is the step's fourteen launches.

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o k9 -- python tools/encoder_train_time.py --only k9 --repeats 1
    python tools/summarize_encoder_train_trace.py out/.../k9_kernel_trace.csv [--steps 1300]
"""
import argparse
import csv
from collections import defaultdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=int, default=1300, help="steps in the trace (warm-up epoch + one repeat of 650)")
    args = ap.parse_args()
    rows = defaultdict(list)
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("kernel_name") or ""
            if "et_" not in name and "mlp_" not in name:   # K9's own kernels, and the forward / backward kernels it shares with K10
                continue
            grid = r.get("Grid_Size_X") or r.get("Grid_Size") or r.get("grid_size_x") or "?"
            wg = r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or "?"
            rows[(name.split("(")[0].split("::")[-1], grid, wg)].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = 0.0
    print("| kernel | grid (threads) | workgroup | launches / step | mean us | us / step |")
    print("|---|---:|---:|---:|---:|---:|")
    for (name, grid, wg), ts in sorted(rows.items(), key=lambda kv: -sum(kv[1])):
        per_step = len(ts) / args.steps
        mean = sum(ts) / len(ts) / 1e3
        total += mean * per_step
        print(f"| {name} | {grid} | {wg} | {per_step:.2f} | {mean:.2f} | {mean * per_step:.2f} |")
    print(f"\nkernel time per step: {total:.1f} us")


if __name__ == "__main__":
    main()
