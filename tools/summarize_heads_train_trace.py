#!/usr/bin/env python3
"""Per-launch times of K10 from a rocprofv3 --kernel-trace CSV: the launches of one kernel are told apart by their grid size (one
size per layer and per largest batch of the step).

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o k10 -- python tools/heads_train_time.py --only k10 --repeats 1
    python tools/summarize_heads_train_trace.py out/.../k10_kernel_trace.csv
"""
import argparse
import csv
from collections import defaultdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    args = ap.parse_args()
    rows = defaultdict(list)
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("kernel_name") or ""
            if "ht_" not in name and "mlp_" not in name:   # K10's own kernels, and the forward / backward kernels it shares with K9
                continue
            grid = (r.get("Grid_Size_X") or r.get("Grid_Size") or "?", r.get("Grid_Size_Y") or "?")
            wg = r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or "?"
            rows[(name.split("(")[0].split("::")[-1], grid, wg)].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = 0.0
    print("| kernel | grid x, y (threads) | workgroup | launches | mean us | total ms |")
    print("|---|---:|---:|---:|---:|---:|")
    for (name, grid, wg), ts in sorted(rows.items(), key=lambda kv: (kv[0][0], -len(kv[1]), kv[0][1])):
        total += sum(ts)
        print(f"| {name} | {grid[0]}, {grid[1]} | {wg} | {len(ts)} | {sum(ts) / len(ts) / 1e3:.2f} | {sum(ts) / 1e6:.2f} |")
    print(f"\nkernel time in the trace: {total / 1e6:.1f} ms over {sum(len(t) for t in rows.values())} launches")


if __name__ == "__main__":
    main()
