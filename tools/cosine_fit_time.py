"""K8 timing: the cosine fit of the pose factors, nine fits (the reference's workload) and 4,096 fits in one launch.

    python tools/cosine_fit_time.py [--reps 20] [--warmup 3] [--out cosine_fit_time.md]

The nine fits are the columns of the shipped factor matrices from their Fourier starts: what TD_Trainer.Train launches.  The 4,096
are those nine columns in turn, each start moved by up to 1 % (a fixed seed), so the fits' evaluation counts differ as real columns'
do.  Each measurement is a pair of device events around one call of ops.cosine_fit (output allocation from torch's caching allocator
and the 16 KB copy of the row counts included); the median is reported with min and max.  The same batches go through
nlml_cosine_fit_host on this host's CPU (one thread, wall clock, one run; of a large batch the first --host-fits fits) and, for nine, through Train end to end (host Fourier
starts, copies, launch, read-back).  No bound is asserted.  Writes a markdown table and prints the same numbers as one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlml_hpe_amd import TD_Trainer, ops  # noqa: E402

BINS = [np.arange(-50, 51, 10), np.arange(-40, 41, 10), np.arange(-30, 31, 10)]


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
    return {"ms": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--many", type=int, default=4096)
    ap.add_argument("--host-fits", type=int, default=64)
    ap.add_argument("--features", default=os.path.join("outputs", "features"))
    ap.add_argument("--out", default="cosine_fit_time.md")    # its table is quoted in profiles/cosine_fit.md
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fm = np.load(os.path.join(args.features, "Factor_Matrices.npz"))
    pairs = [(fm[k], b) for k, b in zip(("U_yaw", "U_pitch", "U_roll"), BINS)]
    guess = TD_Trainer.estimate_init_Fourier_Trans(*pairs)
    y9, w9, n9, x9 = TD_Trainer._pack([(U, w, g) for (U, w), g in zip(pairs, guess)])

    rng = np.random.default_rng(0)
    pick = np.arange(args.many) % 9
    batches = {"9": (y9, w9, n9, x9),
               str(args.many): (y9[pick], w9[pick], n9[pick], x9[pick] * (1.0 + 0.01 * rng.uniform(-1, 1, (args.many, 4))))}
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup, "fits": {}}
    for name, (y, w, n, x0) in batches.items():
        yd, wd, xd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (y, w, x0))
        nl = torch.from_numpy(np.ascontiguousarray(n))
        r = timed(lambda: ops.cosine_fit(yd, wd, nl, xd), args.reps, args.warmup)
        out = ops.cosine_fit(yd, wd, nl, xd)
        nfev = out["nfev"].cpu().numpy()
        r.update(evaluations=int(nfev.sum()), nfev_max=int(nfev.max()), at_maxfev=int((out["status"].cpu().numpy() == 2).sum()))
        hn = min(len(n), args.host_fits)                  # the host form takes ~30 ms a fit: a prefix of a large batch
        t0 = time.perf_counter()
        host = TD_Trainer.fit_columns([(np.ascontiguousarray(y[f:f + 1, :n[f]].T), w[f, :n[f]], x0[f:f + 1]) for f in range(hn)],
                                      backend="host")
        r["host_s"], r["host_fits"] = round(time.perf_counter() - t0, 3), hn
        r["same_bits_as_host"] = bool(np.array_equal(host["x"].view(np.int64), out["x"][:hn].cpu().numpy().view(np.int64)))
        res["fits"][name] = r
    walls = []
    for _ in range(args.warmup + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        TD_Trainer.Train(*pairs, backend="device")
        walls.append(time.perf_counter() - t0)
    res["train_device_s"] = round(min(walls[args.warmup:]), 5)
    print(json.dumps(res), flush=True)

    lines = ["# K8: the pose factors' cosine fits on the device", "",
             f"`python tools/cosine_fit_time.py --reps {args.reps} --warmup {args.warmup}` on {res['device']}: {args.warmup} warm-up calls, then the",
             f"median of {args.reps} measurements, each a pair of device events around one `ops.cosine_fit` call.  One wave per fit, the whole",
             "Powell minimisation inside the launch.  Host: `nlml_cosine_fit_host` on one CPU thread of the same machine, one run.", "",
             "| fits in the launch | evaluations (largest fit; fits at maxfev) | device, ms (min .. max) | host form, s (fits) | device = host bits |",
             "|---|---|---|---|---|"]
    for name, r in res["fits"].items():
        lines.append(f"| {name} | {r['evaluations']:,} ({r['nfev_max']}; {r['at_maxfev']}) | {r['ms']} ({r['ms_min']} .. {r['ms_max']}) | "
                     f"{r['host_s']} ({r['host_fits']}) | {r['same_bits_as_host']} |")
    lines += ["", f"`TD_Trainer.Train` on the shipped factors end to end (host Fourier starts, copies, the launch, read-back): "
              f"**{res['train_device_s'] * 1e3:.2f} ms** wall clock (best of three after warm-up).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
