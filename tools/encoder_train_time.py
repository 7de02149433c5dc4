#!/usr/bin/env python3
"""Steps per second of the encoder's training loop at the reference's settings (batch 256, F = 1404, one epoch of 650 steps):
K9 (ops.encoder_train_steps: the whole epoch enqueued, one synchronisation) next to the same loop in torch eager on the same GPU,
once with the reference's per-step loss.item() and once without it.  The eager loop is given every advantage the reference's does
not have: the dataset and the target tables already on the device, the batch gathered there by index.

    python tools/encoder_train_time.py [--steps 650] [--repeats 3] [--out profiles/encoder_train_time.jsonl]
    python tools/encoder_train_time.py --only k9 --repeats 1       # the workload for a kernel trace

Prints one JSON line per measurement (the median of the repeats, after one warm-up epoch each).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlml_hpe_amd import EncoderTrainer as ET  # noqa: E402
from nlml_hpe_amd import ops  # noqa: E402


def eager_epoch(model, opt, x, labels, tabs, order, batch, item):
    crit = torch.nn.MSELoss()
    total = 0.0
    for s in range(0, order.shape[0], batch):
        idx = order[s:s + batch]
        pred = model(x[idx])
        lab = labels[idx]
        loss = sum(crit(pred[:, 3 * t:3 * t + 3], tabs[t][lab[:, t]]) for t in range(3))
        loss.backward()                                                  # no zero_grad: the reference's loop
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=20.0)
        opt.step()
        if item:
            total += loss.item()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=650)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["k9", "eager"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    F, N = 1404, args.steps * args.batch
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((N, F), generator=g, device=dev) * 4.0 - 2.0
    tabs = [torch.rand((n, 3), generator=g, device=dev) - 0.5 for n in (11, 9, 7)]
    labels = torch.stack([torch.randint(0, n, (N,), generator=g, device=dev) for n in (11, 9, 7)], dim=1).to(torch.int32)
    order = torch.randperm(N, generator=g, device=dev).to(torch.int32)
    sd = ET.initial_state_dict(F, 0)
    results = []

    def timed(fn):
        fn()                                   # warm-up epoch
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    if args.only in (None, "k9"):
        p = torch.from_numpy(ET.flatten_state_dict(sd)).to(dev)
        gr = torch.zeros_like(p)

        def k9():
            loss, norm, status = ops.encoder_train_steps(x, labels, tabs, p, gr, order=order, batch=args.batch)
            return loss.cpu()                  # the epoch's one synchronisation, as the trainer does it
        t = timed(k9)
        results.append({"what": "k9", "steps": args.steps, "batch": args.batch, "F": F, "seconds": t, "steps_per_s": args.steps / t,
                        "us_per_step": 1e6 * t / args.steps})
    if args.only in (None, "eager"):
        for item in (True, False):
            layers, fan_in = [], F
            for i, w in enumerate(ET.ENCODER_WIDTHS):
                lin = torch.nn.Linear(fan_in, w)
                with torch.no_grad():
                    lin.weight.copy_(torch.from_numpy(sd[f"encoder.{2 * i}.weight"]))
                    lin.bias.zero_()
                layers += [lin] + ([torch.nn.ReLU()] if i < 4 else ([torch.nn.Tanh()] if i == 4 else []))
                fan_in = w
            model = torch.nn.Sequential(*layers).to(dev)
            opt = torch.optim.SGD(model.parameters(), lr=1e-4, weight_decay=1e-5)
            lab64, ord64 = labels.long(), order.long()
            t = timed(lambda: eager_epoch(model, opt, x, lab64, tabs, ord64, args.batch, item))
            results.append({"what": "torch eager, loss.item() every step" if item else "torch eager, no item()", "steps": args.steps,
                            "batch": args.batch, "F": F, "seconds": t, "steps_per_s": args.steps / t, "us_per_step": 1e6 * t / args.steps})
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in results)


if __name__ == "__main__":
    main()
