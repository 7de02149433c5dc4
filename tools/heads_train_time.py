#!/usr/bin/env python3
"""Wall-clock time of training the three heads at the reference's settings (50 epochs, batch 256, the shipped table of 1001 / 801 /
601 rows): K10 (MLPHeadsTrainer.train_heads: per epoch one training call for all three networks, one evaluation call, one
synchronisation) next to the reference's loop in torch eager on the same GPU, the three networks one after another as the reference
runs them, once with its per-step loss.item() and once without.  The eager loop is given what the reference's does not have: the
table and the targets already on the device, the batch gathered there by index.

    python tools/heads_train_time.py [--epochs 50] [--repeats 3] [--out profiles/heads_train_time.jsonl]
    python tools/heads_train_time.py --only k10 --repeats 1        # the workload for a kernel trace

Prints one JSON line per measurement (the median of the repeats, after one warm-up run each).  Run each --only under a time limit
of its own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nlml_hpe_amd import MLPHeadsTrainer as MT  # noqa: E402
from nlml_hpe_amd.artefacts import heads_training_table  # noqa: E402
from nlml_hpe_amd.entrypoints import load_config  # noqa: E402
from nlml_hpe_amd.weights import HEAD_NAMES  # noqa: E402


def eager_network(sd, xt, yt, xv, yv, orders, batch, lr, item, dev):
    """train_network (NLML_HPE_MLPHeadsTrainer.py:83-126) for one network."""
    layers, fan_in = [], xt.shape[1]
    for i, w in enumerate(MT.HEADS_WIDTHS):
        lin = torch.nn.Linear(fan_in, w)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(sd[f"model.{2 * i}.weight"]))
            lin.bias.zero_()
        layers += [lin] + ([torch.nn.ReLU()] if i < 4 else [])
        fan_in = w
    net = torch.nn.Sequential(*layers).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=lr, weight_decay=1e-5)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.9)
    crit = torch.nn.MSELoss()
    best = float("inf")
    for order in orders:
        net.train()
        train_loss = 0.0
        for s in range(0, order.shape[0], batch):
            idx = order[s:s + batch]
            opt.zero_grad()
            loss = crit(net(xt[idx]).squeeze(), yt[idx])
            loss.backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
            opt.step()
            if item:
                train_loss += loss.item()
        net.eval()
        val = 0.0 if item else torch.zeros((), device=dev)
        with torch.no_grad():
            for s in range(0, xv.shape[0], batch):
                loss = crit(net(xv[s:s + batch]).squeeze(), yv[s:s + batch])
                val = val + (loss.item() if item else loss)
        if item:
            best = min(best, val)
        sched.step()
    return net, (best if item else float(val))      # without item(): one read-back per network, at its end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["k10", "eager_item", "eager"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = load_config(os.path.join(ROOT, "configs", "config_MlpHeads.yaml"))
    td = np.load(os.path.join(ROOT, "outputs", "features", "Trained_data.npz"))
    results = []

    def timed(fn):
        fn()                                   # warm-up run
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), ts

    steps = None
    if args.only in (None, "k10"):
        hist = {}

        def k10():
            hist["h"] = MT.train_heads(td, cfg, out_dir=None, epochs=args.epochs, batch_size=args.batch, device=dev, verbose=False)[1]
        t, ts = timed(k10)
        steps = sum(len(s) for n in HEAD_NAMES for s in hist["h"][n]["step_loss"])
        results.append({"what": "k10, train_heads (table, 3 networks per launch, one read-back per epoch)", "epochs": args.epochs,
                        "batch": args.batch, "network_steps": steps, "seconds": t, "all": ts,
                        "first_train_loss": {n: hist["h"][n]["train_loss"][0] for n in HEAD_NAMES},
                        "last_train_loss": {n: hist["h"][n]["train_loss"][-1] for n in HEAD_NAMES},
                        "last_val_loss": {n: hist["h"][n]["val_loss"][-1] for n in HEAD_NAMES}})
    if args.only in (None, "eager_item", "eager"):
        tab = heads_training_table(cfg, {n: td[f"optimized_{n}"] for n in HEAD_NAMES}, device=dev)
        rows = [tab[n][0].shape[0] for n in HEAD_NAMES]
        split = MT.split_rows(rows, 0)
        orders = MT.epoch_orders([len(split[n][0]) for n in HEAD_NAMES], args.epochs, 0)
        sds = MT.initial_state_dicts([tab[n][0].shape[1] for n in HEAD_NAMES], 0)
        data = {}
        for n in HEAD_NAMES:
            x, y = tab[n][0].to(torch.float32), torch.from_numpy(tab[n][1]).to(dev)
            tr, va = (torch.from_numpy(np.ascontiguousarray(i)).to(dev) for i in split[n])
            data[n] = (x[tr], y[tr], x[va], y[va], [torch.from_numpy(o).long().to(dev) for o in orders[n]])
        for item in ((True, False) if args.only is None else ((True,) if args.only == "eager_item" else (False,))):
            def eager():
                for n in HEAD_NAMES:
                    xt, yt, xv, yv, od = data[n]
                    eager_network(sds[n], xt, yt, xv, yv, od, args.batch, 5e-3, item, dev)
            t, ts = timed(eager)
            results.append({"what": "torch eager, loss.item() every step (the reference)" if item else "torch eager, no item()",
                            "epochs": args.epochs, "batch": args.batch, "seconds": t, "all": ts})
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.writelines(json.dumps(r) + "\n" for r in results)


if __name__ == "__main__":
    main()
