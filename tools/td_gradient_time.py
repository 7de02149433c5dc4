"""K3g timing at N = 4,096 evaluations, identity rank 5 (BASELINE config 3's inputs):

  (a) ops.tucker_gradient                      the native value-and-gradient call (two launches);
  (b) TD_Tester.compute_gradient_batch         the library path (K3 launch + torch ops + three rocBLAS f64 matmuls), host copies included
                                               as a caller pays them; (b_dev) the same arithmetic on device tensors, copies left out;
  (c) 4 x ops.tucker_objective(order="reference")   four reference-order objective launches: the f64 issue-rate yardstick (a gradient
                                               is four chains of the same pass).

    python tools/td_gradient_time.py [reps]

Device events around each form after warm-up, median of `reps`; prints one JSON line (also: the share of the f64 vector issue rate the
K3g call reaches, counting 22 f64 operations per (q, m): 20 in the four chains, 2 in the identity term)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nlml_hpe_amd import TD_Tester as HT  # noqa: E402
from nlml_hpe_amd import ops, synth, weights  # noqa: E402

N, R = 4096, 5
F64_ISSUE_PER_S = 256 * 4 * 16 * 2.4e9          # CUs x SIMDs x f64 lanes per clock x clock


def _time(fn, reps: int, warm: int = 3) -> float:
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
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dev = torch.device("cuda:0")
    art = weights.load_tucker_artefacts(os.path.join(root, "outputs", "features"))
    Py, Pp, Pr = art["optimized_yaw"][:3], art["optimized_pitch"][:3], art["optimized_roll"][:3]
    P = synth.tucker_params(N, R, seed=2)
    X = synth.tucker_grid_faces(art, synth.tucker_grid_indices(N, seed=2), seed=2)
    Wm = torch.from_numpy(np.asarray(art["W"], np.float32).reshape(-1, 1404)).to(dev)
    Xd, Pd = torch.from_numpy(X).to(dev), torch.from_numpy(P).to(dev)
    cp = torch.from_numpy(np.stack([Py, Pp, Pr])).to(dev)

    t_a = _time(lambda: ops.tucker_gradient(Wm, Xd, Pd, cp), reps)
    t_b = _time(lambda: HT.compute_gradient_batch(P, art["W"], X, Py, Pp, Pr), reps)
    t_c1 = _time(lambda: ops.tucker_objective(Wm, Xd, Pd, cp, order="reference"), reps)
    t_c = _time(lambda: [ops.tucker_objective(Wm, Xd, Pd, cp, order="reference") for _ in range(4)], reps)
    ops_f64 = N * 27 * R * 1404 * 22
    print(json.dumps({"N": N, "R": R, "reps": reps, "k3g_ms": round(t_a, 4), "library_path_ms": round(t_b, 4),
                      "objective_ref_ms": round(t_c1, 4), "four_objectives_ms": round(t_c, 4),
                      "k3g_over_four_objectives": round(t_a / t_c, 3),
                      "k3g_f64_issue_fraction": round(ops_f64 / (t_a * 1e-3) / F64_ISSUE_PER_S, 3),
                      "objective_f64_issue_fraction": round(N * 27 * R * 1404 * 5 / (t_c1 * 1e-3) / F64_ISSUE_PER_S, 3)}))


if __name__ == "__main__":
    main()
