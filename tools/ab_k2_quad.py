"""A/B of the strict-fast mode's four-tile kernel against the fused kernel on ONE box in ONE process, alternating, at 65,536 faces:
  A   nlml_landmarks_to_pose                  the plain call: the fused kernel + the re-evaluation launch
  A'  the same call again                     the run-to-run spread of the harness itself (A against A)
  Q   nlml_landmarks_to_pose_ws + workspace   the dispatcher's choice: on a 256-unit device the four-tile kernel for the whole batch
  O   ops.landmarks_to_pose                   what bench.py times (the host layer's route to Q)
Each round times <launches> launches of each after <settle> untimed ones, in the order A Q A' O; a gain counts where it exceeds three
times the |A / A' - 1| spread.  The bits of Q and O are compared with A's first.
usage: python tools/ab_k2_quad.py [rounds=3] [launches=300] [settle=100]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nlml_hpe_amd import _lib, ops, synth, weights

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 300
settle = int(sys.argv[3]) if len(sys.argv) > 3 else 100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 65536
dev = torch.device("cuda:0")
heads = weights.load_head_state_dicts(os.path.join(ROOT, "models"))
blob = torch.from_numpy(weights.pack_blob(synth.encoder_state_dict(1404, seed=0), heads, _lib.MODE_F16X2S)).to(dev)
raw = torch.from_numpy(synth.raw_landmarks(B, seed=1)).to(dev)
L = _lib.lib()
st = torch.cuda.current_stream().cuda_stream
n, need = C.c_int64(0), C.c_size_t(0)
_lib.check(L.nlml_k2_quad_faces(B, C.byref(n), C.byref(need)), "nlml_k2_quad_faces")
print(f"quad part of {B} faces on this device: {n.value} faces, workspace {need.value} bytes", flush=True)
ws = torch.empty((max(16, need.value),), dtype=torch.uint8, device=dev)
out_a = torch.empty((B, 3), dtype=torch.float32, device=dev)
out_q = torch.empty((B, 3), dtype=torch.float32, device=dev)


def plain():
    _lib.check(L.nlml_landmarks_to_pose(raw.data_ptr(), B, 1, blob.data_ptr(), blob.numel(), out_a.data_ptr(), None, None, st), "plain")


def quad():
    _lib.check(L.nlml_landmarks_to_pose_ws(raw.data_ptr(), B, 1, blob.data_ptr(), blob.numel(), out_q.data_ptr(), None, None, ws.data_ptr(),
                                           ws.numel(), st), "ws")


def host():
    return ops.landmarks_to_pose(raw, blob, True)


plain(); quad()
torch.cuda.synchronize()
assert torch.equal(out_a, out_q) and torch.equal(out_a, host()), "the routes disagree"


def t(fn):
    for _ in range(settle):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / launches


rows = []
for r in range(rounds):
    a, q, a2, o = t(plain), t(quad), t(plain), t(host)
    rows.append((a, q, a2, o))
    ref = 0.5 * (a + a2)
    print(f"round {r}: A {a:.4f}  Q {q:.4f}  A' {a2:.4f}  O {o:.4f} ms   Q gain {100 * (ref / q - 1):+.2f} %  O gain {100 * (ref / o - 1):+.2f} %  "
          f"A/A' spread {100 * abs(a / a2 - 1):.2f} %", flush=True)
spread = max(abs(a / a2 - 1) for a, _, a2, _ in rows)
gq = [0.5 * (a + a2) / q - 1 for a, q, a2, _ in rows]
go = [0.5 * (a + a2) / o - 1 for a, _, a2, o in rows]
print(f"SUMMARY rounds {rounds} launches {launches}: Q gain min {100 * min(gq):+.2f} % max {100 * max(gq):+.2f} %;  O gain min {100 * min(go):+.2f} % "
      f"max {100 * max(go):+.2f} %;  largest A/A' spread {100 * spread:.2f} %;  passes 3x spread: {min(gq) > 3 * spread and min(go) > 3 * spread}")
