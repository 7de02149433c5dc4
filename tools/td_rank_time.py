"""Time the TD kernels by identity rank, through the C ABI of ONE library file (so a build of another commit can be timed too).

  python tools/td_rank_time.py ab    --lib PATH      rank 5 through the EXISTING entry points (nlml_tucker_objective at 4,096
                                                     evaluations, nlml_tucker_powell on BASELINE config 3's 4,096 faces): one JSON
                                                     line; run it in alternating processes against two builds (profiles/td_identity_rank.md)
  python tools/td_rank_time.py ranks --ranks 1,3,5,8,16   the _r entry points: reference-order evaluations/s and Powell faces/s by rank,
                                                     next to the f64 vector issue bound (27 R x 1404 x 5 operations at 39.3 T op/s)
"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from nlml_hpe_amd import synth, weights

ISSUE_RATE = 39.3e12   # f64 vector operations/s: 16 lanes per clock and SIMD at 2.4 GHz
V = C.c_void_p


def load(path):
    L = C.CDLL(path)
    L.nlml_tucker_objective.argtypes = [V, V, C.c_int64, V, V, V, C.c_int64, V, V, V]
    L.nlml_tucker_powell.argtypes = [V, V, C.c_int64, V, C.c_int64, V, V, V, V, V, V, V]
    if hasattr(L, "nlml_tucker_objective_r"):
        L.nlml_tucker_objective_r.argtypes = [V, V, C.c_int64, V, V, V, C.c_int64, V, V, C.c_int, C.c_int, V]
        L.nlml_tucker_powell_r.argtypes = [V, V, C.c_int64, V, C.c_int64, V, V, V, V, V, V, C.c_int, C.c_int, V]
    return L


def rank_art(art, R):
    import rank_fixture as RF
    return dict(art, W=RF.rank_W(art["W"], R), U_id=RF.rank_U_id(art["U_id"], R))


def time_objective(call, N, iters, reps):
    for _ in range(3): call()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters): call()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e3)   # us
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ab", "ranks"])
    ap.add_argument("--lib", default=os.path.join(ROOT, "nlml_hpe_amd", "libnlml_hpe_hip.so"))
    ap.add_argument("--ranks", default="1,3,5,8,16")
    ap.add_argument("--faces", type=int, default=4096)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    L = load(a.lib)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    art5 = weights.load_tucker_artefacts(os.path.join(ROOT, "outputs", "features"))
    cp = torch.from_numpy(np.stack([art5["optimized_yaw"][:3], art5["optimized_pitch"][:3], art5["optimized_roll"][:3]])).to(dev)
    N = a.faces
    idx = synth.tucker_grid_indices(N, seed=2)
    for R in ([5] if a.what == "ab" else [int(r) for r in a.ranks.split(",")]):
        art = art5 if R == 5 else rank_art(art5, R)
        Wm = torch.from_numpy(np.ascontiguousarray(art["W"]).reshape(27 * R, 1404)).to(dev)
        P = torch.from_numpy(synth.tucker_params(N, R)).to(dev)
        X = torch.from_numpy(synth.features(N, 1404, 3)).to(dev)
        Xg = torch.from_numpy(synth.tucker_grid_faces(art, idx, 1e-3, seed=2)).to(dev)
        err = torch.empty(N, dtype=torch.float64, device=dev)
        res = torch.empty(N, 3 + R, dtype=torch.float64, device=dev)
        nfev = torch.empty(N, dtype=torch.int32, device=dev)
        if a.what == "ab":
            obj = lambda: L.nlml_tucker_objective(Wm.data_ptr(), X.data_ptr(), 1404, None, P.data_ptr(), cp.data_ptr(), N, err.data_ptr(), None, stream)
            pw = lambda n: L.nlml_tucker_powell(Wm.data_ptr(), Xg.data_ptr(), 1404, cp.data_ptr(), n, None, res.data_ptr(), None, nfev.data_ptr(), None, None, stream)
        else:
            obj = lambda: L.nlml_tucker_objective_r(Wm.data_ptr(), X.data_ptr(), 1404, None, P.data_ptr(), cp.data_ptr(), N, err.data_ptr(), None, R, 1, stream)
            pw = lambda n: L.nlml_tucker_powell_r(Wm.data_ptr(), Xg.data_ptr(), 1404, cp.data_ptr(), n, None, res.data_ptr(), None, nfev.data_ptr(), None, None, R, 1, stream)
        assert obj() == 0
        us = time_objective(obj, N, 20, 5)
        assert pw(64) == 0
        torch.cuda.synchronize()
        secs = []
        for _ in range(3 if a.what == "ab" else 2):
            t0 = time.perf_counter()
            assert pw(N) == 0
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        nf = nfev.double()
        ops_per_eval = 27 * R * 1404 * 5
        rec = {"tag": a.tag, "what": a.what, "rank": R, "N": N, "objective_us": [round(u, 2) for u in us],
               "objective_evals_per_s": N / (min(us) * 1e-6), "objective_frac_of_issue_rate": N * ops_per_eval / (min(us) * 1e-6) / ISSUE_RATE,
               "issue_bound_evals_per_s": ISSUE_RATE / ops_per_eval,
               "powell_s": [round(s, 4) for s in secs], "powell_faces_per_s": N / min(secs), "powell_mean_nfev": float(nf.mean()),
               "powell_max_nfev": int(nf.max()), "powell_evals_per_s": float(nf.sum()) / min(secs),
               "powell_frac_of_issue_rate": float(nf.sum()) * ops_per_eval / min(secs) / ISSUE_RATE}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
