"""GPU: K5, the evaluation block in one native pass (nlml_pose_eval / ops.pose_eval / metrics.evaluate), against numpy, the ATen
metrics, the oracle and FX6; its determinism, the merge of shards, the degenerate cases, and NLML_HPE_Test.py --metrics device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nlml_hpe_amd import metrics, ops
from nlml_hpe_amd.entrypoints import load_config
from oracle import metrics as MT

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO = (-50.0, -40.0, -30.0)
HI = (51.0, 41.0, 31.0)
NAMES = ("Yaw", "Pitch", "Roll")
KEYS = ("mae_yaw", "mae_pitch", "mae_roll", "mae_total", "maev", "v_left", "v_down", "v_front", "std_yaw", "std_pitch", "std_roll")


def _shipped_intervals():
    cfg = load_config(os.path.join(REPO, "configs", "config_NLML_HPE_Test.yaml"))
    return [[tuple(x) for x in cfg[k]] for k in ("yaw_intervals", "pitch_intervals", "roll_intervals")]


def _flat(intervals):
    return [(a, lo, hi) for a, ivs in enumerate(intervals) for lo, hi in ivs]


def _dataset(B, seed=11):
    """GT with ~10 % of the rows outside LO/HI, values exactly on the range bounds and on interval edges, ~3 % without a face,
    predictions a few degrees off as the model's f32 radians."""
    rng = np.random.default_rng(seed)
    span = np.array([[-51.8, 52.9], [-41.5, 42.5], [-31.1, 32.1]])
    gt = rng.uniform(span[:, 0], span[:, 1], size=(B, 3))
    edges = [np.array(sorted({v for iv in ivs for v in iv} | {LO[a], HI[a]}), dtype=np.float64)
             for a, ivs in enumerate(_shipped_intervals())]
    for a in range(3):
        rows = rng.choice(B, size=B // 50, replace=False)
        gt[rows, a] = rng.choice(edges[a], size=rows.size)
    pose = np.radians(gt + rng.normal(0.0, 3.0, size=(B, 3))).astype(np.float32)
    valid = rng.random(B) >= 0.03
    return gt, pose, valid


def _expected(gt, pose, valid):
    pred = np.round(np.degrees(pose.astype(np.float64)), 3)
    in_range = ((gt >= np.array(LO)) & (gt <= np.array(HI))).all(axis=1)
    return pred, in_range & valid, in_range


def _eval(device, gt, pose, valid, intervals, decimals=3, **kw):
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return ops.pose_eval(dv(pose), dv(gt), dv(valid) if valid is not None else None, LO, HI, _flat(intervals), decimals, **kw)


def test_fx6_maev_and_printed_block(golden_dir, device):
    g = json.load(open(os.path.join(golden_dir, "fx6_metrics.json")))
    gt = torch.tensor(g["gt"], dtype=torch.float64, device=device)
    pr = torch.tensor(g["pred"], dtype=torch.float64, device=device)
    _, res = ops.pose_eval(pr, gt, None, None, None, (), decimals=-1)
    r = res.cpu().numpy()
    assert np.allclose(r[[4, 5, 6, 7]], g["maev"], rtol=0, atol=1e-9)
    printed = dict(line.split(": ") for line in g["printed"])
    for (label, _), v in zip(metrics._ERROR_LINES, r[:11]):
        assert f"{v:.2f}" == printed[label], label
    assert r[11] == 64 and r[12] == 0 and r[13] == 0


@pytest.fixture(scope="module")
def big(device):
    B = 1_048_576
    gt, pose, valid = _dataset(B)
    intervals = _shipped_intervals()
    rec, res, pred, keep = _eval(device, gt, pose, valid, intervals, return_per_face=True)
    return dict(gt=gt, pose=pose, valid=valid, intervals=intervals, rec=rec, res=res, pred=pred, keep=keep)


def test_million_faces_against_numpy_and_aten(big, device):
    gt, pose, valid, intervals = big["gt"], big["pose"], big["valid"], big["intervals"]
    pred, keep, in_range = _expected(gt, pose, valid)
    assert np.array_equal(big["pred"].cpu().numpy().view(np.uint64), pred.view(np.uint64))
    assert np.array_equal(big["keep"].cpu().numpy(), keep)
    r = big["res"].cpu().numpy()
    assert 0.07 < (~in_range).mean() < 0.13 and 0.02 < (~valid).mean() < 0.04
    assert (r[11], r[12], r[13]) == (keep.sum(), (~valid).sum(), (~in_range).sum())
    gk, pk = torch.from_numpy(gt[keep]).to(device), torch.from_numpy(pred[keep]).to(device)
    ref = metrics.compute_errors(gk, pk, verbose=False)
    for i, k in enumerate(KEYS):
        if k in ("maev", "v_left", "v_down", "v_front"):
            assert abs(r[i] - ref[k]) <= 1e-9, (k, r[i], ref[k])
        else:
            assert abs(r[i] - ref[k]) <= 1e-12 * abs(ref[k]), (k, r[i], ref[k])
    iv = metrics.compute_interval_mae(gk, pk, *intervals)
    for k, (a, lo, hi) in enumerate(_flat(intervals)):
        m = keep & (gt[:, a] >= lo) & (gt[:, a] < hi)
        assert r[14 + 2 * k] == m.sum(), (a, lo, hi)
        want = iv[f"{NAMES[a]} ({lo}, {hi}) - NLML_HPE"]
        assert abs(r[15 + 2 * k] - want) <= 1e-12 * want, (a, lo, hi)
    # the bounds and the interval edges are hit exactly, so the inclusive / half-open rules are exercised
    assert (gt == np.array(LO)).any() and (gt == np.array(HI)).any() and (gt[:, 0] == -33.33).any()


def test_oracle_on_a_subset(big, device):
    n = 20_000
    gt, pose, valid, intervals = big["gt"][:n], big["pose"][:n], big["valid"][:n], big["intervals"]
    pred, keep, _ = _expected(gt, pose, valid)
    _, res = _eval(device, gt, pose, valid, intervals)
    r = res.cpu().numpy()
    exp = MT.compute_errors(gt[keep], pred[keep])
    for i, k in enumerate(KEYS):
        tol = 1e-9 if k in ("maev", "v_left", "v_down", "v_front") else 1e-12 * abs(exp[k])
        assert abs(r[i] - exp[k]) <= tol, (k, r[i], exp[k])
    k = 0
    for a, ivs in enumerate(intervals):
        want = MT.interval_mae(gt[keep], pred[keep], a, ivs)
        for lo, hi in ivs:
            assert abs(r[15 + 2 * k] - want[(lo, hi)]) <= 1e-12 * want[(lo, hi)], (a, lo, hi)
            k += 1


def test_two_calls_are_bit_identical(big, device):
    rec2, res2 = _eval(device, big["gt"], big["pose"], big["valid"], big["intervals"])
    assert torch.equal(big["rec"].view(torch.int64), rec2.view(torch.int64))
    assert torch.equal(big["res"].view(torch.int64), res2.view(torch.int64))


def test_uneven_shards_merge_to_the_single_call(big, device):
    gt, pose, valid, intervals = big["gt"], big["pose"], big["valid"], big["intervals"]
    cuts = [(0, 300_001), (300_001, 300_001), (300_001, gt.shape[0])]
    recs = [_eval(device, gt[a:b], pose[a:b], valid[a:b], intervals)[0] for a, b in cuts]
    K = len(_flat(intervals))
    rec, res = ops.pose_eval_merge(torch.stack(recs), K)
    r, one = res.cpu().numpy(), big["res"].cpu().numpy()
    assert np.array_equal(r[11:14], one[11:14]) and np.array_equal(r[14::2], one[14::2])
    assert np.allclose(r, one, rtol=1e-13, atol=0)
    assert np.array_equal(rec.cpu().numpy()[[0, 1, 2]], big["rec"].cpu().numpy()[[0, 1, 2]])


def test_degenerate_cases(device):
    intervals = _shipped_intervals()
    K = len(_flat(intervals))
    gt, pose, valid = _dataset(5000, seed=3)
    gt[:, :] = np.clip(gt, np.array(LO), np.array(HI))
    # no kept face: every row without a face
    _, res = _eval(device, gt, pose, np.zeros(5000, bool), intervals)
    r = res.cpu().numpy()
    assert np.isnan(r[:11]).all() and (r[11], r[12], r[13]) == (0, 5000, 0)
    assert (r[14::2] == 0).all() and np.isnan(r[15::2]).all()
    # one kept face: means as numpy, std NaN (ddof = 1)
    v1 = np.zeros(5000, bool)
    v1[4321] = True
    _, res = _eval(device, gt, pose, v1, intervals)
    r = res.cpu().numpy()
    pred, keep, _ = _expected(gt, pose, v1)
    e = np.abs(gt[keep] - pred[keep])[0]
    assert np.array_equal(r[:3], e) and np.isnan(r[8:11]).all() and r[11] == 1
    # B = 0
    _, res = ops.pose_eval(torch.zeros((0, 3), device=device), torch.zeros((0, 3), dtype=torch.float64, device=device), None, LO, HI,
                           _flat(intervals))
    r = res.cpu().numpy()
    assert r.shape == (14 + 2 * K,) and np.isnan(r[:11]).all() and (r[11:14] == 0).all() and np.isnan(r[15::2]).all()
    # NaN on a kept face propagates as in numpy's f64 sums; the other axes stay finite
    pn, valid = pose.copy(), valid.copy()
    pn[17, 1] = np.nan
    valid[17] = True
    _, res = _eval(device, gt, pn, valid, intervals)
    r = res.cpu().numpy()
    pred, keep, _ = _expected(gt, pn, valid)
    assert keep[17]
    e = np.abs(gt[keep] - pred[keep])
    with np.errstate(invalid="ignore"):
        want_mae, want_std = e.mean(0), e.std(0, ddof=1)
    assert np.isnan(r[1]) and np.isnan(want_mae[1]) and np.isnan(r[9]) and np.isnan(r[4]) and np.isnan(r[6])
    assert np.allclose(r[[0, 2]], want_mae[[0, 2]], rtol=1e-12) and np.allclose(r[[8, 10]], want_std[[0, 2]], rtol=1e-12)


def test_torch_op_equals_ops_and_does_not_synchronise(device):
    intervals = _shipped_intervals()
    gt, pose, valid = _dataset(70_001, seed=9)
    dg, dp, dv = (torch.from_numpy(x).to(device) for x in (gt, pose, valid))
    fl = _flat(intervals)
    rec, res = ops.pose_eval(dp, dg, dv, LO, HI, fl, 3)
    rec2, res2 = torch.ops.nlml_hpe.pose_eval(dp, dv, dg, list(LO), list(HI), 3, [float(v) for _, lo, hi in fl for v in (lo, hi)],
                                              [a for a, _, _ in fl])
    assert torch.equal(rec.view(torch.int64), rec2.view(torch.int64)) and torch.equal(res.view(torch.int64), res2.view(torch.int64))
    m1 = ops.pose_eval_merge(torch.stack([rec, rec]), len(fl))[1]
    m2 = torch.ops.nlml_hpe.pose_eval_merge(torch.stack([rec, rec]), len(fl))[1]
    assert torch.equal(m1.view(torch.int64), m2.view(torch.int64))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.pose_eval(dp, dg, dv, LO, HI, fl, 3)
        ops.pose_eval_merge(torch.stack([rec, rec]), len(fl))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    d = metrics.evaluate(dp, dv, dg, LO, HI, intervals, verbose=False)
    pred, keep, _ = _expected(gt, pose, valid)
    ref = metrics.compute_errors(gt[keep], pred[keep], verbose=False)
    ref.update(metrics.compute_interval_mae(gt[keep], pred[keep], *intervals))
    assert set(d) == set(ref) | {"n_processed", "n_no_face", "n_out_of_range"}
    assert d["n_processed"] == keep.sum()


def _lines(stdout):
    """the printed lines without the timing line and the gloo library's own connection notices (two ranks write theirs to the same
    pipe in pieces, so a notice can arrive split over two lines: "...[Gloo] Rank " / "1 is connected to 1 peer ranks. ...", or two
    notices woven into one line with the second one's line end left behind as an empty line: empty lines straight after a notice
    go with it -- the entry point prints none before its first line)"""
    out, after_notice = [], False
    for l in stdout.splitlines():
        notice = l.startswith("[Gloo]") or "peer ranks. Expected number of connected peer ranks" in l
        if notice or (after_notice and not l):
            after_notice = True
            continue
        after_notice = False
        if not l.startswith("Average Elapsed time"):
            out.append(l)
    return out


def test_test_entry_point_device_metrics_print_the_same_lines(repo_root, device):
    env = dict(os.environ, PYTHONPATH=repo_root)
    runs = {}
    for m in ("host", "device"):
        res = subprocess.run([sys.executable, "NLML_HPE_Test.py", "--metrics", m], cwd=repo_root, env=env, capture_output=True, text=True,
                             timeout=600)
        assert res.returncode == 0, (m, res.stdout[-2000:], res.stderr[-2000:])
        runs[m] = _lines(res.stdout)
    assert any(l.startswith("processed ") for l in runs["host"]) and any(l.startswith("Yaw (") for l in runs["host"])
    assert runs["device"] == runs["host"]
    # the two-rank path on this one GPU (gloo): each rank evaluates its own shard, the records are merged in rank order
    env2 = {k: v for k, v in dict(env, NLML_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1").items()
            if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    port = 29900 + (os.getpid() % 90)
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), "NLML_HPE_Test.py", "--device", "cuda:0", "--metrics", "device"],
                         cwd=repo_root, env=env2, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, (two.stdout[-2000:], two.stderr[-3000:])
    assert _lines(two.stdout) == runs["host"], two.stdout
