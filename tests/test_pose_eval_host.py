"""CPU: the K5 evaluation entry points (nlml_pose_eval, nlml_pose_eval_merge) refuse bad arguments before any HIP call, their
length formulas, the Meta shapes of torch.ops.nlml_hpe.pose_eval / pose_eval_merge, and the merge rule they use."""
import ctypes as C

import numpy as np
import pytest
import torch

from nlml_hpe_amd import _lib, ops  # noqa: F401  (ops registers torch.ops.nlml_hpe.*)
from pose_eval_cases import chan as _chan, part as _part

BADARG = -1
FAKE = 4096       # an aligned non-null "device" pointer: every call below is refused before it could be used


def _h(vals, ctype=C.c_double):
    return (ctype * max(1, len(vals)))(*vals)


def _call(pose_rad=FAKE, pred_deg=None, valid=None, gt=FAKE, B=10, lo=None, hi=None, decimals=3, intervals=(), axes=(),
          K=None, ws=FAKE, ws_bytes=1 << 20, record=FAKE, result=FAKE):
    L = _lib.lib()
    lo = _h([-50.0, -40.0, -30.0]) if lo is None else lo
    hi = _h([51.0, 41.0, 31.0]) if hi is None else hi
    K = len(axes) if K is None else K
    return L.nlml_pose_eval(pose_rad, pred_deg, valid, gt, B, lo, hi, decimals, _h(list(intervals)), _h(list(axes), C.c_int32), K,
                            ws, ws_bytes, record, result, None, None, None)


def _err():
    return _lib.lib().nlml_last_error().decode()


def test_length_formulas():
    L = _lib.lib()
    for K in (0, 1, 18, 64):
        assert L.nlml_pose_eval_record_len(K) == 12 + 2 * K
        assert L.nlml_pose_eval_result_len(K) == 14 + 2 * K
    assert L.nlml_pose_eval_record_len(65) == 0 and L.nlml_pose_eval_result_len(-1) == 0
    per = _lib.POSE_EVAL_FACES_PER_RECORD
    for B, K in ((0, 18), (1, 18), (per, 0), (per + 1, 18), (1_048_576, 18), (1_048_577, 64)):
        assert L.nlml_pose_eval_workspace_bytes(B, K) == -(-B // per) * (12 + 2 * K) * 8, (B, K)
    assert L.nlml_pose_eval_workspace_bytes(-1, 18) == 0 and L.nlml_pose_eval_workspace_bytes(10, 65) == 0


@pytest.mark.parametrize("case, kwargs, text", [
    ("both pose forms", dict(pred_deg=FAKE), "exactly one"),
    ("neither pose form", dict(pose_rad=None), "exactly one"),
    ("both pose forms, B = 0", dict(pred_deg=FAKE, B=0), "exactly one"),
    ("null gt", dict(gt=None), "gt_deg"),
    ("null result", dict(result=None), "result_out"),
    ("negative B", dict(B=-1), "negative B"),
    ("K above the cap", dict(K=65, intervals=[0.0, 1.0] * 65, axes=[0] * 65), "intervals"),
    ("negative K", dict(K=-1), "intervals"),
    ("axis 3", dict(intervals=[0.0, 1.0, 1.0, 2.0], axes=[0, 3]), "axis"),
    ("axis -1", dict(intervals=[0.0, 1.0], axes=[-1]), "axis"),
    ("decimals 16", dict(decimals=16), "decimals"),
    ("workspace too small", dict(B=2049, ws_bytes=2 * 12 * 8 - 8), "workspace"),
    ("null workspace", dict(ws=None), "workspace"),
    ("misaligned gt", dict(gt=FAKE + 4), "aligned"),
])
def test_pose_eval_refuses(case, kwargs, text):
    assert _call(**kwargs) == BADARG, case
    assert text in _err(), (case, _err())


def test_pose_eval_refuses_null_bounds_and_intervals():
    L = _lib.lib()
    lo = _h([0.0, 0.0, 0.0])
    assert L.nlml_pose_eval(FAKE, None, None, FAKE, 4, None, lo, 3, None, None, 0, FAKE, 64, None, FAKE, None, None, None) == BADARG
    assert L.nlml_pose_eval(FAKE, None, None, FAKE, 4, lo, lo, 3, None, None, 2, FAKE, 1024, None, FAKE, None, None, None) == BADARG
    assert "intervals" in _err()


def test_pose_eval_merge_refuses():
    L = _lib.lib()
    assert L.nlml_pose_eval_merge(FAKE, -1, 18, FAKE, FAKE, None) == BADARG and "negative" in _err()
    assert L.nlml_pose_eval_merge(FAKE, 3, 65, FAKE, FAKE, None) == BADARG and "intervals" in _err()
    assert L.nlml_pose_eval_merge(None, 3, 18, FAKE, FAKE, None) == BADARG and "null" in _err()
    assert L.nlml_pose_eval_merge(FAKE, 3, 18, FAKE, None, None) == BADARG and "null" in _err()
    assert L.nlml_pose_eval_merge(FAKE + 4, 3, 18, FAKE, FAKE, None) == BADARG and "aligned" in _err()


def test_torch_ops_meta_shapes():
    K = 18
    pose = torch.empty((1000, 3), dtype=torch.float32, device="meta")
    gt = torch.empty((1000, 3), dtype=torch.float64, device="meta")
    rec, res = torch.ops.nlml_hpe.pose_eval(pose, None, gt, [-50.0, -40.0, -30.0], [51.0, 41.0, 31.0], 3, [0.0, 1.0] * K, [0] * K)
    assert rec.shape == (12 + 2 * K,) and res.shape == (14 + 2 * K,)
    assert rec.dtype == res.dtype == torch.float64
    rec2, res2 = torch.ops.nlml_hpe.pose_eval_merge(torch.empty((3, 12 + 2 * K), dtype=torch.float64, device="meta"), K)
    assert rec2.shape == (12 + 2 * K,) and res2.shape == (14 + 2 * K,) and rec2.dtype == res2.dtype == torch.float64


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    with pytest.raises(_lib.NlmlError):
        ops.pose_eval(torch.zeros((4, 3)), torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(_lib.NlmlError):
        ops.pose_eval_merge(torch.zeros((2, 48), dtype=torch.float64), 18)


@pytest.mark.parametrize("cuts", [(0, 1, 7, 7, 500, 999), (0, 0, 1000), (3, 3, 3, 998), (1000,), (250, 500, 750)])
def test_chan_merge_matches_two_pass_std(cuts):
    """The merge rule restated in numpy, left fold over contiguous parts (empty parts included), against the two-pass std."""
    x = np.random.default_rng(5).gamma(2.0, 3.0, 1000) + 40.0
    edges = [0, *cuts, 1000]
    acc = (0, 0.0, 0.0)
    for lo, hi in zip(edges[:-1], edges[1:]):
        acc = _chan(acc, _part(x[lo:hi]))
    n, m, M = acc
    assert n == 1000
    assert abs(m - x.mean()) <= 1e-13 * x.mean()
    assert abs(np.sqrt(M / (n - 1)) - x.std(ddof=1)) <= 1e-12 * x.std(ddof=1)
