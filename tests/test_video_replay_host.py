"""CPU: the multi-stream video oracle (oracle/video_math.replay) against the reference's own frame loop (FX7), and the conditions
the GPU comparison of tests/test_video_post_gpu.py rests on, measured on the oracle alone for every case that file runs."""
import json
import os

import numpy as np
import pytest

import video_cases as VC
from oracle import video_math as VM


@pytest.fixture(scope="module")
def fx7(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "fx7_video_math.json")))
    gin = np.load(os.path.join(golden_dir, "fx7_video_in.npz"), allow_pickle=False)
    valid = np.ones(len(gin["pose_rad"]), dtype=bool)
    valid[gin["no_face"]] = False
    return g, gin["pose_rad"], gin["landmarks"], valid


def test_replay_reproduces_fx7_exactly(fx7):
    g, pose, lm, valid = fx7
    r = VM.replay(pose[:, None], lm[:, None], valid[:, None], g["width"], g["height"])
    frames = {f["frame"]: f for f in g["frames"]}
    assert sorted(frames) == np.flatnonzero(valid).tolist() and not valid.all()
    assert np.array_equal(r["updated"][:, 0], valid)
    count = 0
    for t in range(len(pose)):
        if not valid[t]:                                           # the no-face frames: nothing moves
            for k in ("smoothed", "centre", "endpoints", "state"):
                assert np.array_equal(r[k][t, 0], r[k][t - 1, 0] if t else np.zeros_like(r[k][t, 0]))
            continue
        fr, count = frames[t], count + 1
        assert r["smoothed"][t, 0].tolist() == fr["smoothed"]      # exact: the JSON holds the reference's floats by repr
        assert r["centre"][t, 0].tolist() == fr["centre"]
        c, e = r["centre"][t, 0], r["endpoints"][t, 0]
        assert [[[int(c[0]), int(c[1])], [int(e[k, 0]), int(e[k, 1])]] for k in range(3)] == fr["lines"]
        assert r["state"][t, 0].tolist() == fr["smoothed"] + fr["centre"] + [count]


def test_replay_keeps_streams_apart(fx7):
    """Stream 0 = FX7, stream 1 = FX7 three ticks late (no face until then): each gets FX7's own result."""
    g, pose, lm, valid = fx7
    T, k = len(pose), 3
    one = VM.replay(pose[:, None], lm[:, None], valid[:, None], g["width"], g["height"])
    p2, l2, v2 = np.zeros((T + k, 2, 3), np.float32), np.zeros((T + k, 2, 468, 3), np.float32), np.zeros((T + k, 2), bool)
    p2[:T, 0], l2[:T, 0], v2[:T, 0] = pose, lm, valid
    p2[k:, 1], l2[k:, 1], v2[k:, 1] = pose, lm, valid
    two = VM.replay(p2, l2, v2, g["width"], g["height"])
    for key, a in one.items():
        assert np.array_equal(two[key][:T, 0], a[:, 0]), key
        assert np.array_equal(two[key][k:, 1], a[:, 0]), key
        assert not two[key][:k, 1].any(), key                     # nothing before the late stream's first face


@pytest.mark.parametrize("consts", sorted(VC.CONSTANTS))
@pytest.mark.parametrize("S", VC.STREAMS)
def test_gpu_cases_meet_their_conditions(S, consts):
    c = VC.case(S, consts)
    q = VC.conditions(c)
    assert q["rounding_differs"] == 0, q                           # round(deg, 2) == rint(deg * 100) / 100 for every pose used
    assert q["gate_margin_px"] > VC.GATE_MARGIN_PX, q              # no gate decision on the threshold
    assert q["int_excluded"] <= VC.MAX_INT_EXCLUDED, q
    assert q["seeded_late"] >= 1 and q["skipped_runs"] >= 1 and q["accepted"] >= 1 and q["rejected"] >= 1, q
    upd, pose = c["ref"]["updated"], c["pose"]
    skipped_faces = c["valid"] & ~upd                              # a face, but a NaN / Inf pose
    assert (skipped_faces.sum(axis=0) == 2).all()
    assert np.isnan(pose[skipped_faces]).any(axis=1).sum() == S and np.isinf(pose[skipped_faces]).any(axis=1).sum() == S
    assert np.abs(pose[upd]).max() <= np.float32(np.pi / 2)
    for s in {S - 1, min(64, S - 1)}:                              # the last stream, and the first one of the second block
        assert not c["valid"][0, s] and upd[:, s].sum() >= 5
    if S >= 63:
        assert q["rejected_then_accepted"] >= S // 2, q            # moves measured from the kept centre after a rejected one
        schedules = {(tuple(c["valid"][:, s]), tuple(upd[:, s])) for s in range(S)}
        assert len(schedules) > S // 2                             # the streams are on schedules of their own


def test_cases_are_cached_and_read_only():
    a = VC.case(65)
    assert a is VC.case(65) and not a["pose"].flags.writeable and not a["ref"]["state"].flags.writeable
