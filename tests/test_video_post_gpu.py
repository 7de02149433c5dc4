"""K4 (csrc/video_post.hip) over many streams and ticks against oracle/video_math.replay, which test_video_replay_host.py pins to
the reference's own frame loop (FX7).  nlml_video_post_ex is driven through VideoPoseTracker.post with the synthetic poses,
landmarks and schedules of tests/video_cases.py, so the expected values depend on K4 alone.

What is asserted, for every tick and every stream:
  smoothed, centre, state (all six columns)   the oracle's bits; `updated` the oracle's mask
  a skipped stream                            smoothed, centre, end points and state keep the previous tick's bits
  end points                                  within the bound below; int() of them equal wherever the oracle's value lies more
                                              than 1e-6 from an integer (at most 0.1 % may lie closer: video_cases.conditions)

The end-point bound.  With contraction off the kernel evaluates  size * (c1*c2 [+- c3*c4*c5]) + centre  through the same IEEE
operations in the same order as the oracle, on the same angles (x * pi / 180, two roundings) and the same centre, so the two differ
only through the trig factors: the device library's f64 sin / cos, taken as within 2 ulp (the HIP math API reference's figure for
both), against the host libm's, within 1 ulp (glibc manual, x86-64).  With eps = 2^-52 >= ulp(x) / |x| and |factor| <= 1:
  one factor              differs by at most (2 + 1) eps
  one product             at most three factors -> 9 eps, and each side rounds its (at most two) multiplications on its own:
                          eps per side -> 11 eps
  the sum                 two products -> 22 eps; its rounding, magnitude <= 2: eps per side -> 24 eps
  times size              24 eps * size, and the rounding of a product of magnitude <= 2 * size: eps * size per side -> 26 eps * size
  plus centre             one rounding per side at a magnitude of at most |centre| + 2 * size: eps * (|centre| + 2 * size) together
  bound = eps * (26 * size + |centre| + 2 * size)        (first order; every term above is taken at a worst case the others exclude
                                                          -- the sum never reaches 2 -- which covers the eps^2 terms many times over)
The measured maximum, in units of eps * (|centre| + 2 * size), goes to the suite's margins file (test_gpu_parity._report) next to the bound in
the same units; the asserted figure is the derived one.  Measured on an MI355X: at most 0.86 of that unit where the bound is 3.8-4.8 of
it, with 0.2-1.5 % of the end points differing at all."""
import numpy as np
import pytest
import torch

import video_cases as VC
from nlml_hpe_amd import _lib, ops, synth
from nlml_hpe_amd.video import GraphedTick, VideoPoseTracker
from oracle import video_math as VM
from test_gpu_parity import _report          # the suite's one margins file: a JSON line per measured figure

pytestmark = pytest.mark.gpu

KEYS = ("smoothed", "centre", "endpoints", "state")
EPS = 2.0 ** -52


class _OnDevice:                     # the tracker only needs .device from the model when post() is driven directly
    def __init__(self, device):
        self.device = device


def _tracker(device, S, constants):
    W, H, alpha, max_jump, size = constants
    return VideoPoseTracker(_OnDevice(device), S, W, H, alpha, max_jump, size)


def _snapshot(tr):
    got = {k: getattr(tr, k).cpu().numpy() for k in KEYS}
    got["updated"] = tr.updated.cpu().numpy().astype(bool)
    return got


def _run(tr, pose, lm, valid, device):
    """All ticks through tr.post -> {smoothed [T,S,3], centre [T,S,2], endpoints [T,S,3,2], state [T,S,6], updated [T,S]}."""
    P, L = torch.from_numpy(np.array(pose)).to(device), torch.from_numpy(np.array(lm)).to(device)
    V = None if valid is None else torch.from_numpy(np.array(valid)).to(device)
    ticks = []
    for t in range(len(pose)):
        sm, c, ep = tr.post(P[t], L[t], None if V is None else V[t])
        assert sm is tr.smoothed and c is tr.centre and ep is tr.endpoints
        ticks.append(_snapshot(tr))
    return {k: np.stack([g[k] for g in ticks]) for k in ticks[0]}


_runs = {}


def _case_run(device, S, consts):
    """The case's ticks on the device, once per session: several tests look at the same run."""
    if (S, consts) not in _runs:
        c = VC.case(S, consts)
        _runs[S, consts] = _run(_tracker(device, S, c["constants"]), c["pose"], c["landmarks"], c["valid"], device)
    return _runs[S, consts]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    if not np.array_equal(g, w):
        at = tuple(int(i) for i in np.argwhere(g != w)[0])
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} values differ, first at [tick, stream, ...] = {at}: "
                             f"{np.asarray(got)[at]!r} instead of {np.asarray(want)[at]!r}")


def _check_against_oracle(got, ref, constants, name):
    size = constants[4]
    for k in ("smoothed", "centre", "state"):
        _assert_same_bits(got[k], ref[k], f"{name} {k}")
    assert np.array_equal(got["updated"], ref["updated"]), name
    zeros = {k: np.zeros_like(got[k][0]) for k in KEYS}
    for t in range(len(got["updated"])):                       # a skipped stream: the previous tick's bits (zeros before the first)
        skipped = ~ref["updated"][t]
        for k in KEYS:
            _assert_same_bits(got[k][t][skipped], (got[k][t - 1] if t else zeros[k])[skipped], f"{name} {k} of skipped streams, tick {t}")
    diff = np.abs(got["endpoints"] - ref["endpoints"])
    bound = VC.endpoint_bound(ref["centre"], size)
    unit = EPS * (np.abs(ref["centre"])[..., None, :] + 2.0 * size)
    seeded = ref["state"][..., 5] > 0                          # before a stream's first applied tick both sides hold zeros
    _report(f"video_post_endpoints_{name}", max_in_eps_units=(diff / unit)[seeded].max(), bound_in_eps_units=(bound / unit)[seeded].max(),
            differing=(diff[seeded] > 0).mean())
    assert (diff <= bound).all(), (name, float((diff / unit).max()), float((bound / unit)[seeded].max()))
    applied = ref["updated"]
    e_ref, e_got = ref["endpoints"][applied], got["endpoints"][applied]
    near = np.abs(e_ref - np.rint(e_ref)) <= VC.INT_MARGIN     # int() is only asked for where the oracle's value is clear of an integer
    assert near.mean() <= VC.MAX_INT_EXCLUDED, near.mean()
    assert np.array_equal(np.trunc(e_got)[~near], np.trunc(e_ref)[~near]), name


def _assert_conditions(c):
    q = VC.conditions(c)
    assert q["rounding_differs"] == 0 and q["gate_margin_px"] > VC.GATE_MARGIN_PX and q["int_excluded"] <= VC.MAX_INT_EXCLUDED, q


@pytest.mark.parametrize("consts", sorted(VC.CONSTANTS))
@pytest.mark.parametrize("S", VC.STREAMS)
def test_streams_and_ticks_match_the_oracle(S, consts, device):
    c = VC.case(S, consts)
    _assert_conditions(c)
    _check_against_oracle(_case_run(device, S, consts), c["ref"], c["constants"], f"S{S}_{consts}")


def test_valid_none_means_every_stream_has_a_face(device):
    c = VC.case(65)
    pose = np.nan_to_num(c["pose"][:4], nan=0.25, posinf=-0.5, neginf=0.5)
    every = np.ones(pose.shape[:2], dtype=bool)
    ref = VM.replay(pose, c["landmarks"][:4], every, *c["constants"])
    assert ref["updated"].all()
    _assert_conditions({"pose": pose, "landmarks": c["landmarks"][:4], "constants": c["constants"], "ref": ref})
    got = _run(_tracker(device, 65, c["constants"]), pose, c["landmarks"][:4], None, device)
    _check_against_oracle(got, ref, c["constants"], "S65_valid_none")


def test_plain_entry_point_gives_the_ex_bits(device):
    """nlml_video_post (no `updated` buffer) against nlml_video_post_ex on the same ticks."""
    S = 65
    c = VC.case(S)
    W, H, alpha, max_jump, size = c["constants"]
    want = _case_run(device, S, "default")
    P, L = torch.from_numpy(np.array(c["pose"])).to(device), torch.from_numpy(np.array(c["landmarks"])).to(device)
    V = torch.from_numpy(c["valid"].astype(np.uint8)).to(device)
    buf = {k: torch.zeros(want[k].shape[1:], dtype=torch.float64, device=device) for k in KEYS}
    for t in range(VC.T):
        with ops._on_device_of(("state", buf["state"]), ("pose_rad", P), ("raw", L), ("valid", V)) as stream:
            _lib.check(_lib.lib().nlml_video_post(P[t].data_ptr(), L[t].data_ptr(), V[t].data_ptr(), S, float(W), float(H), alpha,
                                                  max_jump, size, buf["state"].data_ptr(), buf["smoothed"].data_ptr(),
                                                  buf["centre"].data_ptr(), buf["endpoints"].data_ptr(), stream), "nlml_video_post")
        for k in KEYS:
            _assert_same_bits(buf[k].cpu().numpy(), want[k][t], f"plain entry point, {k}, tick {t}")


def test_zero_streams_touches_nothing(device):
    c = VC.case(1)
    W, H, alpha, max_jump, size = c["constants"]
    P, L = torch.from_numpy(np.array(c["pose"][1])).to(device), torch.from_numpy(np.array(c["landmarks"][1])).to(device)
    V = torch.ones(1, dtype=torch.uint8, device=device)
    buf = {k: torch.full(n, 1234.5, dtype=torch.float64, device=device) for k, n in
           (("state", (1, 6)), ("smoothed", (1, 3)), ("centre", (1, 2)), ("endpoints", (1, 3, 2)))}
    upd = torch.full((1,), 7, dtype=torch.uint8, device=device)
    with ops._on_device_of(("state", buf["state"]), ("pose_rad", P)) as stream:
        assert _lib.lib().nlml_video_post_ex(P.data_ptr(), L.data_ptr(), V.data_ptr(), 0, float(W), float(H), alpha, max_jump, size,
                                             buf["state"].data_ptr(), buf["smoothed"].data_ptr(), buf["centre"].data_ptr(),
                                             buf["endpoints"].data_ptr(), upd.data_ptr(), stream) == 0
        assert _lib.lib().nlml_video_post_ex(None, None, None, 0, float(W), float(H), alpha, max_jump, size, None, None, None, None,
                                             None, stream) == 0
    torch.cuda.synchronize(device)
    assert all((b == 1234.5).all() for b in buf.values()) and int(upd[0]) == 7


def test_skipped_rows_keep_their_initial_bits(device):
    """S = 130 with streams 0..64 skipped in every tick (no face, NaN or Inf pose in turn): their rows of every buffer keep the bits
    they started with -- the whole first block and the first stream of the second -- while streams 65..129 advance as in the plain
    run.  A stride or a bound that is off writes into those rows."""
    S, n = 130, 65
    c = VC.case(S)
    pose, valid = np.array(c["pose"]), np.array(c["valid"])
    pose[:, :n] = np.nan_to_num(pose[:, :n], nan=0.1, posinf=0.2, neginf=-0.2)
    for t in range(VC.T):
        if t % 3 == 0:
            valid[t, :n] = False
        else:
            valid[t, :n] = True
            pose[t, :n, t % 3] = np.nan if t % 2 else np.inf
    tr = _tracker(device, S, c["constants"])
    marks = {k: torch.arange(getattr(tr, k)[:n].numel(), dtype=torch.float64, device=device).reshape(getattr(tr, k)[:n].shape) + 0.5
             for k in KEYS}
    for k in KEYS:
        getattr(tr, k)[:n] = marks[k]
    got = _run(tr, pose, c["landmarks"], valid, device)
    for k in KEYS:
        _assert_same_bits(got[k][:, :n], np.broadcast_to(marks[k].cpu().numpy(), got[k][:, :n].shape), f"{k} of the skipped rows")
        _assert_same_bits(got[k][:, n:], _case_run(device, S, "default")[k][:, n:], f"{k} of the live rows")
    assert not got["updated"][:, :n].any() and np.array_equal(got["updated"][:, n:], c["ref"]["updated"][:, n:])
    for k in ("smoothed", "centre", "state"):
        _assert_same_bits(got[k][:, n:], c["ref"][k][:, n:], f"{k} of the live rows against the oracle")


@pytest.mark.parametrize("k", [0, 64, 129])
def test_streams_are_independent(k, device):
    """Stream k of the S = 130 run against the same stream alone in an S = 1 tracker: bit for bit, end points included."""
    c = VC.case(130)
    many = _case_run(device, 130, "default")
    alone = _run(_tracker(device, 1, c["constants"]), c["pose"][:, k:k + 1], c["landmarks"][:, k:k + 1], c["valid"][:, k:k + 1], device)
    for key in KEYS:
        _assert_same_bits(alone[key][:, 0], many[key][:, k], f"stream {k} alone, {key}")
    assert np.array_equal(alone["updated"][:, 0], many["updated"][:, k])


def test_a_move_of_exactly_max_jump_is_accepted(device):
    """The gate keeps the previous centre only if the move is GREATER than max_jump (generatePose_on_video.py:100).  Dyadic landmarks
    put the centre at exactly (480, 540) and then (580, 540): 100 px, accepted at max_jump = 100, rejected one ulp below."""
    lm = np.zeros((2, 1, 468, 3), np.float32)
    lm[:, 0, [1, 33, 263], 0], lm[:, 0, [1, 33, 263], 1] = 0.25, 0.5
    lm[1, 0, 263, 0] = 0.40625
    pose = np.array([[[0.3, -0.2, 0.1]], [[0.25, -0.1, 0.2]]], np.float32)
    every = np.ones((2, 1), dtype=bool)
    for max_jump, centre in ((100.0, [580.0, 540.0]), (float(np.nextafter(100.0, 0.0)), [480.0, 540.0])):
        constants = (1920, 1080, 0.4, max_jump, 80.0)
        ref = VM.replay(pose, lm, every, *constants)
        assert ref["centre"][0, 0].tolist() == [480.0, 540.0] and ref["centre"][1, 0].tolist() == centre
        assert VC.conditions({"pose": pose, "landmarks": lm, "constants": constants, "ref": ref})["rounding_differs"] == 0
        got = _run(_tracker(device, 1, constants), pose, lm, every, device)
        _check_against_oracle(got, ref, constants, f"on_the_gate_{max_jump == 100.0}")


def test_graphed_tick_matches_eager_at_a_partial_tile(head_sds, device):
    """GraphedTick through the model at S = 65 (a second, one-stream block) with no-face rows and a NaN landmark, the replayed input
    changing every tick: the eager tick()'s bits on a second tracker."""
    from nlml_hpe_amd.model import HIPPoseModel
    model = HIPPoseModel(synth.encoder_state_dict(1404, seed=0), head_sds, device=device)
    S, T = 65, 6
    frames = synth.raw_landmarks(S * T, seed=58).reshape(T, S, 468, 3) * np.float32(0.2) + np.float32(0.4)
    no_face = [(0, 64), (1, 3), (2, 63), (2, 64), (4, 64), (5, 0)]
    for t, s in no_face:
        frames[t, s] = 0.0
    frames[3, 64, 10, 0] = np.nan                                   # a NaN pose: skipped and reported, the stream goes on
    frames = torch.from_numpy(frames).to(device)
    a, b = VideoPoseTracker(model, S, 1920, 1080), VideoPoseTracker(model, S, 1920, 1080)
    g = GraphedTick(b)
    before = None
    for t in range(T):
        out_a = a.tick(frames[t])
        g.static_raw.copy_(frames[t])
        out_b = g.replay()
        torch.cuda.synchronize(device)
        for x, y in zip(out_a, out_b):
            assert torch.equal(x, y), t
        assert torch.equal(a.state, b.state) and torch.isfinite(b.state).all()
        applied = out_b[3].cpu().numpy()
        want = np.ones(S, dtype=bool)
        want[[s for tt, s in no_face if tt == t] + ([64] if t == 3 else [])] = False
        assert np.array_equal(applied, want), t
        now = _snapshot(b)
        if before is not None:
            for k in KEYS:
                _assert_same_bits(now[k][~want], before[k][~want], f"graphed tick {t}, {k} of skipped streams")
        before = now
    assert b.state[:, 5].cpu().tolist() == [float(T - sum(1 for _, s in no_face if s == i) - (i == 64)) for i in range(S)]
