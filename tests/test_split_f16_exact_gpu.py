"""The parity modes of K2 (f32, f16x2, f16x2s) bit for bit against exactly summable networks WITH LIVE LO PIECES (tests/exact_nets.py).

The split-f16 kernels accumulate b s + a_hi w_hi + a_lo w_hi + a_hi w_lo per stage (a_lo w_lo dropped); on the pools of
exact_nets.SPLIT_POOLS both lo pieces are non-zero under every stage kind (a_lo under E5 excepted: its input is the saturated Tanh), and
every accumulator is an exact f32 sum in any order and any split over accumulators (certify_split: the three kinds and the scaled bias
together inside 2^20 quanta; every activation hi + lo exactly and below 65,504).  So each kernel has ONE right answer,
exact_nets.reference_split gives it (tests/test_exact_nets_host.py ties that model to the packed blob), and every comparison here is
np.array_equal on the f32 bits of pose and latent and on the validity mask -- the fused kernels, the layer-per-launch path, the
streamed tail, the in-kernel rescue and the f32 re-evaluation launch against the model, never against each other.

Pool E0wx (x in {0, +-1, +-(1 + 2^-11)} under a bumped E0) has a_lo AND w_lo under layer 0: all three kinds on one accumulator, and the
dropped a_lo w_lo is non-zero, so the split model's bits there are NOT the plain f64 forward's -- a split kernel that took the f32 or
rescue arithmetic, or kept lo lo, fails on it.  It runs in the split modes only: whole-f32 products of two 12-bit operands do not
certify.  Behind layer 0 no stage has both lo pieces (26.5 bits at E1, exact_nets.py), so on the other pools the f32 mode's right
answer, the plain f64 forward, is the same bits as the split modes'."""
import numpy as np
import pytest
import torch

import exact_nets as XN
from exact_gpu import _bits, _blob, _fwd, _report_pool, _same, _tile
from nlml_hpe_amd import _lib, ops

pytestmark = pytest.mark.gpu

MODES = ["f32", "f16x2", "f16x2s"]
SPLIT = ["f16x2", "f16x2s"]
LAYER0_POOLS = ["E0w", "E0x", "E0wx"]
SMALL_MAX = 4096 + 37            # the layer-per-launch path's workspace grows with B (11 KB per face): run up to here


def _cases(names):
    """(pool, mode) pairs; E0wx in the split modes only (module docstring)."""
    return [(n, m) for n in names for m in MODES if not (n == "E0wx" and m == "f32")]


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _small(xt, blob, F):
    return ops.encoder_heads_fwd_small(xt, blob, F, return_latent=True, return_valid=True)


_f32_views: dict = {}


def _for_mode(p, mode):
    """The pool as the mode's kernel must answer it.  Split modes: the pool itself.  f32: its faces that certify for whole-f32
    arithmetic (certify(rounded=False): products a w instead of the pieces'), with the plain f64 forward as the answer."""
    if mode != "f32":
        return p
    if p["key"] not in _f32_views:
        ok, worst = XN.certify(p["x"], p["enc"], p["heads"], rounded=False)
        assert ok[0] and ok.mean() >= 1.0 - XN.MAX_EXCLUDED_SHARE, ok.mean()
        pose, lat, valid = XN.reference(p["x"][ok], p["enc"], p["heads"], rounded=False)
        _f32_views[p["key"]] = dict(p, key=p["key"] + ("f32",), x=p["x"][ok], pose=pose, latent=lat, valid=valid, bits=XN.worst_bits(worst, ok),
                                 excluded=1.0 - (1.0 - p["excluded"]) * ok.mean())
    return _f32_views[p["key"]]


def _entry_points(p, mode, idx, device, F, tag, raw_seed=11):
    """Every way into the mode's kernels on the faces idx, each against the model."""
    blob = _blob(p, mode, device)
    xt = _dev(p["x"][idx], device)
    _same(_fwd(xt, blob, F), p, idx, f"{tag} {mode} fused, features")
    if mode in SPLIT and len(idx) <= SMALL_MAX:
        _same(_small(xt, blob, F), p, idx, f"{tag} {mode} layer per launch, features")
    if F != 1404:
        return
    rt = _dev(XN.raw_landmarks(p["x"], seed=raw_seed)[idx], device)
    _same(ops.landmarks_to_pose(rt, blob, True, return_latent=True, return_valid=True), p, idx, f"{tag} {mode} fused, raw landmarks")
    if mode in SPLIT and len(idx) <= SMALL_MAX:
        _same(ops.landmarks_to_pose_small(rt, blob, True, return_latent=True, return_valid=True), p, idx, f"{tag} {mode} layer per launch, raw")
    if mode == "f16x2s":
        _same(ops.landmarks_to_pose_streamed(rt, blob, True, return_latent=True, return_valid=True), p, idx, f"{tag} streamed tail")


# ---- every stage kind --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", _cases(sorted(XN.SPLIT_POOLS)))
def test_every_stage_kind(name, mode, device):
    """Each pool (a bump in the trunk and one behind the Tanh; the x-lo pool) at B = 130 through every entry point of the mode."""
    p = _for_mode(XN.split_pool(name), mode)
    idx = _tile(p, 130, seed=len(name) + 7)
    _entry_points(p, mode, idx, device, 1404, f"pool {name}")
    _report_pool(f"split_exact_{name}_{mode}", p, **{f"cover_{st}_{k}": v for st, c in p["cover"].items() for k, v in c.items() if k != "hi_hi"})


# ---- batch shape -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 31, 32, 33, 63, 64, 65, 127, 300, 4096 + 37, 65536 - 63])
def test_batch_shapes(B, mode, device):
    """Whole and partial tiles, one face, the small path's range and the bench size: certified faces tiled in a shuffled order, so a
    face's bits depend neither on its position nor on its neighbours.  The streamed tail takes every shape (strict-fast blob, raw
    landmarks); the layer-per-launch path runs up to 4,133 faces."""
    p = _for_mode(XN.split_pool("E0w"), mode)
    idx = _tile(p, B, seed=B)
    _entry_points(p, mode, idx, device, 1404, f"B={B}")
    _report_pool(f"split_exact_E0w_{mode}_B{B}", p)


# ---- feature width -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", _cases(LAYER0_POOLS))
@pytest.mark.parametrize("F", [1404, 136, 64, 16, 13, 1407])
def test_feature_widths(F, name, mode, device):
    """Both staging paths (16-byte loads: F % 4 == 0; scalar: 13, 1407), short K, and the padded K tail with non-zero lo pieces of
    the weights (E0w), of x (E0x) and of both (E0wx) next to it."""
    p = _for_mode(XN.split_pool(name, F), mode)
    idx = _tile(p, 130, seed=F)
    _entry_points(p, mode, idx, device, F, f"F={F} pool {name}")
    _report_pool(f"split_exact_{name}_{mode}_F{F}", p)


# ---- row placement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", _cases(LAYER0_POOLS))
def test_row_placement_every_phase_packed_and_unaligned(name, mode, device):
    """The same certified features behind base offsets of 0, 4, ..., 28 floats in line-aligned padded rows, in packed 5,616-byte rows
    and behind an odd float offset / an odd row stride (rows not 16-byte aligned: the scalar staging) -- each against the model."""
    p = _for_mode(XN.split_pool(name), mode)
    blob = _blob(p, mode, device)
    B = 200
    idx = _tile(p, B, seed=5)
    feats = _dev(p["x"][idx], device)
    fwds = [("fused", _fwd)] + ([("layer per launch", _small)] if mode in SPLIT else [])
    for what, fwd in fwds:
        _same(fwd(feats, blob, 1404), p, idx, f"{mode} {what}: packed rows")
        for off in range(0, 32, 4):
            buf = torch.zeros((B, 1408 + 32), dtype=torch.float32, device=device)   # 5,760-byte rows: 45 whole lines
            assert buf.data_ptr() % 128 == 0
            view = buf[:, off:off + 1404]
            view.copy_(feats)
            _same(fwd(view, blob, 1404), p, idx, f"{mode} {what}: line-aligned rows, offset {off} floats")
        for width, off in ((1408, 1), (1441, 0), (1441, 3)):                        # misaligned base / odd stride / both
            buf = torch.zeros((B, width), dtype=torch.float32, device=device)
            view = buf[:, off:off + 1404]
            view.copy_(feats)
            _same(fwd(view, blob, 1404), p, idx, f"{mode} {what}: row stride {width}, offset {off}")


# ---- rescue ------------------------------------------------------------------------------------------------------------------------
def _rescue_layout(p, B, spots, crowd):
    """idx int[B] into the rescue pool: rescued rows (hidden-layer and input overflow alternating) at `spots` and at crowd[0]..crowd[1],
    plain and just-inside rows everywhere else."""
    g = np.random.default_rng(3)
    calm, over = np.flatnonzero(~p["rescued"]), np.flatnonzero(p["rescued"])
    idx = calm[g.integers(0, len(calm), size=B)]
    idx[B // 2 + 1] = 0
    where = list(spots) + list(range(*crowd))
    hidden, inp = over[p["kind"][over] == 2], over[p["kind"][over] == 3]
    for i, r in enumerate(where):
        src = hidden if i % 2 == 0 else inp
        idx[r] = src[(7 * i) % len(src)]
    return idx, np.array(where)


@pytest.mark.parametrize("form", ["fused", "small"])
@pytest.mark.parametrize("mode", SPLIT)
def test_rescue(mode, form, device):
    """Faces whose activations leave f16's range are evaluated again in f32: by the workgroup itself in f16x2 (vector ALUs, weight =
    hi + lo, encoder_heads_f16x2_rescue.h), by a second launch on the f32 image in f16x2s (which rescues nothing in its own kernel: any
    tile with one such face goes to that launch).  Rescued faces at tile rows 0, 31, 32 and 63, in the partial last tile, and a tile
    with 40 of them (ten groups of four in the in-kernel path): a rescued face has the bits of the unscaled face it is a power-of-two
    multiple of, its neighbours -- among them faces scaled to just below 65,504 -- the model's."""
    p = XN.rescue_pool()
    blob = _blob(p, mode, device)
    B = 64 * 3 + 21
    idx, where = _rescue_layout(p, B, spots=(64 + 0, 64 + 31, 64 + 32, 64 + 63, 192 + 5, B - 1), crowd=(128 + 3, 128 + 43))
    assert p["rescued"][idx[where]].all() and p["rescued"][idx].sum() == len(where) and (p["kind"][idx] == 1).sum() >= 20
    xt = _dev(p["x"][idx], device)
    got = _fwd(xt, blob, 1404) if form == "fused" else _small(xt, blob, 1404)
    _same(got, p, idx, f"{mode} {form}: rescue")
    base = p["base"][idx[where]]
    assert np.array_equal(_bits(got[0])[where], _bits(p["pose"][base])) and np.array_equal(_bits(got[1])[where], _bits(p["latent"][base]))
    _report_pool(f"split_exact_rescue_{mode}_{form}", p, rescued=len(where))


@pytest.mark.parametrize("mode", SPLIT)
def test_nan_and_inf_faces_stay_alone(mode, device):
    """NaN, +Inf and -Inf faces at rows 0, 31, 32 and 63 of a tile and in a partial last tile: they take the rescue path and stay
    non-finite; neighbours keep the model's bits (fused kernel and layer-per-launch path)."""
    p = XN.split_pool("E0x")
    blob = _blob(p, mode, device)
    B = 64 * 2 + 40
    idx = _tile(p, B, seed=23)
    x = p["x"][idx].copy()
    rows = [64 + 0, 64 + 31, 64 + 32, 64 + 63, 128 + 5, B - 1]
    for i, r in enumerate(rows):       # column 1403 is the last real one, next to the padded K columns
        x[r, (100, 1403, 0)[(i + i // 3) % 3]] = (np.nan, np.inf, -np.inf)[i % 3]
    keep = np.ones(B, bool)
    keep[rows] = False
    k = torch.from_numpy(keep).to(device)
    for what, fwd in (("fused", _fwd), ("layer per launch", _small)):
        pose, lat, valid = fwd(_dev(x, device), blob, 1404)
        _same((pose[k], lat[k], valid[k]), p, idx[keep], f"{mode} {what}: neighbours of poisoned faces")
        assert not torch.isfinite(pose[~k]).all(dim=1).any(), pose[~k]


# ---- wrappers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_registered_ops_and_graph_replay(mode, device):
    p = _for_mode(XN.split_pool("E0x"), mode)
    blob = _blob(p, mode, device)
    idx = _tile(p, 200, seed=29)
    xt = _dev(p["x"][idx], device)
    rt = _dev(XN.raw_landmarks(p["x"], seed=11)[idx], device)
    want = _dev(p["pose"][idx], device)
    got = [ops.encoder_heads_fwd(xt, blob, 1404), torch.ops.nlml_hpe.encoder_heads_fwd(xt, blob, 1404),
           ops.landmarks_to_pose(rt, blob, True), torch.ops.nlml_hpe.landmarks_to_pose(rt, blob, True)]
    if mode in SPLIT:
        ws = torch.empty((_lib.lib().nlml_encoder_heads_small_workspace_bytes(200, 1404),), dtype=torch.uint8, device=device)
        got += [torch.ops.nlml_hpe.encoder_heads_fwd_small(xt, blob, 1404, ws), torch.ops.nlml_hpe.landmarks_to_pose_small(rt, blob, True, ws)]
    for i, g in enumerate(got):
        assert torch.equal(g.view(torch.int32), want.view(torch.int32)), (mode, i)
    # one hipGraph capture + replay, on other faces than the ones it was captured with
    static_in = xt.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ops.encoder_heads_fwd(static_in, blob, 1404)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_out = ops.encoder_heads_fwd(static_in, blob, 1404)
    idx2 = _tile(p, 200, seed=31)
    static_in.copy_(_dev(p["x"][idx2], device))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, ops.encoder_heads_fwd(static_in, blob, 1404))
    assert np.array_equal(_bits(static_out), _bits(p["pose"][idx2]))


# ---- the all-integer nets (every lo piece zero), f32 activations, through the parity modes ------------------------------------------
@pytest.mark.parametrize("B", [65, 300])
@pytest.mark.parametrize("mode", ["f32", "f16x2", "f16x2s"])
def test_parity_modes_on_exact_nets(mode, B, device):
    """Saturated Tanh, activations kept in f32 (certificate with rounded=False): the f64 value is the one right answer for the f32
    kernel and for the split-f16 modes too -- an integer below 2^22 splits exactly into hi + lo f16 pieces, the weight pre-scale is a
    power of two, and the split accumulators are exact sums again.  An absolute, order-independent answer instead of a tolerance or a
    sibling implementation: fused kernel from features and from raw landmarks; strict-fast also on the layer-per-launch path and
    the streamed-tail path."""
    p = XN.pool(1404, "saturated", rounded=False)
    assert p["excluded"] == 0.0
    blob = _blob(p, mode, device)
    idx = _tile(p, B, seed=100 + B)
    xt = torch.from_numpy(p["x"][idx]).to(device)
    rt = torch.from_numpy(XN.raw_landmarks(p["x"], seed=11)[idx]).to(device)
    _same(_fwd(xt, blob, 1404), p, idx, f"{mode} fused, features")
    _same(ops.landmarks_to_pose(rt, blob, True, return_latent=True, return_valid=True), p, idx, f"{mode} fused, raw landmarks")
    if mode == "f16x2s":
        _same(ops.encoder_heads_fwd_small(xt, blob, 1404, return_latent=True, return_valid=True), p, idx, "layer per launch")
        _same(ops.landmarks_to_pose_small(rt, blob, True, return_latent=True, return_valid=True), p, idx, "layer per launch, raw")
        _same(ops.landmarks_to_pose_streamed(rt, blob, True, return_latent=True, return_valid=True), p, idx, "streamed tail")
    _report_pool(f"exact_unrounded_{mode}_B{B}", p)
