"""The bf16 K2 kernel (encoder_heads_bf16_w8.hip) bit for bit against exactly summable networks (tests/exact_nets.py).

Every accumulator of these networks is an exact sum in f32 whatever the order (certified per face: sum|addends| + |bias| < 2^20 quanta),
so the kernel has one correct answer per rounding point and oracle.encoder_heads.forward_bf16_emulated gives it.  Every comparison is
np.array_equal on the f32 bits of pose and latent and on the validity mask.  The parity modes (f32, f16x2, f16x2s) have their own file,
tests/test_split_f16_exact_gpu.py.

Live-Tanh form: the device's tanhf, measured against the f64 tanh on these networks' own E4 pre-activations: 1.27 f32 ulps at most
(test_device_tanhf_error_is_inside_the_tie_margin measures it again on every run, reports it and asserts it stays <= margin / 8); the
margin around a bf16 tie is 8 x 1.27 rounded up to a power of two = 16 ulps, which leaves out 0-4.3 % of the faces (cap: 15 %)."""
import numpy as np
import pytest
import torch

import exact_nets as XN
from exact_gpu import _bits, _blob, _fwd, _report, _report_pool, _same, _tile
from nlml_hpe_amd import _lib, ops, synth, weights

pytestmark = pytest.mark.gpu


def _live_cap(p):
    assert p["excluded"] <= XN.MAX_EXCLUDED_SHARE, p["excluded"]


# ---- the device's tanhf, measured --------------------------------------------------------------------------------------------------
def _device_tanhf(z, heads, device):
    """tanhf of the f32 values z on the device, through the f32 K2 kernel: synth.passthrough_encoder_state_dict builds x_i = relu(x_i) -
    relu(-x_i) in front of the Tanh layer and hands tanh(x_i) to the latent through a single 1.0 weight, all of it exact."""
    F = 16
    sd = synth.passthrough_encoder_state_dict(F, out_gain=1.0)
    blob = torch.from_numpy(weights.pack_blob(sd, heads, _lib.MODE_F32)).to(device)
    flat = np.asarray(z, np.float32).ravel()
    n = (len(flat) + 8) // 9
    x = np.zeros((n, F), np.float32)
    x[:, :9].flat[:len(flat)] = flat
    _, lat = ops.encoder_heads_fwd(torch.from_numpy(x).to(device), blob, F, return_latent=True)
    return lat.cpu().numpy().ravel()[:len(flat)].reshape(np.shape(z))


@pytest.mark.parametrize("F", [1404, 136, 13])
def test_device_tanhf_error_is_inside_the_tie_margin(F, device):
    """Reference: numpy's f64 tanh.  Measured on the live nets' own E4 pre-activations: 1.17 / 1.27 / 1.22 f32 ulps at most (mean 0.26);
    the tie margin (16 ulps) stands as long as the figure stays <= 2 = margin / 8."""
    p = XN.pool(F, "live")
    z = XN.e4_preactivations(p["x_all"], p["enc"], p["heads"])
    t_dev = _device_tanhf(z, p["heads"], device).astype(np.float64)
    t = np.tanh(z.astype(np.float64))
    ulp = np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
    err = np.abs(t_dev - t) / ulp
    _report(f"device_tanhf_vs_f64_F{F}", max_ulps=err.max(), mean_ulps=err.mean(), values=z.size, margin_ulps=XN.LIVE_TIE_MARGIN_ULPS,
            excluded_share=p["excluded"])
    print(f"tanhf on {z.size} E4 pre-activations (|z| <= {np.abs(z).max():.3f}): max {err.max():.3f} ulp, mean {err.mean():.3f}")
    assert 8 * err.max() <= XN.LIVE_TIE_MARGIN_ULPS, err.max()


# ---- batch shape -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 31, 32, 33, 63, 64, 65, 127, 300, 4096 + 37, 65536 - 63])
def test_batch_shapes_saturated(B, device):
    """Whole and partial tiles (rows beyond B are clamped to B - 1 and must not be written), one face, the bench size; a few hundred
    certified faces tiled in a shuffled order, so a face's bits do not depend on its position or its neighbours either."""
    p = XN.pool(1404, "saturated")
    idx = _tile(p, B, seed=B)
    xt = torch.from_numpy(p["x"]).to(device)[torch.from_numpy(idx).to(device)]
    _same(_fwd(xt, _blob(p, "bf16", device), 1404), p, idx, f"B={B}")
    _report_pool(f"bf16_exact_saturated_B{B}", p)


@pytest.mark.parametrize("B", [300, 4096 + 37])
def test_batch_shapes_live_tanh(B, device):
    p = XN.pool(1404, "live")
    _live_cap(p)
    idx = _tile(p, B, seed=B + 1)
    xt = torch.from_numpy(p["x"]).to(device)[torch.from_numpy(idx).to(device)]
    _same(_fwd(xt, _blob(p, "bf16", device), 1404), p, idx, f"live B={B}")
    _report_pool(f"bf16_exact_live_B{B}", p, tanhf_measured_ulps=XN.TANHF_MEASURED_ULPS, tie_margin_ulps=XN.LIVE_TIE_MARGIN_ULPS)


# ---- feature width -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["saturated", "live"])
@pytest.mark.parametrize("F", [1404, 136, 64, 16, 13, 1407])
def test_feature_widths(F, form, device):
    """Both staging instantiations (16-byte loads: F % 4 == 0; scalar: 13, 1407), two slabs only (F <= 128: the prologue's third slab is
    the clamped second), the padded tail of K (zero weights over re-read columns)."""
    assert _lib.lib().nlml_encoder_heads_packed_bytes(F, _lib.MODE_BF16) > 0
    p = XN.pool(F, form)
    _live_cap(p)
    B = 130
    idx = _tile(p, B, seed=F)
    xt = torch.from_numpy(p["x"][idx]).to(device)
    _same(_fwd(xt, _blob(p, "bf16", device), F), p, idx, f"F={F} {form}")
    _report_pool(f"bf16_exact_{form}_F{F}", p)


# ---- row placement -----------------------------------------------------------------------------------------------------------------
def test_row_placement_every_phase_packed_and_unaligned(device):
    """The units of a slab's first 128-byte line are loaded one slab ahead, by the row's phase within its line (`xphase`, eight values).
    The same certified features behind base offsets of 0, 4, ..., 28 floats in line-aligned padded rows, in packed 5,616-byte rows
    (phase changes from row to row), and behind an odd float offset / an odd row stride (rows not 16-byte aligned: the scalar path) --
    each against the model, not against another launch."""
    p = XN.pool(1404, "saturated")
    blob = _blob(p, "bf16", device)
    B = 333
    idx = _tile(p, B, seed=5)
    feats = torch.from_numpy(p["x"][idx]).to(device)
    assert feats.data_ptr() % 128 == 0
    _same(_fwd(feats, blob, 1404), p, idx, "packed rows")
    for off in range(0, 32, 4):
        buf = torch.zeros((B, 1408 + 32), dtype=torch.float32, device=device)   # 5,760-byte rows: 45 whole lines
        assert buf.data_ptr() % 128 == 0
        view = buf[:, off:off + 1404]
        view.copy_(feats)
        assert (view.data_ptr() >> 4) & 7 == off // 4
        _same(_fwd(view, blob, 1404), p, idx, f"line-aligned rows, offset {off} floats")
    for width, off in ((1408, 1), (1441, 0), (1441, 3)):                        # misaligned base / odd stride / both
        buf = torch.zeros((B, width), dtype=torch.float32, device=device)
        view = buf[:, off:off + 1404]
        view.copy_(feats)
        _same(_fwd(view, blob, 1404), p, idx, f"scalar path, row stride {width}, offset {off}")


# ---- fused raw landmarks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
def test_fused_raw_landmarks(normalize, device):
    """Raw landmarks in eighths with a power-of-two IPD: the in-kernel f64 normalisation is exact, so the fused launch must give the
    model's bits on the certified integers (normalize=True) or on the raw coordinates themselves (False), equal K1 -> K2, and flag
    the all-zero face."""
    p = XN.pool(1404, "saturated")
    blob = _blob(p, "bf16", device)
    raw_pool = XN.raw_landmarks(p["x"], seed=11)
    if normalize:
        q = p
    else:
        flat = raw_pool.reshape(len(raw_pool), 1404)
        ok, worst = XN.certify(flat, p["enc"], p["heads"])
        assert ok[0] and ok.mean() >= 0.9
        pose, lat, valid = XN.reference(flat[ok], p["enc"], p["heads"])
        q = {"x": flat[ok], "pose": pose, "latent": lat, "valid": valid, "bits": XN.worst_bits(worst, ok), "excluded": 1.0 - ok.mean()}
        raw_pool = raw_pool[ok]
    idx = _tile(q, 300, seed=17)
    rt = torch.from_numpy(raw_pool[idx]).to(device)
    fused = ops.landmarks_to_pose(rt, blob, normalize, return_latent=True, return_valid=True)
    _same(fused, q, idx, f"fused normalize={normalize}")
    assert not bool(fused[2][150]) and int(fused[2].sum()) == int(q["valid"][idx].sum())
    two_step = _fwd(ops.normalize_ipd(rt, normalize), blob, 1404)
    for a, b in zip(fused, two_step):
        assert torch.equal(a, b)
    _report_pool(f"bf16_exact_fused_norm{int(normalize)}", q)


# ---- isolation ---------------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_faces_stay_alone(device):
    """NaN, +Inf and -Inf faces at positions 0, 31, 32 and 63 of a tile and in a partial last tile (its last row is also what the dead
    rows are clamped to): neighbours keep the model's bits, the poisoned faces come out non-finite."""
    p = XN.pool(1404, "saturated")
    blob = _blob(p, "bf16", device)
    B = 64 * 2 + 40
    idx = _tile(p, B, seed=23)
    x = p["x"][idx].copy()
    rows = [64 + 0, 64 + 31, 64 + 32, 64 + 63, 128 + 5, B - 1]
    for i, r in enumerate(rows):       # column 1403 is the last real one: its clamped re-read feeds the padded K columns
        x[r, (100, 1403, 0)[(i + i // 3) % 3]] = (np.nan, np.inf, -np.inf)[i % 3]
    pose, lat, valid = _fwd(torch.from_numpy(x).to(device), blob, 1404)
    keep = np.ones(B, bool)
    keep[rows] = False
    k = torch.from_numpy(keep).to(device)
    _same((pose[k], lat[k], valid[k]), p, idx[keep], "neighbours of poisoned faces")
    assert not torch.isfinite(pose[~k]).all(dim=1).any(), pose[~k]


# ---- wrappers ----------------------------------------------------------------------------------------------------------------------
def test_registered_ops_and_graph_replay(device):
    p = XN.pool(1404, "saturated")
    blob = _blob(p, "bf16", device)
    idx = _tile(p, 200, seed=29)
    xt = torch.from_numpy(p["x"][idx]).to(device)
    rt = torch.from_numpy(XN.raw_landmarks(p["x"], seed=11)[idx]).to(device)
    want = torch.from_numpy(p["pose"][idx]).to(device)
    for got in (ops.encoder_heads_fwd(xt, blob, 1404), torch.ops.nlml_hpe.encoder_heads_fwd(xt, blob, 1404),
                ops.landmarks_to_pose(rt, blob, True), torch.ops.nlml_hpe.landmarks_to_pose(rt, blob, True)):
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
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
    static_in.copy_(torch.from_numpy(p["x"][idx2]).to(device))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, ops.encoder_heads_fwd(static_in, blob, 1404))
    assert np.array_equal(_bits(static_out), _bits(p["pose"][idx2]))
