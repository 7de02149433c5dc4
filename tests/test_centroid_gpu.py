"""Centroid / RMS-radius landmark normalisation on the GPU (csrc/normalize_centroid.hip): the kernel against the reference's recorded
results (FX11) and against the host restatement of the same operation order, bit for bit, and every layer above it.  Reads fixtures
only, never the reference."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nlml_hpe_amd import _lib, ops, synth, weights
from nlml_hpe_amd.model import HIPPoseModel
from nlml_hpe_amd.pipeline import HostPipeline
from test_centroid_host import FX11, host, philox_faces, same_bits

pytestmark = pytest.mark.gpu


def special_faces(n, seed):
    """Philox faces in FX11's three ranges with "no face" rows and an all-equal face mixed in (where the batch has room)."""
    raw = philox_faces(n, seed)
    for b, v in ((0, 0.0), (n // 2, -0.0), (n - 1, 0.0)):
        if n > 3:
            raw[b] = v
    if n > 5:
        raw[n // 3] = np.float32(0.625)
        raw[n // 3 + 1, :, 2] = -0.0
    return raw


def device_call(raw_t, want_valid, want_stats):
    """The C entry point itself on torch's current stream; buffers pre-filled so that an unwritten element shows."""
    B = raw_t.shape[0]
    out = torch.full((B, 1404), 7.0, dtype=torch.float32, device=raw_t.device)
    valid = torch.full((B,), 9, dtype=torch.uint8, device=raw_t.device) if want_valid else None
    stats = torch.full((B, 4), 7.0, dtype=torch.float64, device=raw_t.device) if want_stats else None
    rc = _lib.lib().nlml_normalize_centroid(raw_t.data_ptr(), B, out.data_ptr(), valid.data_ptr() if want_valid else None,
                                            stats.data_ptr() if want_stats else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().nlml_last_error()
    return out, valid, stats


def test_kernel_equals_fx11(device, golden_dir):
    g = np.load(os.path.join(golden_dir, FX11))
    out, valid, stats = ops.normalize_centroid(torch.from_numpy(g["raw"]).to(device), return_valid=True, return_stats=True)
    assert same_bits(out.cpu().numpy(), g["out_bits"].view(np.float32))
    assert np.array_equal(valid.cpu().numpy(), g["valid"].astype(bool))
    st = stats.cpu().numpy()
    assert same_bits(st[:, :3], g["centroid"]) and same_bits(st[:, 3], g["scale"])


@pytest.mark.parametrize("B", [1, 63, 64, 65, 4097, 65537])
def test_kernel_equals_host_restatement(device, B):
    raw = special_faces(B, seed=100 + B)
    exp_out, exp_valid, exp_stats = host(raw)
    side = torch.cuda.Stream(device=device)
    raw_t = torch.from_numpy(raw).to(device)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(side):                   # a non-default stream
        got = [(wv, ws, device_call(raw_t, wv, ws)) for wv in (True, False) for ws in (True, False)]
    side.synchronize()
    for wv, ws, (out, valid, stats) in got:
        assert same_bits(out.cpu().numpy(), exp_out), (B, wv, ws)
        if wv:
            assert np.array_equal(valid.cpu().numpy(), exp_valid), (B, wv, ws)
        if ws:
            assert same_bits(stats.cpu().numpy(), exp_stats), (B, wv, ws)


@pytest.mark.parametrize("B", [24, 21])
def test_kernel_sums_the_squared_norms_in_numpys_order(device, B):
    """The first faces of test_centroid_host.test_pairwise_tree_is_numpys's input (the same draws: coordinates six decimal orders of
    magnitude apart within a face, so the scale depends on the order in which the 468 squared norms are added): three workgroups of
    eight faces, each in two LDS parts, and at 21 a ragged last one."""
    g = synth.rng(43, 0)
    raw = (g.standard_normal((300, 468, 3)) * 10.0 ** g.uniform(-3, 3, (300, 468, 1))).astype(np.float32)[:B]
    exp_out, exp_valid, exp_stats = host(raw)
    a = raw.astype(np.float64)
    n = np.sum((a - np.mean(a, axis=1, keepdims=True)) ** 2, axis=2)
    assert (np.cumsum(n, axis=1)[:, -1] != np.sum(n, axis=1)).any()          # added left to right, the norms give another sum
    out, valid, stats = device_call(torch.from_numpy(raw).to(device), True, True)
    torch.cuda.synchronize(device)
    assert same_bits(stats.cpu().numpy(), exp_stats)
    assert same_bits(out.cpu().numpy(), exp_out)
    assert np.array_equal(valid.cpu().numpy(), exp_valid) and exp_valid.all()


def test_empty_batch(device):
    raw = torch.zeros((0, 468, 3), dtype=torch.float32, device=device)
    out, valid, stats = ops.normalize_centroid(raw, return_valid=True, return_stats=True)
    assert tuple(out.shape) == (0, 1404) and tuple(valid.shape) == (0,) and tuple(stats.shape) == (0, 4)
    assert tuple(torch.ops.nlml_hpe.normalize_centroid(raw).shape) == (0, 1404)
    assert _lib.lib().nlml_normalize_centroid(None, 0, None, None, None, None) == 0


def test_ops_and_torch_ops_agree(device):
    raw = torch.from_numpy(special_faces(777, seed=5)).to(device)
    a = ops.normalize_centroid(raw)
    b = torch.ops.nlml_hpe.normalize_centroid(raw)
    assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    # a strided view is made contiguous by both
    wide = torch.zeros((40, 468, 4), dtype=torch.float32, device=device)
    wide[:, :, :3] = raw[:40]
    assert same_bits(ops.normalize_centroid(wide[:, :, :3]).cpu().numpy(), a[:40].cpu().numpy())
    assert same_bits(torch.ops.nlml_hpe.normalize_centroid(wide[:, :, :3]).cpu().numpy(), a[:40].cpu().numpy())


@pytest.fixture(scope="module")
def state_dicts(head_sds):
    return synth.encoder_state_dict(1404, seed=0), head_sds


@pytest.mark.parametrize("mode", ["f16x2s", "f32", "f16x2", "bf16"])
@pytest.mark.parametrize("B", [96, 5000])      # the layer-per-launch path of the split-f16 modes / the fused kernel
def test_from_landmarks_centroid_is_the_two_launch_form(device, state_dicts, mode, B):
    model = HIPPoseModel(*state_dicts, device=device, mode=mode)
    raw_np = philox_faces(B, seed=7)
    raw_np[B // 2] = 0.0
    raw = torch.from_numpy(raw_np).to(device)
    feats = ops.normalize_centroid(raw)
    y, p, r = model(feats)
    direct = torch.cat([y, p, r], dim=1).cpu().numpy()
    pose, latent, valid = model.from_landmarks(raw, normalization="centroid", return_latent=True, return_valid=True)
    assert same_bits(pose.cpu().numpy(), direct)
    assert same_bits(model.from_landmarks(raw, normalization="centroid").cpu().numpy(), direct)
    exp_valid = np.ones((B,), bool)
    exp_valid[B // 2] = False
    assert np.array_equal(valid.cpu().numpy(), exp_valid)
    assert same_bits(latent.cpu().numpy(), model.forward_packed(feats, return_latent=True)[1].cpu().numpy())
    assert np.isfinite(direct).all()


@pytest.mark.parametrize("B", [96, 5000])
def test_default_normalisation_is_untouched(device, state_dicts, B):
    model = HIPPoseModel(*state_dicts, device=device)
    raw = torch.from_numpy(synth.raw_landmarks(B, seed=9)).to(device)
    fused = ops.landmarks_to_pose(raw, model.blob, True).cpu().numpy()
    assert same_bits(model.from_landmarks(raw).cpu().numpy(), fused)
    assert same_bits(model.from_landmarks(raw, normalization="ipd").cpu().numpy(), fused)
    assert not same_bits(model.from_landmarks(raw, normalization="centroid").cpu().numpy(), fused)


def test_host_pipeline_centroid(device, state_dicts):
    model = HIPPoseModel(*state_dicts, device=device)
    raw = philox_faces(1500, seed=12)
    raw[3] = 0.0
    pose, valid = HostPipeline(model, batch=512, normalization="centroid").run(raw)
    # the pipeline's batches of 512 and 476 faces take the same path the direct call takes at those sizes
    exp = np.concatenate([model.from_landmarks(torch.from_numpy(raw[a:a + 512]).to(device), normalization="centroid").cpu().numpy()
                          for a in range(0, 1500, 512)])
    assert same_bits(pose, exp)
    assert valid.tolist() == [b != 3 for b in range(1500)]
    assert HostPipeline(model, batch=512).normalization == "ipd"


def test_video_tracker_centroid(device, state_dicts):
    from nlml_hpe_amd.video import VideoPoseTracker
    model = HIPPoseModel(*state_dicts, device=device)
    raw = philox_faces(8, seed=13)
    raw[5] = 0.0
    raw_t = torch.from_numpy(raw).to(device)
    a = VideoPoseTracker(model, 8, 640, 480, normalization="centroid")
    sm, _, _, applied = a.tick(raw_t)
    pose = model.from_landmarks(raw_t, normalization="centroid").cpu().numpy().astype(np.float64)
    exp = np.round(np.degrees(pose), 2)          # the first tick's smoothed value is the rounded pose itself
    keep = np.arange(8) != 5
    assert applied.cpu().numpy().tolist() == keep.tolist()
    assert np.allclose(sm.cpu().numpy()[keep], exp[keep], rtol=0, atol=1e-9)


def test_test_entry_point_with_centroid(device, state_dicts, repo_root, tmp_path):
    """NLML_HPE_Test.py --normalization centroid in landmarks-npz mode, as a child process: the poses it prints are the direct
    computation's."""
    import shutil
    import yaml
    n = 300
    raw = philox_faces(n, seed=14)
    raw[11] = 0.0
    gt = synth.poses_deg(n, seed=4)
    np.savez(tmp_path / "val.npz", landmarks=raw, pose=gt)
    os.makedirs(tmp_path / "configs")
    shutil.copy(os.path.join(repo_root, "configs", "config_EncoderTrainer.yaml"), tmp_path / "configs")
    cfg = yaml.safe_load(open(os.path.join(repo_root, "configs", "config_NLML_HPE_Test.yaml")))
    cfg.update(val_set="landmarks_npz", val_set_path=str(tmp_path / "val.npz"))
    yaml.safe_dump(cfg, open(tmp_path / "configs" / "config_NLML_HPE_Test.yaml", "w"))
    os.symlink(os.path.join(repo_root, "models"), tmp_path / "models")
    env = dict(os.environ, PYTHONPATH=repo_root, NLML_HPE_MODE="f16x2s")
    res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(repo_root, "NLML_HPE_Test.py"), "--normalization",
                          "centroid", "--print-poses"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=330)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    printed = {int(line.split(":")[0].split()[1]): line.split(": ")[1] for line in res.stdout.splitlines() if line.startswith("pose ")}
    model = HIPPoseModel(*state_dicts, device=device, mode="f16x2s")      # what resolve_model builds here: synthetic encoder, seed 0
    pose = model.from_landmarks(torch.from_numpy(raw).to(device), normalization="centroid").cpu().numpy()
    pred = np.round(np.degrees(pose.astype(np.float64)), 3)
    lo, hi = np.array([-50, -40, -30.0]), np.array([51, 41, 31.0])
    keep = ((gt >= lo) & (gt <= hi)).all(axis=1)
    keep[11] = False
    assert sorted(printed) == np.flatnonzero(keep).tolist() and len(printed) > 100
    for i in printed:
        assert printed[i] == f"{pred[i, 0]:.3f} {pred[i, 1]:.3f} {pred[i, 2]:.3f}", i
    assert "1 without landmarks" in res.stdout
