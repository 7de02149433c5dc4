"""Centroid / RMS-radius landmark normalisation without a GPU: the host restatement of the kernel's operation order
(nlml_normalize_centroid_host, csrc/centroid_ref.h) against the reference's recorded results (FX11) and against numpy itself, and the
checks the device entry point makes before any HIP call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nlml_hpe_amd import _lib, ops, synth  # noqa: F401  (ops registers torch.ops.nlml_hpe.*)

BADARG = -1
FAKE = 4096       # an aligned non-null "device" pointer: every call below is refused before it could be used
REF = "/root/reference"
FX11 = "fx11_centroid_normalise.npz"


def host(raw, want_valid=True, want_stats=True):
    """nlml_normalize_centroid_host on raw f32[B,468,3] -> (out f32[B,1404], valid u8[B] | None, stats f64[B,4] | None)."""
    raw = np.ascontiguousarray(raw, np.float32)
    B = raw.shape[0]
    out = np.full((B, 1404), 7.0, np.float32)
    valid = np.full((B,), 9, np.uint8) if want_valid else None
    stats = np.full((B, 4), 7.0, np.float64) if want_stats else None
    rc = _lib.lib().nlml_normalize_centroid_host(raw.ctypes.data, B, out.ctypes.data, valid.ctypes.data if want_valid else None,
                                                 stats.ctypes.data if want_stats else None)
    assert rc == 0, _lib.lib().nlml_last_error()
    return out, valid, stats


def same_bits(a, b):
    """Equal bit for bit, except that any NaN equals any NaN (the sign and payload of 0/0 differ between machines)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(nan_a, nan_b) and np.array_equal(a.view(u)[~nan_a], b.view(u)[~nan_b]))


def numpy_centroid(face):
    """The calls Normalization_using_Centroid makes (helpers/FeatureExtractor.py:17-28), on one face f32[468,3], and the f32 cast of
    its caller (:101) -> (out f32[1404], centroid f64[3], scale f64)."""
    landmark_array = np.array([[float(p[0]), float(p[1]), float(p[2])] for p in face])
    centroid = np.mean(landmark_array, axis=0)
    centered = landmark_array - centroid
    norm_squared = np.sum(centered ** 2, axis=1)
    scale = np.sqrt(np.mean(norm_squared))
    with np.errstate(invalid="ignore", divide="ignore"):
        scaled = centered / scale
    return torch.tensor(scaled.flatten().tolist()).float().numpy(), centroid, scale


def philox_faces(n, seed):
    """n faces in the three coordinate ranges of FX11, by turns."""
    u = synth.rng(seed, 0).random((n, 468, 3))
    k = np.arange(n)[:, None, None] % 3
    return np.where(k == 0, u, np.where(k == 1, u * 640.0, u - 0.5)).astype(np.float32)


def test_host_equals_fx11(golden_dir):
    g = np.load(os.path.join(golden_dir, FX11))
    assert g["raw"].shape == (64, 468, 3) and os.path.getsize(os.path.join(golden_dir, FX11)) < 1_000_000
    out, valid, stats = host(g["raw"])
    assert same_bits(out, g["out_bits"].view(np.float32))
    assert same_bits(stats[:, :3], g["centroid"]) and same_bits(stats[:, 3], g["scale"])
    assert np.array_equal(valid, g["valid"])
    # the fixture holds what its recipe says: 62 finite faces, the NaN face, the sentinel
    ref = g["out_bits"].view(np.float32)
    assert np.isfinite(ref[:62]).all() and np.isnan(ref[62]).all() and not ref[63].any()
    assert g["valid"].tolist() == [1] * 63 + [0] and g["scale"][62] == 0.0


def test_host_equals_numpy_on_philox_faces():
    raw = philox_faces(2001, seed=41)
    raw[7, :, 2] = -0.0                      # a coordinate that is -0 throughout: numpy's sum starts from +0
    raw[8, 100:, :] = 0.0                    # mostly zero, not the sentinel
    out, valid, stats = host(raw)
    differing = 0
    for b in range(raw.shape[0]):
        o, c, s = numpy_centroid(raw[b])
        differing += int(np.count_nonzero(o.view(np.uint32) != out[b].view(np.uint32)))
        differing += int(np.count_nonzero(c.view(np.uint64) != stats[b, :3].view(np.uint64))) + int(np.float64(s).view(np.uint64) != stats[b, 3:].view(np.uint64)[0])
    assert differing == 0
    assert valid.all()


def test_sentinel_nan_and_special_rows():
    raw = philox_faces(6, seed=42)
    raw[1] = 0.0                             # the "no face" row
    raw[2] = -0.0                            # ... with the sign bit set: still no face
    raw[3] = np.float32(-12.5)               # every landmark equal: 0/0
    raw[4, 17, 1] = np.nan
    raw[5, 400, 0] = np.inf
    for want_valid in (True, False):
        for want_stats in (True, False):
            out, valid, stats = host(raw, want_valid, want_stats)
            assert np.isfinite(out[0]).all() and out[0].any()
            assert not out[1].any() and not out[2].any() and not np.signbit(out[1:3]).any()
            assert np.isnan(out[3]).all() and np.isnan(out[4]).all() and np.isnan(out[5]).all()
            if want_valid:
                assert valid.tolist() == [1, 0, 0, 1, 1, 1]
            if want_stats:
                assert not stats[1].any() and not stats[2].any()
                assert stats[3].tolist() == [-12.5, -12.5, -12.5, 0.0]
    # numpy agrees on the rows the bare function is defined for (the sentinel is the extractor's rule, not the function's)
    for b in (0, 3, 4, 5):
        with np.errstate(invalid="ignore"):
            o, _, _ = numpy_centroid(raw[b])
        assert same_bits(o, out[b])
    empty, v0, s0 = host(np.zeros((0, 468, 3), np.float32))
    assert empty.shape == (0, 1404)


def test_pairwise_tree_is_numpys():
    """The mean of the squared norms alone: numpy's np.sum over 468 f64 values against the host function's scale, with values whose
    sum depends on the order (fifteen decimal orders of magnitude apart)."""
    g = synth.rng(43, 0)
    raw = (g.standard_normal((300, 468, 3)) * 10.0 ** g.uniform(-3, 3, (300, 468, 1))).astype(np.float32)
    _, _, stats = host(raw)
    for b in range(raw.shape[0]):
        a = raw[b].astype(np.float64)
        d = a - np.mean(a, axis=0)
        assert np.sqrt(np.sum(np.sum(d ** 2, axis=1)) / 468.0) == stats[b, 3]


def _err():
    return _lib.lib().nlml_last_error().decode()


@pytest.mark.parametrize("case, args, text", [
    ("null raw", (None, 4, FAKE, None, None), "null"),
    ("null out", (FAKE, 4, None, None, None), "null"),
    ("negative B", (FAKE, -1, FAKE, None, None), "negative B"),
    ("misaligned raw", (FAKE + 4, 4, FAKE, None, None), "aligned"),
    ("misaligned out", (FAKE, 4, FAKE + 8, None, None), "aligned"),
    ("misaligned stats", (FAKE, 4, FAKE, None, FAKE + 4), "aligned"),
])
def test_device_entry_point_refuses(case, args, text):
    assert _lib.lib().nlml_normalize_centroid(*args, None) == BADARG, case
    assert text in _err() and "normalize_centroid" in _err(), (case, _err())


def test_host_entry_point_refuses():
    L = _lib.lib()
    buf = np.zeros((1404,), np.float32)
    assert L.nlml_normalize_centroid_host(None, 1, buf.ctypes.data, None, None) == BADARG and "null" in _err()
    assert L.nlml_normalize_centroid_host(buf.ctypes.data, 1, None, None, None) == BADARG and "null" in _err()
    assert L.nlml_normalize_centroid_host(buf.ctypes.data, -1, buf.ctypes.data, None, None) == BADARG and "negative" in _err()


def test_meta_kernel_shapes():
    raw = torch.empty((5, 468, 3), dtype=torch.float32, device="meta")
    out = torch.ops.nlml_hpe.normalize_centroid(raw)
    assert tuple(out.shape) == (5, 1404) and out.dtype == torch.float32 and out.device.type == "meta"
    assert tuple(torch.ops.nlml_hpe.normalize_centroid(raw[:0]).shape) == (0, 1404)


def test_cpu_tensor_is_refused():
    with pytest.raises(_lib.NlmlError, match="no CPU fallback"):
        ops.normalize_centroid(torch.zeros((2, 468, 3)))
    with pytest.raises(Exception):
        torch.ops.nlml_hpe.normalize_centroid(torch.zeros((2, 468, 3)))


def test_centroid_without_normalisation_is_refused():
    from nlml_hpe_amd.model import HIPPoseModel
    from nlml_hpe_amd.pipeline import HostPipeline
    m = HIPPoseModel.__new__(HIPPoseModel)      # no GPU here: the refusal comes before anything touches the device
    m.input_size, m.device = 1404, torch.device("cuda:0")
    raw = torch.zeros((2, 468, 3))
    with pytest.raises(ValueError, match="centroid"):
        m.from_landmarks(raw, normalize=False, normalization="centroid")
    with pytest.raises(ValueError, match="unknown normalization"):
        m.from_landmarks(raw, normalization="rms")
    with pytest.raises(ValueError):
        HostPipeline(m, normalize=False, normalization="centroid")
    with pytest.raises(ValueError, match="unknown normalization"):
        HostPipeline(m, normalization="rms")


@pytest.mark.parametrize("script", ["NLML_HPE_Test.py", "generatePose_on_video.py", "TD_Inference.py"])
def test_entry_points_offer_the_flag(script, repo_root):
    res = subprocess.run([sys.executable, os.path.join(repo_root, script), "--help"], cwd=repo_root, capture_output=True, text=True,
                         env=dict(os.environ, PYTHONPATH=repo_root), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "--normalization {ipd,centroid}" in res.stdout


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout")
def test_fx11_regenerates_bit_identically(tmp_path, repo_root, golden_dir):
    env = dict(os.environ, NLML_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    res = subprocess.run([sys.executable, os.path.join(golden_dir, "make_golden_centroid.py")], cwd=repo_root, env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    a, b = np.load(os.path.join(str(tmp_path), FX11)), np.load(os.path.join(golden_dir, FX11))
    assert set(a.files) == set(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        if k == "out_bits":
            assert same_bits(a[k].view(np.float32), b[k].view(np.float32)), k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
