"""What the bit-for-bit GPU tests of K2 on exactly summable networks share (tests/test_bf16_exact_gpu.py, tests/test_split_f16_exact_gpu.py):
the packed blob of a pool on the device, shuffled picks of its certified faces, and the comparison of (pose, latent, valid) bits."""
import numpy as np
import torch

from nlml_hpe_amd import _lib, ops, synth, weights
from test_gpu_parity import _report          # the suite's one margins file: a JSON line per measured figure


def _report_pool(name, p, **kv):
    _report(name, worst_bits_needed=max(p["bits"].values()), excluded_share=p["excluded"], **{f"bits_{k}": v for k, v in p["bits"].items()}, **kv)


_blobs: dict = {}


def _blob(p, mode, device):
    key = (p["key"], mode)
    if key not in _blobs:
        _blobs[key] = torch.from_numpy(weights.pack_blob(p["enc"], p["heads"], _lib.mode_from_name(mode))).to(device)
    return _blobs[key]


def _tile(p, B, seed):
    """B picks (with repeats, shuffled) out of the pool's certified faces; the "no face" row is among them when B > 2."""
    idx = synth.rng(seed, 41).integers(0, len(p["x"]), size=B)
    if B > 2:
        idx[B // 2] = 0
    return idx


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, p, idx, tag):
    """got = (pose, latent, valid) tensors; the model's bits for the pool rows idx."""
    pose, lat, valid = got
    bad = np.flatnonzero((_bits(pose) != _bits(p["pose"][idx])).any(axis=1) | (_bits(lat) != _bits(p["latent"][idx])).any(axis=1))
    if len(bad):
        r = int(bad[0])
        lat_cols = np.flatnonzero(_bits(lat)[r] != _bits(p["latent"][idx])[r])
        raise AssertionError(f"{tag}: {len(bad)} of {len(idx)} faces differ, first row {r} (tile row {r % 64}): latent columns {lat_cols.tolist()} "
                             f"got {lat.cpu().numpy()[r].tolist()} want {p['latent'][idx][r].tolist()}; pose got {pose.cpu().numpy()[r].tolist()} "
                             f"want {p['pose'][idx][r].tolist()}")
    assert np.array_equal(valid.cpu().numpy(), p["valid"][idx]), tag


def _fwd(xt, blob, F):
    return ops.encoder_heads_fwd(xt, blob, F, return_latent=True, return_valid=True)
