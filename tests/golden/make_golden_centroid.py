#!/usr/bin/env python3
"""Generate tests/golden/fx11_centroid_normalise.npz by running the reference's own centroid normalisation.

Run ONCE in the build container (needs /root/reference; the GPU box has neither the reference nor a need to run this):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_centroid.py

What is imported from /root/reference and called (file:line of the callee):
  FX11 helpers/FeatureExtractor.py:17  Normalization_using_Centroid   once per face, on landmark objects with .x/.y/.z as FaceMesh gives
                                                                     them; the returned list goes through torch.tensor(...).float() as at :101
The centroid and the scale are locals of that function: they are recorded by handing the reference module a numpy proxy that notes
what its np.mean (first call: the centroid) and np.sqrt (the scale) return.

64 faces from Generator G (nlml_hpe_amd/synth.py rng), seed 11:
   0..20   coordinates U(0, 1)            FaceMesh's normalised image coordinates
  21..41   U(0, 1) * 640                  pixel scale
  42..61   U(-0.5, 0.5)                   centred at 0
  62       every landmark equal           scale 0: the function returns 0/0 = NaN everywhere, and so must the kernel
  63       all zero                       the extractor's "no face" row.  The bare function returns NaN there too, but
                                          get_feature_vector never calls it for such a frame: it returns the zero row
                                          (FeatureExtractor.py:105-106).  The fixture records THAT: out = 0, centroid = scale = 0,
                                          valid = 0 -- written here, not returned by the reference.
Nothing of the reference's source is written to the fixture: it holds the inputs and the numbers the reference returned.
"""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.environ.get("NLML_GOLDEN_OUT", HERE)      # where the fixture is written (the regeneration test uses a temp dir)
# The reference first on sys.path; the repo root (which holds files named like the reference's modules) must not shadow it.
sys.path[:] = [p for p in sys.path if os.path.abspath(p or os.getcwd()) != REPO]
sys.path.insert(0, REF)
sys.path.insert(1, REPO)
sys.dont_write_bytecode = True

for _n in ("cv2", "mediapipe"):
    sys.modules.setdefault(_n, types.ModuleType(_n))

import torch  # noqa: E402

from nlml_hpe_amd import synth  # noqa: E402

SEED = 11
N_FACES = 64


def _ref(name: str):
    """Import a module of the reference and make sure it IS the reference's file (not a same-named file of this repo)."""
    import importlib
    mod = importlib.import_module(name)
    path = os.path.abspath(getattr(mod, "__file__", "") or "")
    if not path.startswith(REF + os.sep):
        raise ImportError(f"{name} resolved to {path}, not to the reference under {REF}")
    return mod


class _NumpyProxy:
    """numpy, noting what mean and sqrt return."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        attr = getattr(np, name)
        if name not in ("mean", "sqrt"):
            return attr

        def noted(*a, **k):
            r = attr(*a, **k)
            self.log.append((name, r))
            return r
        return noted


def inputs() -> np.ndarray:
    """raw f32[64,468,3]; the recipe in the module docstring."""
    raw = np.zeros((N_FACES, 468, 3), np.float32)
    for b in range(62):
        u = synth.rng(SEED, b).random((468, 3))
        v = u if b < 21 else (u * 640.0 if b < 42 else u - 0.5)
        raw[b] = v.astype(np.float32)
    raw[62] = np.float32(0.37)
    return raw


def fx11_centroid_normalise():
    FE = _ref("helpers.FeatureExtractor")
    raw = inputs()
    out = np.zeros((N_FACES, 1404), np.float32)
    centroid = np.zeros((N_FACES, 3), np.float64)
    scale = np.zeros((N_FACES,), np.float64)
    valid = np.ones((N_FACES,), np.uint8)
    real_np = FE.np
    try:
        for b in range(N_FACES - 1):
            proxy = _NumpyProxy()
            FE.np = proxy
            landmark = [types.SimpleNamespace(x=float(p[0]), y=float(p[1]), z=float(p[2])) for p in raw[b]]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)      # face 62: 0/0
                lst = FE.Normalization_using_Centroid(landmark)
            out[b] = torch.tensor(lst[0:1404]).float().numpy()       # FeatureExtractor.py:101
            means = [r for n, r in proxy.log if n == "mean"]
            centroid[b] = means[0]
            scale[b] = [r for n, r in proxy.log if n == "sqrt"][0]
    finally:
        FE.np = real_np
    valid[63] = 0          # the sentinel row: what get_feature_vector returns (see the docstring), not a call of the function
    assert np.isnan(out[62]).all() and scale[62] == 0.0 and np.isfinite(out[:62]).all()
    np.savez_compressed(os.path.join(OUT, "fx11_centroid_normalise.npz"), raw=raw, out_bits=out.view(np.uint32), centroid=centroid,
                        scale=scale, valid=valid)
    print("FX11 written:", os.path.join(OUT, "fx11_centroid_normalise.npz"))


if __name__ == "__main__":
    fx11_centroid_normalise()
