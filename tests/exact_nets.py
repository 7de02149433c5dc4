"""Networks on which every accumulation of the K2 forward is EXACT -- test helper.

If every addend of an accumulator is an integer multiple of a quantum q and sum|addends| + |bias| < 2^24 q, an f32 accumulation is
exact in any order; with 2^20 q it is exact on a matrix instruction that aligns its addends to the largest one and keeps a few guard
bits as well (profiles/r03_mfma_f16_numerics_probe.txt measures ~3 for the f16 instruction; the bf16 one has not been probed, hence
four spare bits).  On such a network a kernel has ONE correct answer per rounding point, and a numpy model that sums in f64 and rounds
where the kernel rounds gives it: oracle.encoder_heads.forward_bf16_emulated for the bf16 mode, the plain f64 forward for the modes that
keep f32 activations.  Integer sums land on bf16 ties all the time (257 -> 256, 259 -> 260), so round-to-nearest-even is exercised.

  make(F, seed, ...)        integer-valued x, +-1 weights (dense or a few per row), small integer biases, from synth.rng (portable bits)
  certify(x, enc, heads)    per face: does every accumulator of the 6 + 3 x 5 stages meet the bound?  + the worst bits per stage
  reference(x, enc, heads)  the answer: (pose f32[B,3], latent f32[B,9], valid bool[B])
  tanh_tie_clear(...)       live-Tanh form: faces whose Tanh outputs stay `margin` f32 ulps away from every bf16 rounding tie
  raw_landmarks(x, seed)    raw [B,468,3] whose IPD-normalised features are exactly x
"""
from __future__ import annotations

import numpy as np

from nlml_hpe_amd import synth
from oracle import encoder_heads as EH

ENCODER_OUT = (1024, 512, 256, 128, 64, 9)
HEAD_SHAPES = ((128, 3), (256, 128), (128, 256), (64, 128), (1, 64))   # == nlml_hpe_amd.weights.HEAD_SHAPES
STAGE_NAMES = ("E0", "E1", "E2", "E3", "E4", "E5") + tuple(f"{n}.H{i}" for n in EH.HEAD_NAMES for i in range(5))
_STREAM = 40          # Philox stream ids 40.. of synth.rng belong to this file

# non-zero weights per row (None: dense).  Dense where K is small or the inputs are small, a few per row where the inputs are large.
DEFAULT_NNZ = {"E0": None, "E1": None, "E2": 16, "E3": 16, "E4": 16, "E5": None, "H0": None, "H1": 16, "H2": 16, "H3": 16, "H4": None}
# live Tanh: the Tanh outputs carry bf16's own 2^-8 relative quantum, so a dense E5 row needs ~20 bits; 16 per row needs ~15
LIVE_NNZ = dict(DEFAULT_NNZ, E5=16)
SATURATING_GAIN = 64.0   # E4 pre-activations are 0 or |z| >= 64: tanh is exactly 0 or +-1 in f32 and f64 on any math library


def _pm1(g, n_out, n_in, nnz):
    w = (2 * g.integers(0, 2, size=(n_out, n_in)) - 1).astype(np.float32)
    if nnz is not None and nnz < n_in:
        keep = np.argsort(g.random((n_out, n_in)), axis=1)[:, :nnz]
        m = np.zeros((n_out, n_in), bool)
        np.put_along_axis(m, keep, True, axis=1)
        w *= m
    return w


def _ibias(g, n):
    return g.integers(-2, 3, size=n).astype(np.float32)


def make(F: int, seed: int, tanh: str = "saturated", B: int = 128, nnz: dict | None = None):
    """-> (encoder state dict, {head: state dict}, x f32[B,F]); x integers in [-2,2] with row 0 all zero (the "no face" row) and,
    for F >= 792, the structure raw_landmarks() needs: landmark 1 at the origin, landmarks 33 and 263 one unit apart along x."""
    assert tanh in ("saturated", "live")
    nz = dict(LIVE_NNZ if tanh == "live" else DEFAULT_NNZ)
    nz.update(nnz or {})
    g = synth.rng(seed, _STREAM)
    x = g.integers(-2, 3, size=(B, F)).astype(np.float32)
    if F >= 6:
        x[:, 3:6] = 0.0
    if F >= 792:
        x[:, 99:102] = x[:, 789:792]
        x[:, 99] = x[:, 789] + 1.0          # may reach 3: still a small integer
    x[0] = 0.0
    enc, fan_in = {}, F
    for i, width in enumerate(ENCODER_OUT):
        enc[f"encoder.{2 * i}.weight"] = _pm1(g, width, fan_in, nz[f"E{i}"])
        enc[f"encoder.{2 * i}.bias"] = _ibias(g, width)
        fan_in = width
    heads = {}
    for n in EH.HEAD_NAMES:
        heads[n] = {}
        for i, (n_out, n_in) in enumerate(HEAD_SHAPES):
            heads[n][f"model.{2 * i}.weight"] = _pm1(g, n_out, n_in, nz[f"H{i}"])
            heads[n][f"model.{2 * i}.bias"] = _ibias(g, n_out)
    if tanh == "saturated":
        enc["encoder.8.weight"] = enc["encoder.8.weight"] * np.float32(SATURATING_GAIN)
        enc["encoder.8.bias"] = np.zeros(64, np.float32)
    else:
        # a power of two that brings the largest |z| of this batch to <= 2 (weights and bias alike: still one quantum per row)
        z = _walk(x, enc, heads, True, upto=5)[4]["z"]
        shift = max(0, int(np.ceil(np.log2(max(np.abs(z).max(), 1.0)))) - 1)
        s = np.float32(2.0 ** -shift)
        enc["encoder.8.weight"] = enc["encoder.8.weight"] * s
        enc["encoder.8.bias"] = enc["encoder.8.bias"] * s
    return enc, heads, x


def _r(h, rounded):
    return EH._bf16_round(h.astype(np.float32)).astype(np.float64) if rounded else h


def _walk(x, enc_sd, head_sds, rounded, upto=None):
    """The 21 stages in f64: a list of dict(name, a = input, w, b, z = pre-activation, h = what the next stage reads)."""
    p = EH.Params(enc_sd, head_sds)
    out = []
    h = _r(np.asarray(x, np.float64), rounded)
    for li, (w, b) in enumerate(p.enc):
        w64 = _r(w.astype(np.float64), rounded)
        z = h @ w64.T + b.astype(np.float64)
        a = h
        h = np.maximum(z, 0) if li < 4 else (np.tanh(z) if li == 4 else z)
        if li < 5:
            h = _r(h, rounded)
        out.append({"name": f"E{li}", "a": a, "w": w64, "b": b.astype(np.float64), "z": z, "h": h})
        if upto is not None and len(out) >= upto:
            return out
    lat = _r(h, rounded)
    for g, n in enumerate(EH.HEAD_NAMES):
        h = lat[:, 3 * g:3 * g + 3]
        for li, (w, b) in enumerate(p.heads[n]):
            w64 = _r(w.astype(np.float64), rounded)
            z = h @ w64.T + b.astype(np.float64)
            a = h
            h = _r(np.maximum(z, 0), rounded) if li < 4 else z
            out.append({"name": f"{n}.H{li}", "a": a, "w": w64, "b": b.astype(np.float64), "z": z, "h": h})
    return out


def _lsb_exp(v):
    """Exponent of the lowest set bit of each f64 (its place value is 2^that); +inf where v == 0."""
    m, e = np.frexp(np.abs(v))
    mant = (m * 2.0 ** 53).astype(np.int64)
    low = mant & -mant
    tz = np.zeros(mant.shape)
    np.log2(low, out=tz, where=mant != 0)
    return np.where(mant != 0, e - 53 + tz, np.inf)


def _row_quantum_exp(a, w, b):
    """log2 q per (face, neuron): the smallest place value among the row's non-zero products and its bias.  The place value of a
    product of two binary floats is the product of their place values, so this is a min-plus product of two small-alphabet matrices."""
    la, lw = _lsb_exp(a), _lsb_exp(w)
    q = np.broadcast_to(_lsb_exp(b)[None, :], (a.shape[0], w.shape[0])).copy()
    for ew in np.unique(lw[np.isfinite(lw)]):
        mw = (lw == ew).astype(np.float32)
        for ea in np.unique(la[np.isfinite(la)]):
            present = ((la == ea).astype(np.float32) @ mw.T) > 0
            q = np.where(present, np.minimum(q, ea + ew), q)
    return q


def certify(x, enc_sd, head_sds, rounded: bool = True, bits: int = 20, return_stages: bool = False):
    """-> (ok bool[B], worst {stage: bits needed}): ok[f] iff sum|w a| + |b| < 2^bits q at every neuron of every stage for face f.
    rounded: activations and weights pass through bf16 where the bf16 kernel rounds them; False: the f32-activation modes."""
    stages = _walk(x, enc_sd, head_sds, rounded)
    ok = np.ones(len(x), bool)
    worst = {}
    for st in stages:
        s = np.abs(st["a"]) @ np.abs(st["w"]).T + np.abs(st["b"])[None, :]
        lq = _row_quantum_exp(st["a"], st["w"], st["b"])
        need = np.where(s > 0, np.log2(np.where(s > 0, s, 1.0)) - np.where(np.isfinite(lq), lq, 0.0), -np.inf)
        ok &= (s < 2.0 ** bits * 2.0 ** np.where(np.isfinite(lq), lq, 0.0)).all(axis=1)
        worst[st["name"]] = need.max(axis=1)            # per face, reduced by the caller over the faces it keeps
    if return_stages:
        return ok, worst, stages
    return ok, worst


def worst_bits(worst: dict, faces=None) -> dict:
    """Per-stage maximum of certify()'s per-face figures over `faces` (default all); the heads' stages merged by layer."""
    out = {}
    for name, v in worst.items():
        v = v if faces is None else v[faces]
        key = name.split(".")[-1]
        out[key] = max(out.get(key, -np.inf), float(v.max()))
    return out


def reference(x, enc_sd, head_sds, rounded: bool = True):
    """The exact answer -> (pose f32[B,3], latent f32[B,9], valid bool[B])."""
    p = EH.Params(enc_sd, head_sds)
    if rounded:
        pose, lat = EH.forward_bf16_emulated(x, p)
    else:
        pose, lat = EH.forward_numpy(x, p, np.float64), EH.encoder_latent_numpy(x, p, np.float64)
    pose32, lat32 = pose.astype(np.float32), lat.astype(np.float32)
    assert np.array_equal(pose32.astype(np.float64), pose) and np.array_equal(lat32.astype(np.float64), lat), "not exact in f32"
    return pose32, lat32, (np.asarray(x) != 0).any(axis=1)


def tie_distance_ulps(t):
    """Distance of each f64 value from the nearest f32 -> bf16 rounding tie of its binade, in f32 ulps (inf for 0)."""
    t = np.abs(np.asarray(t, np.float64))
    _, e = np.frexp(t)
    ulp32, ulp16 = 2.0 ** (e - 24.0), 2.0 ** (e - 8.0)
    tie = np.floor(t / ulp16) * ulp16 + 0.5 * ulp16
    return np.where(t > 0, np.abs(t - tie) / ulp32, np.inf)


def tanh_tie_clear(x, enc_sd, head_sds, margin_ulps: float):
    """bool[B]: every Tanh output of the face lies at least margin_ulps f32 ulps from a bf16 tie, so a tanhf that is within
    margin_ulps of the f64 tanh rounds to the same bf16 value as the model."""
    z = _walk(x, enc_sd, head_sds, True, upto=5)[4]["z"]
    return (tie_distance_ulps(np.tanh(z)) >= margin_ulps).all(axis=1)


def e4_preactivations(x, enc_sd, head_sds):
    """f32[B,64]: the (exact) E4 pre-activations of the bf16 model -- what the live form's Tanh sees."""
    z = _walk(x, enc_sd, head_sds, True, upto=5)[4]["z"]
    z32 = z.astype(np.float32)
    assert np.array_equal(z32.astype(np.float64), z)
    return z32


def raw_landmarks(x, seed: int):
    """x f32[B,1404] from make() -> raw f32[B,468,3], coordinates multiples of 1/8, with (raw - landmark 1) / IPD == x in exact f64
    arithmetic: raw = origin + ipd * x, ipd a power of two in [1/8, 2], origin multiples of 1/8; landmarks 33 and 263 differ by
    (ipd, 0, 0), so the IPD is exactly ipd.  An all-zero x row becomes all-zero landmarks (IPD 0 -> 1e-6 -> features 0: no face)."""
    x = np.asarray(x, np.float64)
    B = len(x)
    assert x.shape[1] == 1404 and not x[:, 3:6].any()
    g = synth.rng(seed, _STREAM + 1)
    ipd = 2.0 ** g.integers(-3, 2, size=B).astype(np.float64)
    origin = g.integers(0, 9, size=(B, 3)).astype(np.float64) / 8.0
    raw = np.tile(origin, (1, 468)) + ipd[:, None] * x
    raw[~x.any(axis=1)] = 0.0
    return raw.astype(np.float32).reshape(B, 468, 3)


# ---- the pools of certified faces the CPU and the GPU tests share ---------------------------------------------------------------
# Live Tanh: the kernel rounds tanhf(z) to bf16, the model rounds the f64 tanh.  The device's tanhf against numpy's f64 tanh on these
# nets' own E4 pre-activations (3 x 16,384 values, |z| <= 1.8) measured 1.27 f32 ulps at most (1.17 / 1.27 / 1.22 for F = 1404 / 136 / 13;
# mean 0.26).  The margin is 8 x that = 10.2, rounded up to a power of two: 16 ulps, so a math library whose error doubles or quadruples
# still cannot flip a rounding.  Faces with a Tanh output closer than the margin to a bf16 tie are left out (0 - 4.3 % of a pool).
# tests/test_bf16_exact_gpu.py::test_device_tanhf_error_is_inside_the_tie_margin measures again and asserts <= margin / 8.
TANHF_MEASURED_ULPS = 1.27
LIVE_TIE_MARGIN_ULPS = 16.0
MAX_EXCLUDED_SHARE = 0.15

_pools: dict = {}


def seed_of(F: int, form: str, rounded: bool) -> int:
    return F + (7 if form == "live" else 0) + (100000 if not rounded else 0)


def pool(F: int, form: str = "saturated", rounded: bool = True, B: int = 256) -> dict:
    """make() + certify() + reference(), cached: dict(enc, heads, x = the kept faces, pose, latent, valid, bits = worst bits per stage
    over them, excluded = share of the B faces left out (certificate or tie margin), n_all = B).  Row 0 of x is the "no face" row."""
    key = (F, form, rounded, B)
    if key not in _pools:
        enc, heads, x = make(F, seed_of(F, form, rounded), form, B)
        ok, worst = certify(x, enc, heads, rounded)
        if form == "live":
            ok = ok & tanh_tie_clear(x, enc, heads, LIVE_TIE_MARGIN_ULPS)
        assert ok[0], "the all-zero face is always exact"
        pose, lat, valid = reference(x[ok], enc, heads, rounded)
        _pools[key] = {"enc": enc, "heads": heads, "x": x[ok], "pose": pose, "latent": lat, "valid": valid,
                       "bits": worst_bits(worst, ok), "excluded": 1.0 - ok.mean(), "n_all": B, "x_all": x, "kept": ok}
    return _pools[key]
