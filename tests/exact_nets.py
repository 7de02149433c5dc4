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
        _pools[key] = {"key": key, "enc": enc, "heads": heads, "x": x[ok], "pose": pose, "latent": lat, "valid": valid,
                       "bits": worst_bits(worst, ok), "excluded": 1.0 - ok.mean(), "n_all": B, "x_all": x, "kept": ok}
    return _pools[key]


# ---- networks with live lo pieces: the split-f16 modes (f16x2, f16x2s) -----------------------------------------------------------------
# The split-f16 kernels scale a stage's weights by a power of two s (largest |w s| in [128, 256), pack.cpp), split w s and the f32
# activation a into f16 pieces hi = f16(v), lo = f16(v - hi), and accumulate b s + a_hi w_hi + a_lo w_hi + a_hi w_lo in f32; a_lo w_lo
# is dropped.  The nets above have +-1 weights and small integer activations: every lo piece is zero.  Here a weight of
# +-(1 + 2^-11) becomes hi = 128, lo = 2^-4 after scaling, an activation that needs more than 11 bits has a non-zero lo, and the model
# below sums the three products per piece, so a kernel that drops, swaps or misplaces a lo piece gets different bits.
#
# All three kinds on one accumulator fit 20 bits only where the activation that meets w_lo has a SHORT hi: a_hi w_lo has the place value
# lsb(a_hi) 2^-4 and a_hi w_hi reaches a_hi 128.  The input layer can be built that way: x = +-(1 + 2^-11) splits into hi = +-1,
# lo = +-2^-11, so pool "E0wx" (x in {0, +-1, +-(1 + 2^-11)} under a bumped E0) has all three kinds on > 89 % of E0's accumulators inside
# 17.7 bits, and there a_lo w_lo is non-zero and dropped: the split model's bits differ from the plain f64 forward's.  A hidden stage's
# inputs are sums and cannot be kept short: with E0 and E1 both bumped, E0's outputs such as 1 + 3 2^-11 have an 11-bit hi
# and E1 needs 26.5 bits (measured, F = 1404; certify_split refuses every face but the all-zero one).  So behind layer 0 a net is
# "bumped" (two weights per row times 1 + 2^-11) at a stage whose inputs are small integers (a_lo == 0 there), and the 11 fractional
# bits its outputs then carry make a_lo live in every stage behind it, where the weights are +-1: w_lo is covered at the bumped stage,
# a_lo behind it, and the pools TOGETHER put both under every stage kind (except a_lo under E5, whose input is the saturated Tanh:
# -1, 0 or 1).  A saturated Tanh resets the width, so a net carries one bump in the trunk and one behind it.
BUMP = np.float32(1.0 + 2.0 ** -11)
SPLIT_GAIN = SATURATING_GAIN * 2.0 ** 11     # E4 pre-activations carry 11 fractional bits and are still 0 or >= 64 in magnitude
F16_MAX = 65504.0                            # the largest f16; f32 values from 65520 on convert to inf
F16_OVER = 65520.0
_THIN = {"E1": 4, "E2": 4, "E3": 4, "E4": 4, "H1": 4, "H2": 4, "H3": 4, "H4": 4}
# name -> bumped stages, the kind of x, non-zero weights per row
SPLIT_POOLS = {
    "E0w": dict(bump=("E0", "E5"), x="int", nnz=dict(_THIN, E0=16)),
    "E0wx": dict(bump=("E0",), x="short", nnz=dict(_THIN, E0=16)),
    "E0x": dict(bump=("H4",), x="frac", nnz=dict(_THIN, E0=16, H1=8, H2=4, H3=2)),
    "E1": dict(bump=("E1", "H0"), x="int", nnz=dict(_THIN, E0=16, E1=8, E3=2, E4=2)),
    "E2": dict(bump=("E2", "H1"), x="int", nnz=dict(_THIN, E0=16, E1=16, E2=8, E3=2, E4=2, H1=8)),
    "E3": dict(bump=("E3", "H2"), x="int", nnz=dict(_THIN, E0=16, E1=8, E2=8, E3=4, E4=2, H1=8, H2=4, H4=2)),
    "E4": dict(bump=("E4", "H3"), x="int", nnz=dict(_THIN, E0=16, E1=8, E2=4, E3=4, E4=4, H1=8, H2=4, H3=4)),
}
SPLIT_KINDS = ("hi_hi", "lo_hi", "hi_lo")    # (activation piece, weight piece)


def _bump_rows(g, w):
    """Two of each row's non-zero weights times 1 + 2^-11 (exact in f32: +-1 times a power of two before)."""
    score = np.where(w != 0, g.random(w.shape), 2.0)
    pick = np.argsort(score, axis=1)[:, :2]
    m = np.zeros(w.shape, bool)
    np.put_along_axis(m, pick, True, axis=1)
    return np.where(m & (w != 0), w * BUMP, w).astype(np.float32)


def make_split(F: int, seed: int, bump=("E0",), x_kind: str = "int", nnz: dict | None = None, B: int = 256, zero_trunk_bias: bool = False):
    """Saturated-Tanh net as make(), with the stages in `bump` bumped and the E4 gain 2^17.  x_kind "int": x in {-1, 0, 1};
    "frac": x = k + j 2^-11, k in {-1, 0, 1}, j in -3..3; "short": x in {0, +-1, +-(1 + 2^-11)}, every hi piece -1, 0 or 1.  zero_trunk_bias: E0..E3 without
    bias, which makes the ReLU trunk positively homogeneous (the rescue pool scales rows by powers of two)."""
    nz = dict(DEFAULT_NNZ)
    nz.update(nnz or {})
    g = synth.rng(seed, _STREAM + 2)
    x = g.integers(-1, 2, size=(B, F)).astype(np.float64)
    if x_kind == "frac":
        x = x + g.integers(-3, 4, size=(B, F)) * 2.0 ** -11
    elif x_kind == "short":
        x = x + np.sign(x) * g.integers(0, 2, size=(B, F)) * 2.0 ** -11
        if F >= 792:
            x[:, 789:792] = np.trunc(x[:, 789:792])     # column 99 below is column 789 + 1: -(1 + 2^-11) + 1 would be a short -2^-11
    if F >= 6:
        x[:, 3:6] = 0.0
    if F >= 792:
        x[:, 99:102] = x[:, 789:792]
        x[:, 99] = x[:, 789] + 1.0
    x[0] = 0.0
    x = x.astype(np.float32)
    enc, fan_in = {}, F
    for i, width in enumerate(ENCODER_OUT):
        w = _pm1(g, width, fan_in, nz[f"E{i}"])
        if i == 0:      # every neuron reads the LAST real column, next to the padded K tail -- with a lo piece when E0 is bumped
            w[:, F - 1] = (2 * g.integers(0, 2, size=width) - 1).astype(np.float32)
        enc[f"encoder.{2 * i}.weight"] = _bump_rows(g, w) if f"E{i}" in bump else w
        if i == 0 and "E0" in bump:
            enc["encoder.0.weight"][:, F - 1] = np.sign(w[:, F - 1]) * BUMP
        enc[f"encoder.{2 * i}.bias"] = np.zeros(width, np.float32) if (zero_trunk_bias and i < 4) else _ibias(g, width)
        fan_in = width
    heads = {}
    for n in EH.HEAD_NAMES:
        heads[n] = {}
        for i, (n_out, n_in) in enumerate(HEAD_SHAPES):
            w = _pm1(g, n_out, n_in, nz[f"H{i}"])
            heads[n][f"model.{2 * i}.weight"] = _bump_rows(g, w) if f"H{i}" in bump else w
            heads[n][f"model.{2 * i}.bias"] = _ibias(g, n_out)
    enc["encoder.8.weight"] = enc["encoder.8.weight"] * np.float32(SPLIT_GAIN)
    enc["encoder.8.bias"] = np.zeros(64, np.float32)
    return enc, heads, x


def stage_scale(*ws) -> float:
    """pack.cpp's power-of-two scale of a stage: the largest |w| of its matrices (a head stage: all three heads) times s in [128, 256)."""
    mx = max(float(np.abs(w).max()) for w in ws)
    if mx == 0.0:
        return 1.0
    _, ex = np.frexp(mx)
    return float(2.0 ** int(np.clip(8 - ex, -100, 100)))


def f16_split(v):
    """f32 values -> (hi, lo) as f64: hi = f16(v), lo = f16(v - hi), the difference taken in f32 (== blob_emulator._split)."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _split_walk(x, enc_sd, head_sds, whole: bool = False):
    """The 21 stages of the split-f16 modes -> list of dict(name, a = the f32 input, a_hi, a_lo, w_hi, w_lo, bs = b s, s,
    z = the f32 pre-activation, h = the f32 image the next stage reads), every array f64-typed.  whole: the rescued face's arithmetic
    instead -- the whole f32 activation times (w_hi + w_lo), nothing dropped."""
    p = EH.Params(enc_sd, head_sds)
    out = []

    def stage(name, a32, w, b, s, act):
        a = a32.astype(np.float64)
        a_hi, a_lo = f16_split(a32)
        w_hi, w_lo = f16_split(w * np.float32(s))
        bs = b.astype(np.float64) * s
        with np.errstate(over="ignore", invalid="ignore"):
            if whole:
                z = (bs + a @ (w_hi + w_lo).T) / s
            else:
                z = (bs + a_hi @ w_hi.T + a_lo @ w_hi.T + a_hi @ w_lo.T) / s
            z32 = z.astype(np.float32)
            h = np.maximum(z32, 0) if act == "relu" else (np.tanh(z32.astype(np.float64)).astype(np.float32) if act == "tanh" else z32)
        out.append({"name": name, "a": a, "a_hi": a_hi, "a_lo": a_lo, "w_hi": w_hi, "w_lo": w_lo, "ws": w.astype(np.float64) * s, "bs": bs,
                    "s": s, "z64": z, "z": z32.astype(np.float64), "h": h})
        return h

    h = np.asarray(x, np.float32)
    for li, (w, b) in enumerate(p.enc):
        h = stage(f"E{li}", h, w, b, stage_scale(w), "relu" if li < 4 else ("tanh" if li == 4 else "none"))
    lat = h
    scales = [stage_scale(*(p.heads[n][li][0] for n in EH.HEAD_NAMES)) for li in range(5)]
    for gi, n in enumerate(EH.HEAD_NAMES):
        h = lat[:, 3 * gi:3 * gi + 3]
        for li, (w, b) in enumerate(p.heads[n]):
            h = stage(f"{n}.H{li}", h, w, b, scales[li], "relu" if li < 4 else "none")
    return out


def _answer(stages):
    lat = stages[5]["z"].astype(np.float32)
    pose = np.concatenate([stages[10]["z"], stages[15]["z"], stages[20]["z"]], axis=1).astype(np.float32)
    return pose, lat


def rescued_faces(stages):
    """(over, inside) bool[B] of a split walk: some f32 image value a kernel splits converts to an infinite f16 (|a| >= 65,520: the
    face's pose comes out non-finite and the face is evaluated again in f32) / every such value is below 65,504."""
    amax = np.max([np.abs(st["a"]).max(axis=1) for st in stages], axis=0)      # NaN behind an overflow: neither comparison holds
    return ~(amax < F16_OVER), amax < F16_MAX


def reference_split(x, enc_sd, head_sds, return_stages: bool = False):
    """The split-f16 modes' answer on the state dicts (dense numpy, no blob) -> (pose f32[B,3], latent f32[B,9], valid bool[B],
    rescued bool[B]); a rescued face is the whole-f32-activation model's.  return_stages: + the split walk's 21 stage images."""
    stages = _split_walk(x, enc_sd, head_sds)
    pose, lat = _answer(stages)
    over, _ = rescued_faces(stages)
    if over.any():
        pose_w, lat_w = _answer(_split_walk(np.asarray(x)[over], enc_sd, head_sds, whole=True))
        pose[over], lat[over] = pose_w, lat_w
    res = (pose, lat, (np.asarray(x) != 0).any(axis=1), over)
    return res + (stages,) if return_stages else res


def certify_split(x, enc_sd, head_sds, bits: int = 20):
    """-> (ok bool[B], worst {stage: bits needed per face}, cover {stage: {kind: bool[B, N]}}, stages).  ok[f]: at every neuron of
    every stage the scaled bias and the three kinds of products TOGETHER are multiples of a quantum q with sum|addends| + |b s| <
    2^bits q -- the same answer from one accumulator, from split accumulators and from layer 1's mid-K merge --, every value the
    kernels split does so exactly (f32(hi) + f32(lo) == a) and stays below 65,504, every pre-activation is an f32, and every scaled
    weight is hi + lo.  cover: which accumulators receive a non-zero product of each kind."""
    stages = _split_walk(x, enc_sd, head_sds)
    ok = np.ones(len(x), bool)
    worst, cover = {}, {}
    for st in stages:
        pairs = ((st["a_hi"], st["w_hi"]), (st["a_lo"], st["w_hi"]), (st["a_hi"], st["w_lo"]))
        assert np.array_equal(st["w_hi"] + st["w_lo"], st["ws"]), f"{st['name']}: a scaled weight is not hi + lo"
        s = np.abs(st["bs"])[None, :] + sum(np.abs(a) @ np.abs(w).T for a, w in pairs)
        lq = np.min([_row_quantum_exp(a, w, st["bs"]) for a, w in pairs], axis=0)
        lq0 = np.where(np.isfinite(lq), lq, 0.0)
        ok &= (s < 2.0 ** bits * 2.0 ** lq0).all(axis=1)
        ok &= (st["a_hi"] + st["a_lo"] == st["a"]).all(axis=1) & (np.abs(st["a"]) < F16_MAX).all(axis=1)
        ok &= (st["z"] == st["z64"]).all(axis=1)
        worst[st["name"]] = np.where(s > 0, np.log2(np.where(s > 0, s, 1.0)) - lq0, -np.inf).max(axis=1)
        cover[st["name"]] = {k: ((a != 0).astype(np.float32) @ (w != 0).astype(np.float32).T) > 0 for k, (a, w) in zip(SPLIT_KINDS, pairs)}
    return ok, worst, cover, stages


def coverage(cover: dict, faces) -> dict:
    """{layer: {kind: share of the (face, neuron) accumulators of `faces` that receive a non-zero product of the kind}}, heads merged."""
    cnt = {}
    for name, kinds in cover.items():
        key = name.split(".")[-1]
        for k, m in kinds.items():
            c = cnt.setdefault(key, {}).setdefault(k, [0, 0])
            c[0] += int(m[faces].sum())
            c[1] += int(m[faces].size)
    return {key: {k: c[0] / max(c[1], 1) for k, c in kinds.items()} for key, kinds in cnt.items()}


def lo_lo_is_zero(stages, faces) -> bool:
    """No stage of these faces has a non-zero a_lo w_lo product: the split model drops nothing and equals the plain f64 forward."""
    return not any((((st["a_lo"][faces] != 0).astype(np.float32) @ (st["w_lo"] != 0).astype(np.float32).T) > 0).any() for st in stages)


def split_seed(name: str, F: int) -> int:
    return 200000 + 1000 * sorted(SPLIT_POOLS).index(name) + F


def split_pool(name: str, F: int = 1404, B: int = 256) -> dict:
    """make_split() + certify_split() + reference_split(), cached, in pool()'s form; + cover = coverage() over the kept faces."""
    key = ("split", name, F, B)
    if key not in _pools:
        cfg = SPLIT_POOLS[name]
        enc, heads, x = make_split(F, split_seed(name, F), cfg["bump"], cfg["x"], cfg["nnz"], B)
        ok, worst, cover, _ = certify_split(x, enc, heads)
        assert ok[0], "the all-zero face is always exact"
        pose, lat, valid, over = reference_split(x[ok], enc, heads)
        assert not over.any()
        _pools[key] = {"key": key, "enc": enc, "heads": heads, "x": x[ok], "pose": pose, "latent": lat, "valid": valid, "bits": worst_bits(worst, ok),
                       "excluded": 1.0 - ok.mean(), "n_all": B, "x_all": x, "kept": ok, "cover": coverage(cover, ok), "bump": cfg["bump"]}
    return _pools[key]


RESCUE_KINDS = ("plain", "inside", "hidden", "input")


def rescue_pool(F: int = 1404, B: int = 96) -> dict:
    """Faces around f16's range, in pool()'s form + kind int8[n] (index into RESCUE_KINDS), base int[n] (the "plain" row a row is a
    power-of-two multiple of) and rescued bool[n].  The net is bumped at E0 only and its trunk biases E0..E3 are zero, so the ReLU trunk
    is positively homogeneous: row r times 2^k has row r's E4 pre-activations times 2^k, the saturated Tanh gives the same -1, 0, 1,
    and latent and pose are row r's, bit for bit.  Per plain row r with the largest trunk image value m:
      inside  k = the largest with m 2^k < 65,504: every f16 piece finite, not rescued;
      hidden  k + 1: x still fits (|x| 2^(k+1) <= 32,768) but a hidden activation converts to inf: rescued;
      input   k = 16: x itself converts to inf: rescued.
    No stage of this net has both a_lo and w_lo, so the split model equals the plain f64 forward on it and a rescued row's answer (whole
    f32 activations) IS the unscaled row's.  Rescued rows are certified by certify(rounded=False), the others by certify_split()."""
    key = ("rescue", F, B)
    if key in _pools:
        return _pools[key]
    enc, heads, x = make_split(F, 300000 + F, ("E0",), "int", SPLIT_POOLS["E0w"]["nnz"], B, zero_trunk_bias=True)
    ok, _, _, stages = certify_split(x, enc, heads)
    m = np.max([np.abs(st["a"]).max(axis=1) for st in stages[:5]], axis=0)
    ok &= m > 0
    ok[0] = True
    rows = np.flatnonzero(ok)
    live = rows[1:]
    k_in = np.floor(np.log2(65503.0 / m[live])).astype(int)
    xs = [x[rows]] + [x[live] * (2.0 ** k)[:, None].astype(np.float32) for k in (k_in, k_in + 1, np.full(len(live), 16))]
    kind = np.concatenate([np.full(len(v), i, np.int8) for i, v in enumerate(xs)])
    base = np.concatenate([np.arange(len(rows))] + [np.arange(1, len(rows))] * 3)
    xp = np.concatenate(xs)
    pose, lat, valid, over, st_all = reference_split(xp, enc, heads, return_stages=True)
    _, inside = rescued_faces(st_all)
    ok_split, worst, _, _ = certify_split(np.where(over[:, None], np.float32(0), xp), enc, heads)
    ok_whole, _ = certify(xp, enc, heads, rounded=False)
    keep = np.where(over, ok_whole, ok_split & inside) & (over == (kind >= 2))
    keep &= keep[base]                                            # a multiple stays only with its plain row
    assert lo_lo_is_zero(st_all, ~over)
    idx = np.cumsum(keep) - 1                                     # old row -> new row
    _pools[key] = {"key": key, "enc": enc, "heads": heads, "x": xp[keep], "pose": pose[keep], "latent": lat[keep], "valid": valid[keep],
                   "rescued": over[keep], "kind": kind[keep], "base": idx[base[keep]], "bits": worst_bits(worst, keep & ~over),
                   "excluded": 1.0 - keep.mean(), "n_all": len(xp)}
    return _pools[key]
