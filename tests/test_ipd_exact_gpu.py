"""Every copy of the IPD landmark normalisation bit for bit on inputs built to be hard (tests/ipd_cases.py; its host side:
tests/test_ipd_exact_host.py).

K1 (normalize_ipd.hip) is compared element by element with ipd_cases.reference(): the rational reference on the engineered elements --
f64 quotients within 2 f64 ulps of an f32 rounding midpoint, where one wrong f64 ulp anywhere in the chain flips the f32 result --, on
the sampled elements and on the zero / sign / subnormal faces, the C oracle elsewhere.

The fused f32 prologue (encoder_heads.hip) is pinned directly: ipd_cases.readout_net(60) hands the kernel's own x to the pose with every
sum of one non-zero term and the Tanh where it is the identity, so the pose must be the C oracle's f32 chain on the rational reference's
features, bit for bit -- which is x itself.

Every other copy (the f16x2 kernel's hand-scheduled chain, the eight-wave f16x2s and bf16 kernels, the layer-per-launch form, the
streamed tail's trunk, the in-kernel rescue) is compared with its own K2 on K1's output, on every family; the live-Tanh read-out net
(shift 0) on the probe families makes x visible, and each form prints on how many faces a one-ulp nudge of the engineered x moves its
pose bits -- the share of faces on which the equality can see one ulp.  A form that sees none on the probe families fails as powerless.
Measured on an MI355X, faces of 465 whose pose bits move (families A / B / C / D / P / PF):
    f32 fused                        465 / 462 /  13 / 185 / 462 / 463
    f16x2 fused, layer per launch    389 / 305 /  12 / 140 / 284 / 463      (PF: every face rescued, 463 of them move)
    f16x2s fused eight-wave, layer per launch, streamed tail
                                     374 / 309 /  13 / 135 / 284 / 463      (PF: every face rescued, 463 of them move)
    bf16 fused                         0 /   0 /   0 /   0 / 125 / 111
(C and a part of D: features of ~1e6 and beyond saturate the random network's Tanh; bf16 keeps 8 bits of x and sees the probe faces whose
float32 neighbours straddle a bf16 tie.)"""
import numpy as np
import pytest
import torch

import ipd_cases as IC
from nlml_hpe_amd import _lib, ops, synth, weights
from oracle import c_oracle as CO
from oracle import encoder_heads as EH
from test_gpu_parity import _report

pytestmark = pytest.mark.gpu

FAMILIES = IC.DENSE + IC.PROBES
# encoder_heads.hip: TILE = 32 * NFB; launch_encoder_heads_f32 takes NFB = 2 (64 faces, a second row per staging thread) when that
# saves a round of tiles over the 256 CUs -- from 8,193 faces on -- and NFB = 1 (32 faces) below
F32_TILE = 64
F32_WIDE_MIN = 8193


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return IC.f32_bits(a)


_cat: dict = {}


def _all():
    """Every family concatenated -> (raw, features, valid, family name per face)."""
    if not _cat:
        refs = [IC.reference(n) for n in FAMILIES]
        _cat["v"] = (np.concatenate([IC.family(n)["raw"] for n in FAMILIES]), np.concatenate([r[0] for r in refs]),
                     np.concatenate([r[1] for r in refs]), np.concatenate([[n] * len(r[0]) for n, r in zip(FAMILIES, refs)]))
    return _cat["v"]


def _case(name):
    if name == "all":
        return _all()[:3]
    return (IC.family(name)["raw"],) + IC.reference(name)


def _check_k1(got, valid, want, want_valid, tag):
    bad = np.argwhere(_bits(got) != _bits(want))
    if len(bad):
        f, c = bad[0]
        raise AssertionError(f"{tag}: {len(bad)} elements on {len(set(bad[:, 0].tolist()))} faces differ, first face {f} column {c} (landmark "
                             f"{c // 3}, lane {(c // 4) % 64}): got {_bits(got)[f, c]:#010x} want {_bits(want)[f, c]:#010x}")
    assert np.array_equal(valid.cpu().numpy(), want_valid), tag


# ---- K1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES + ("all",))
def test_k1_bits_and_valid(name, device):
    """Each family and all of them in one batch (2,803 faces); the slices [:1], [:3], [:5] and [1:] (a block takes 4 faces, a wave one);
    the registered op; normalize=False hands the input bits through (family E's -0.0 included)."""
    raw, want, want_valid = _case(name)
    rt = _dev(raw, device)
    out, valid = ops.normalize_ipd(rt, True, return_valid=True)
    _check_k1(out, valid, want, want_valid, f"family {name}")
    for sl in (slice(0, 1), slice(0, 3), slice(0, 5), slice(1, None)):
        o, v = ops.normalize_ipd(rt[sl], True, return_valid=True)
        _check_k1(o, v, want[sl], want_valid[sl], f"family {name}, faces {sl}")
    assert np.array_equal(_bits(torch.ops.nlml_hpe.normalize_ipd(rt, True)), _bits(want))
    o, v = ops.normalize_ipd(rt, False, return_valid=True)
    flat = raw.reshape(len(raw), -1)
    assert np.array_equal(_bits(o), _bits(flat)) and np.array_equal(_bits(torch.ops.nlml_hpe.normalize_ipd(rt, False)), _bits(flat))
    assert np.array_equal(v.cpu().numpy(), ((_bits(flat) & 0x7FFFFFFF) != 0).any(axis=1))


# ---- the fused f32 prologue, pinned directly ---------------------------------------------------------------------------------------------
_nets: dict = {}


def _net(kind, head_sds=None):
    """kind: "exact" (read-out, Tanh the identity), "tanh" (read-out, live Tanh), "synth" (a dense random encoder + the shipped heads)."""
    if kind not in _nets:
        if kind == "synth":
            _nets[kind] = (synth.encoder_state_dict(1404, seed=0), head_sds)
        else:
            _nets[kind] = IC.readout_net(IC.READOUT_EXACT_SHIFT if kind == "exact" else 0)
    return _nets[kind]


_blobs: dict = {}


def _blob(kind, mode, device, head_sds=None):
    if (kind, mode) not in _blobs:
        _blobs[kind, mode] = _dev(weights.pack_blob(*_net(kind, head_sds), _lib.mode_from_name(mode)), device)
    return _blobs[kind, mode]


@pytest.mark.parametrize("name", IC.PROBES)
def test_fused_f32_prologue_against_the_rational_reference(name, device):
    """ops.landmarks_to_pose with the f32 blob of the exact read-out net == the C oracle's f32 chain (order 2) on the rational
    reference's features, bit for bit, and that is the engineered x itself; whole batch, batches that end in partial tiles, and both tile forms."""
    fam = IC.family(name)
    feats, want_valid = IC.reference(name)
    want = CO.encoder_heads(feats, EH.Params(*_net("exact")), order=2)
    f, c = fam["eng_face"], fam["eng_col"]
    assert np.array_equal(_bits(want[f, c % 3]), _bits(feats[f, c]))
    blob = _blob("exact", "f32", device)
    rt = _dev(fam["raw"], device)
    T = F32_TILE
    for sl in (slice(None), slice(0, 1), slice(0, T // 2 - 1), slice(0, T // 2 + 1), slice(0, T - 1), slice(0, T + 1), slice(3, 3 * T + 2 + 3),
               slice(T // 2 + 5, None)):
        pose, valid = ops.landmarks_to_pose(rt[sl], blob, True, return_valid=True)
        bad = np.flatnonzero((_bits(pose) != _bits(want[sl])).any(axis=1))
        assert not len(bad), (f"family {name}, faces {sl}: {len(bad)} faces differ, first {bad[0]} (landmark {IC.ENG[(bad[0] + (sl.start or 0)) % 465]}): got "
                              f"{pose[bad[0]].tolist()} want {want[sl][bad[0]].tolist()}")
        assert np.array_equal(valid.cpu().numpy(), want_valid[sl])
    assert np.array_equal(_bits(ops.encoder_heads_fwd(_dev(feats, device), blob, 1404)), _bits(want))
    # the 64-face form: the family 18 times over (8,370 faces: 130 tiles and 50 faces), and 8,193 faces (one face in the last tile)
    reps = -(-F32_WIDE_MIN // len(want))
    wide, wide_want = rt.repeat(reps, 1, 1), np.tile(want, (reps, 1))
    for n in (len(wide_want), F32_WIDE_MIN):
        pose, valid = ops.landmarks_to_pose(wide[:n], blob, True, return_valid=True)
        bad = np.flatnonzero((_bits(pose) != _bits(wide_want[:n])).any(axis=1))
        assert not len(bad), f"family {name}, {n} faces (64-face tiles): {len(bad)} faces differ, first {bad[0]} (tile row {bad[0] % 64})"
        assert valid.all()


# ---- every other copy: fused == K2(K1) ---------------------------------------------------------------------------------------------------
def _fused(raw, blob):
    return ops.landmarks_to_pose(raw, blob, True, return_valid=True)


def _small(raw, blob):
    return ops.landmarks_to_pose_small(raw, blob, True, return_valid=True)


def _streamed(raw, blob):
    return ops.landmarks_to_pose_streamed(raw, blob, True, return_valid=True)


# form -> (blob mode, the call on raw landmarks, rescued faces expected)
FORMS = {
    "f32 fused": ("f32", _fused, False),
    "f16x2 fused": ("f16x2", _fused, True),
    "f16x2 layer per launch": ("f16x2", _small, True),
    "f16x2s fused eight-wave": ("f16x2s", _fused, True),
    "f16x2s layer per launch": ("f16x2s", _small, True),
    "f16x2s streamed tail": ("f16x2s", _streamed, True),
    "bf16 fused": ("bf16", _fused, False),
}


def _same_pose(a, b):
    """Bit-identical, or NaN in the same places (a face whose features overflow to +-inf has a NaN pose; NaN payloads are not pinned)."""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return ((IC.f32_bits(a) == IC.f32_bits(b)) | (np.isnan(a) & np.isnan(b))).all(axis=1)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_fused_equals_k2_of_k1(form, head_sds, device):
    mode, call, rescues = FORMS[form]
    seen = {}
    for name in FAMILIES:
        fam = IC.family(name)
        kind = "tanh" if name in IC.PROBES else "synth"
        blob = _blob(kind, mode, device, head_sds)
        rt = _dev(fam["raw"], device)
        feats, v1 = ops.normalize_ipd(rt, True, return_valid=True)
        pose2 = ops.encoder_heads_fwd(feats, blob, 1404)
        pose, valid = call(rt, blob)
        ok = _same_pose(pose, pose2)
        assert ok.all(), f"{form}, family {name}: {int((~ok).sum())} faces differ from K2(K1), first {int(np.flatnonzero(~ok)[0])}"
        assert torch.equal(valid, v1), (form, name)
        if rescues and name in ("PF", "D"):
            x = IC.reference(name)[0]
            with np.errstate(invalid="ignore"):
                over = ~(np.abs(x).max(axis=1) < IC.F16_OVER)          # the kernels' rule: an f16 piece of x would be infinite
            assert over.all() if name == "PF" else (over[fam["kind"] == 2].all() and over[fam["kind"] == 3].all()), (form, name)
            seen[f"rescued_{name}"] = int(over.sum())
        if len(fam["eng_face"]):
            near = _dev(IC.nudged(feats.cpu().numpy(), fam), device)
            moved = ~_same_pose(ops.encoder_heads_fwd(near, blob, 1404), pose2)
            seen[f"moved_{name}"] = int(moved.sum())
            if rescues and name == "PF":
                seen["rescued_PF_moved"] = int(moved[over].sum())
    print(f"{form}: faces whose pose bits move under a one-ulp nudge of the engineered x: "
          + ", ".join(f"{k[6:]} {v}/{IC.N_FACES}" for k, v in seen.items() if k.startswith("moved_"))
          + "".join(f"; {k} {v}" for k, v in seen.items() if not k.startswith("moved_")))
    _report(f"ipd_exact_{form.replace(' ', '_')}", **seen)
    assert seen["moved_P"] + seen["moved_PF"] > 0, f"{form}: powerless -- no probe face shows a one-ulp difference of x"


# ---- non-finite landmarks ----------------------------------------------------------------------------------------------------------------
def test_non_finite_landmarks_agree_across_the_copies(head_sds, device):
    """An infinite landmark or an infinite IPD: the reciprocal chain q = n y, r = fma(-q, ipd, n), q' = fma(r, y, q) returns NaN where
    IEEE division (numpy, the C oracle) returns +-inf (inf / ipd: r = inf - inf) or 0 (n / inf: y = 0, r = 0 x inf), so K1's row differs
    from numpy's THERE, by design: the face is unusable either way, its pose is NaN and it does not leak into its neighbours
    (test_nan_and_inf_stay_in_their_face).  Pinned here: which elements K1 makes NaN, that every fused form gives the same valid and the
    same NaN-ness of the pose as its K2 on K1's row, and that the other faces keep their bits."""
    raw = synth.raw_landmarks(131, seed=31)
    clean = raw.copy()
    raw[5, 200, 1] = np.inf              # one infinite landmark: NaN there (numpy: +inf), the rest of the face finite
    raw[40, IC.EYE_L, 0] = np.inf        # infinite IPD: the whole row NaN (numpy: zeros, and NaN at landmark 33's x)
    raw[64, IC.NOSE, 2] = -np.inf        # infinite landmark 1: every z NaN (numpy: +inf, NaN at landmark 1's own z)
    raw[95, 7, 0] = np.nan
    raw[130, IC.EYE_R, 1] = -np.inf      # last face, a partial tile
    rows = [5, 40, 64, 95, 130]
    keep = np.ones(131, bool)
    keep[rows] = False
    rt, ct = _dev(raw, device), _dev(clean, device)
    feats, v1 = ops.normalize_ipd(rt, True, return_valid=True)
    k1 = feats.cpu().numpy()
    nan = np.isnan(k1)
    assert not nan[keep].any() and np.array_equal(_bits(k1[keep]), _bits(ops.normalize_ipd(ct, True))[keep])
    assert nan[5].sum() == 1 and nan[5, 601] and nan[40].all() and nan[130].all() and nan[95].sum() == 1 and nan[95, 21]
    assert np.array_equal(nan[64], np.arange(1404) % 3 == 2)
    assert v1.all()
    for form in sorted(FORMS):
        mode, call, _ = FORMS[form]
        blob = _blob("synth", mode, device, head_sds)
        pose, valid = call(rt, blob)
        pose2 = ops.encoder_heads_fwd(feats, blob, 1404)
        want, _ = call(ct, blob)
        assert torch.equal(valid, v1), form
        assert torch.equal(torch.isnan(pose).any(dim=1), torch.isnan(pose2).any(dim=1)), form
        assert torch.isnan(pose[rows]).any(dim=1).all(), (form, pose[rows])
        k = _dev(keep, device)
        assert torch.equal(pose[k].view(torch.int32), want[k].view(torch.int32)) and torch.equal(pose[k].view(torch.int32), pose2[k].view(torch.int32)), form
