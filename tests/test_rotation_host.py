"""Landmark rotation without a GPU: the host restatement of the kernel's operation order (nlml_compose_rotation_tensor_host,
nlml_rotate_landmarks_host, csrc/rotate_ref.h) against the reference's recorded results (FX12), the matrix tables, the copy rule, the
signed zeros, and the checks the device entry points make before any HIP call.

WHAT THE DATA TELLS APART.  The contract is, per output, acc = +0.0; acc = fma(a0, m0, acc); fma(a1, m1, acc); fma(a2, m2, acc), three
stages.  Two plausible wrong chains are evaluated here in Python on FX12's own inputs (the f64 results of both rotation types on the
eight poses, identity 1's 468 points and the 64-row sign table: 25,536 entries), with an exactly rounded fma from rationals:
    no fma at all       ((0.0 + a0*m0) + a1*m1) + a2*m2, every product rounded        3,889 entries differ
    bare first product  a0*m0, then fma(a1, m1, .), fma(a2, m2, .)                         7 entries differ, every one a zero's sign
while the contract's chain, evaluated the same way, differs in none.  A kernel built with either wrong chain cannot pass.
"""
import itertools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from nlml_hpe_amd import CreateTensor as CT
from nlml_hpe_amd import IntrinsicRotation as IR
from nlml_hpe_amd import _lib, ops, synth  # noqa: F401  (ops registers torch.ops.nlml_hpe.*)

BADARG = -1
FAKE = 4096       # an aligned non-null "device" pointer: every call below is refused before it could be used
REF = "/root/reference"
FX12 = "fx12_rotation_tensor.npz"
TYPES = ("intrinsic", "extrinsic")
NEG0_32, NEG0_64 = np.uint32(0x80000000), np.uint64(0x8000000000000000)


def load_fx12(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, FX12)))
    g["base"] = g["base_bits"].view(np.float32)
    g["signs"] = g["signs_bits"].view(np.float32)
    return g


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def grid_tables(yaw, pitch, roll, order="intrinsic"):
    """The per-axis matrix tables of a grid, as CreateTensor.Compose_Tensor builds them; transposed for the extrinsic order."""
    t = [IR.rotation_matrices("y", yaw), IR.rotation_matrices("x", pitch), IR.rotation_matrices("z", roll)]
    return t if order == "intrinsic" else [np.ascontiguousarray(m.transpose(0, 2, 1)) for m in t]


def host_grid(base, tables, order="intrinsic", zero=(-1, -1, -1), want64=True):
    """nlml_compose_rotation_tensor_host -> (out f32[I,ny,np,nr,1404], out64 f64 or None)."""
    base = np.ascontiguousarray(base, np.float32)
    ry, rp, rr = (np.ascontiguousarray(t, np.float64) for t in tables)
    shape = (base.shape[0], ry.shape[0], rp.shape[0], rr.shape[0], 1404)
    out = np.full(shape, 7.0, np.float32)
    out64 = np.full(shape, 7.0, np.float64) if want64 else None
    rc = _lib.lib().nlml_compose_rotation_tensor_host(base.ctypes.data, shape[0], ry.ctypes.data, shape[1], rp.ctypes.data, shape[2],
                                                      rr.ctypes.data, shape[3], _lib.rot_order_from_name(order), *zero, out.ctypes.data,
                                                      out64.ctypes.data if want64 else None)
    assert rc == 0, _lib.lib().nlml_last_error()
    return out, out64


def host_faces(lm, rot):
    """nlml_rotate_landmarks_host -> (out f32[B,468,3], out64 f64[B,468,3])."""
    lm, rot = np.ascontiguousarray(lm, np.float32), np.ascontiguousarray(rot, np.float64)
    B = lm.shape[0]
    assert lm.shape == (B, 468, 3) and rot.shape == (B, 3, 3, 3)
    out, out64 = np.full((B, 468, 3), 7.0, np.float32), np.full((B, 468, 3), 7.0, np.float64)
    rc = _lib.lib().nlml_rotate_landmarks_host(lm.ctypes.data, rot.ctypes.data, out.ctypes.data, out64.ctypes.data, B)
    assert rc == 0, _lib.lib().nlml_last_error()
    return out, out64


def sign_block(g):
    """Identity 1 with the 64-row sign table in its first rows: the kernels take [468,3] blocks only."""
    lm = g["base"][1].copy()
    lm[:64] = g["signs"]
    return lm


def special_faces(n, seed):
    """n faces: U(-2, 2), pixel scale and 1e-3 scale by turns, with signed zeros sprinkled in."""
    u = synth.rng(seed, 0).random((n, 468, 3)) * 4.0 - 2.0
    k = np.arange(n)[:, None, None] % 3
    lm = np.where(k == 0, u, np.where(k == 1, u * 320.0, u * 1e-3)).astype(np.float32)
    lm[:, 7, 0], lm[:, 7, 2], lm[:, 11] = -0.0, 0.0, -0.0
    return lm


def random_poses(n, seed):
    """(yaw, pitch, roll) degrees f64[n,3]: ordinary poses with zeros, multiples of 90 and the all-zero pose mixed in."""
    p = synth.rng(seed, 1).uniform(-180.0, 180.0, (n, 3))
    for b in range(0, n, 5):
        p[b, b % 3] = 0.0
    for b in range(3, n, 11):
        p[b] = np.array([90.0, -180.0, 270.0])[np.arange(3) - b % 3]
    if n > 2:
        p[2] = 0.0
    return p


def nonfinite_faces():
    lm = special_faces(3, seed=9)
    lm[0, 17] = np.nan
    lm[0, 9], lm[0, 10] = 3e38, -3e38        # finite in f64 at every pose; their sums overflow the f32 rounding to +-Inf
    lm[1, 400, 0] = np.inf                   # Inf times a matrix's zero entries: NaN
    lm[2, 5, 1] = -np.inf
    lm[2, 6, 2] = np.nan
    return lm


def numpy_faces(lm, rot):
    """apply_rotations' own expression per face: landmarks @ M0 @ M1 @ M2 on the f32 block, numpy promoting it to f64."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([lm[b] @ rot[b, 0] @ rot[b, 1] @ rot[b, 2] for b in range(lm.shape[0])])


def same_nonfinite(a, b):
    """Which outputs are NaN, which +Inf and which -Inf; finite outputs bit for bit.  NaN payloads are not compared."""
    fin = np.isfinite(a)
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) and
            np.array_equal(np.isneginf(a), np.isneginf(b)) and np.array_equal(bits(a)[fin], bits(b)[fin]))


# ---- the fixture --------------------------------------------------------------------------------------------------------------
def test_fx12_is_what_its_recipe_says(golden_dir):
    g = load_fx12(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, FX12)) < 700_000
    assert g["base"].shape == (2, 468, 3) and g["tensor_bits"].shape == (2, 3, 3, 3, 1404) and g["poses"].shape == (8, 3)
    assert g["apply_f64_bits"].shape == (2, 8, 468, 3) and g["signs_f64_bits"].shape == (2, 8, 64, 3)
    assert not g["base"][0, 1].any() and (bits(g["base"][1, 300]) == NEG0_32).all()
    assert int((bits(g["base"][1]) == NEG0_32).sum()) == 8 and int((bits(g["base"][1]) == 0).sum()) == 2
    assert len({tuple(r) for r in bits(g["signs"]).tolist()}) == 64
    for k in ("tensor_bits", "apply_f64_bits", "signs_f64_bits"):
        f = g[k].view(np.float32 if g[k].dtype == np.uint32 else np.float64)
        assert np.isfinite(f).all(), k
    # the centre cell is the base, bit for bit; no other cell is
    assert np.array_equal(g["tensor_bits"][:, 1, 1, 1], g["base_bits"].reshape(2, 1404))
    assert g["poses"][0].tolist() == [0, 0, 0] and (np.abs(g["poses"][1:4]) % 90 == 0).all()


def test_host_tensor_equals_fx12(golden_dir):
    g = load_fx12(golden_dir)
    out, out64 = host_grid(g["base"], grid_tables(g["yaw"], g["pitch"], g["roll"]), zero=(1, 1, 1))
    assert np.array_equal(bits(out), g["tensor_bits"])
    assert np.array_equal(out64.astype(np.float32).view(np.uint32), g["tensor_bits"])       # out is one rounding of out64
    out_only, none = host_grid(g["base"], grid_tables(g["yaw"], g["pitch"], g["roll"]), zero=(1, 1, 1), want64=False)
    assert none is None and np.array_equal(bits(out_only), g["tensor_bits"])


@pytest.mark.parametrize("k, rotation_type", list(enumerate(TYPES)))
def test_host_apply_rotations_equals_fx12(golden_dir, k, rotation_type):
    g = load_fx12(golden_dir)
    rot = IR.pose_matrices(g["poses"], rotation_type)
    P = len(g["poses"])
    out, out64 = host_faces(np.broadcast_to(g["base"][1], (P, 468, 3)), rot)
    assert np.array_equal(bits(out64), g["apply_f64_bits"][k])
    assert np.array_equal(bits(out), bits(g["apply_f64_bits"][k].view(np.float64).astype(np.float32)))
    # the same poses through the grid entry point: one pose per axis bin, no copy rule
    for j, (yw, pt, rl) in enumerate(g["poses"]):
        o, o64 = host_grid(g["base"][1:2], grid_tables([yw], [pt], [rl], rotation_type), order=rotation_type)
        assert np.array_equal(bits(o64.reshape(468, 3)), g["apply_f64_bits"][k, j]), (rotation_type, j)


@pytest.mark.parametrize("k, rotation_type", list(enumerate(TYPES)))
def test_all_64_sign_combinations(golden_dir, k, rotation_type):
    g = load_fx12(golden_dir)
    assert sorted({float(v) for v in g["signs"].ravel()}) == [-0.75, 0.0, 1.25] and int(np.signbit(g["signs"]).sum()) == 96
    P = len(g["poses"])
    _, out64 = host_faces(np.broadcast_to(sign_block(g), (P, 468, 3)), IR.pose_matrices(g["poses"], rotation_type))
    assert np.array_equal(bits(out64[:, :64]), g["signs_f64_bits"][k])
    assert np.array_equal(bits(out64[:, 64:]), g["apply_f64_bits"][k][:, 64:])


# ---- the matrices --------------------------------------------------------------------------------------------------------------
def test_rotation_matrix_equals_the_fixture_tables(golden_dir):
    g = load_fx12(golden_dir)
    for ax in ("x", "y", "z"):
        for nm in ("yaw", "pitch", "roll"):
            vals, want = g[f"full_{nm}"], g[f"rot_{ax}_{nm}_bits"]
            assert want.shape == (len(vals), 3, 3)
            for a, w in zip(vals, want):
                m = IR.rotation_matrix(ax, a)
                assert m.dtype == np.float64 and np.array_equal(bits(m), w), (ax, nm, a)
            assert np.array_equal(bits(IR.rotation_matrices(ax, vals)), want)
            assert np.array_equal(bits(IR._axis_matrices_vectorised(ax, vals)), want)
    assert len(g["full_yaw"]) == 11 and len(g["full_pitch"]) == 9 and len(g["full_roll"]) == 7
    # -np.sin(0) is -0.0: in Rx and Rz it lands above the diagonal, in Ry below
    for ax, at in (("x", (1, 2)), ("y", (2, 0)), ("z", (0, 1))):
        m0 = IR.rotation_matrix(ax, 0)
        assert bits(m0)[at] == NEG0_64 and int((bits(m0) == NEG0_64).sum()) == 1
    with pytest.raises(ValueError, match="Axis must be"):
        IR.rotation_matrix("w", 3)


def test_vectorised_pose_matrices_are_the_scalar_ones():
    poses = random_poses(300, seed=3)
    for rt in TYPES:
        rot = IR.pose_matrices(poses, rt)
        for b, (yw, pt, rl) in enumerate(poses):
            rx, ry, rz = IR.rotation_matrix("x", pt), IR.rotation_matrix("y", yw), IR.rotation_matrix("z", rl)
            want = np.stack([rx, ry, rz] if rt == "intrinsic" else [rz.T, ry.T, rx.T])
            assert np.array_equal(bits(rot[b]), bits(want)), (rt, b)
    with pytest.raises(ValueError, match="intrinsic"):
        IR.pose_matrices(poses, "euler")


def test_discretize_interval():
    pts, spacing = CT.discretize_interval(-50, 50, 11)
    assert pts == [-50 + i * 10.0 for i in range(11)] and spacing == 10.0
    with pytest.raises(ValueError, match="positive"):
        CT.discretize_interval(0, 1, 0)
    with pytest.raises(ValueError, match="less than"):
        CT.discretize_interval(1, 1, 3)


# ---- the copy rule -------------------------------------------------------------------------------------------------------------
def test_copy_rule_keeps_negative_zero_and_rotation_does_not(golden_dir):
    g = load_fx12(golden_dir)
    tables = grid_tables(g["yaw"], g["pitch"], g["roll"])
    copied, copied64 = host_grid(g["base"], tables, zero=(1, 1, 1))
    rotated, rotated64 = host_grid(g["base"], tables, zero=(-1, -1, -1))
    neg0 = bits(g["base"]).reshape(2, 1404) == NEG0_32
    assert neg0[1].sum() == 8
    centre, centre_rot = bits(copied[:, 1, 1, 1]), bits(rotated[:, 1, 1, 1])
    assert np.array_equal(centre, bits(g["base"]).reshape(2, 1404)) and (centre[neg0] == NEG0_32).all()
    assert (centre_rot[neg0] == 0).all()                                  # rotated by the three identity matrices: +0.0
    assert np.array_equal(centre_rot[~neg0], centre[~neg0])               # ... and nothing else changes
    assert np.array_equal(bits(copied64[:, 1, 1, 1]), bits(g["base"].reshape(2, 1404).astype(np.float64)))
    assert (bits(rotated64[:, 1, 1, 1])[neg0] == 0).all()
    # every other cell is the same with and without the rule; a zero bin on two axes only copies nothing
    other = np.ones(copied.shape[:4], bool)
    other[:, 1, 1, 1] = False
    assert np.array_equal(bits(copied)[other], bits(rotated)[other])
    assert np.array_equal(bits(host_grid(g["base"], tables, zero=(1, 1, -1))[0]), bits(rotated))
    # the rule follows the index, not the matrix: told that bin (0, 2, 1) is the zero bin, that cell is the copy
    moved, _ = host_grid(g["base"], tables, zero=(0, 2, 1))
    assert np.array_equal(bits(moved[:, 0, 2, 1]), bits(g["base"]).reshape(2, 1404))
    assert np.array_equal(bits(moved[:, 1, 1, 1]), centre_rot)


# ---- wrong chains must be told apart -------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fma on Python floats, exactly rounded (finite inputs), with IEEE's sign for an exact zero."""
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact != 0:
        return float(exact)          # Fraction -> float rounds to nearest, ties to even
    prod_negative = (np.signbit(a) != np.signbit(b))
    if a * b == 0 and c == 0:        # (+-0) + (+-0): -0 only if both are
        return -0.0 if prod_negative and np.signbit(c) else 0.0
    return 0.0                       # exact cancellation of non-zero terms


def _chain(kind, a, M):
    out = []
    for j in range(3):
        if kind == "contract":
            acc = _fma(a[2], M[2][j], _fma(a[1], M[1][j], _fma(a[0], M[0][j], 0.0)))
        elif kind == "bare first product":
            acc = _fma(a[2], M[2][j], _fma(a[1], M[1][j], a[0] * M[0][j]))
        else:                        # "no fma"
            acc = ((0.0 + a[0] * M[0][j]) + a[1] * M[1][j]) + a[2] * M[2][j]
        out.append(acc)
    return out


def _python_poses(kind, pts, rot):
    """pts f32[n,3] at the poses rot f64[P,3,3,3] through the Python chain -> u64 bits [P,n,3]."""
    res = np.zeros((rot.shape[0], pts.shape[0], 3), np.float64)
    for j, (M0, M1, M2) in enumerate(rot.tolist()):
        for i, p in enumerate(pts.astype(np.float64).tolist()):
            res[j, i] = _chain(kind, _chain(kind, _chain(kind, p, M0), M1), M2)
    return bits(res)


def test_wrong_chains_are_told_apart_by_fx12(golden_dir):
    g = load_fx12(golden_dir)
    pts = np.concatenate([g["signs"], g["base"][1]])
    differing = {"contract": 0, "no fma": 0, "bare first product": 0}
    sign_only = True
    for k, rt in enumerate(TYPES):
        want = np.concatenate([g["signs_f64_bits"][k], g["apply_f64_bits"][k]], axis=1)
        rot = IR.pose_matrices(g["poses"], rt)
        for kind in differing:
            d = _python_poses(kind, pts, rot) != want
            differing[kind] += int(d.sum())
            if kind == "bare first product":
                sign_only &= bool((want[d] & ~NEG0_64 == 0).all())
    print(f"entries of {2 * 8 * 532 * 3} that differ from the reference: {differing}")
    assert differing["contract"] == 0
    assert differing["no fma"] > 0 and differing["bare first product"] > 0
    assert sign_only                 # the bare product is wrong only in a zero's sign: the signed-zero data is what catches it


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotation_type", TYPES)
def test_nonfinite_inputs_propagate_as_in_numpy(rotation_type):
    lm = nonfinite_faces()
    rot = IR.pose_matrices([(31, 12, -7), (0, 0, 17), (90, 0, 0)], rotation_type)
    out, out64 = host_faces(lm, rot)
    want = numpy_faces(lm, rot)
    assert same_nonfinite(out64, want)
    with np.errstate(invalid="ignore", over="ignore"):
        assert same_nonfinite(out, want.astype(np.float32))
    assert np.isnan(out64[0, 17]).all() and np.isfinite(out64[0, :17]).all() and np.isfinite(out64[0, 18:]).all()
    assert not np.isfinite(out64[1, 400]).all() and np.isfinite(out64[1, :400]).all()
    assert np.isposinf(out[0, 9:11]).any() and np.isneginf(out[0, 9:11]).any() and np.isfinite(out64[0, 9:11]).all()
    # the grid entry point on the same faces: the copied cell keeps them as they are
    g_out, _ = host_grid(lm, grid_tables([0, 31], [0, 12], [0, -7], rotation_type), order=rotation_type, zero=(0, 0, 0))
    assert np.array_equal(bits(g_out[:, 0, 0, 0]), bits(lm).reshape(3, 1404))
    assert same_nonfinite(g_out[0, 1, 1, 1].reshape(468, 3), out[0])


# ---- host against numpy on more faces --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotation_type", TYPES)
def test_host_equals_numpy_on_philox_faces(rotation_type):
    lm, poses = special_faces(60, seed=21), random_poses(60, seed=22)
    rot = IR.pose_matrices(poses, rotation_type)
    out, out64 = host_faces(lm, rot)
    want = numpy_faces(lm, rot)
    assert np.array_equal(bits(out64), bits(want))
    assert np.array_equal(bits(out), bits(want.astype(np.float32)))


# ---- argument checks, in the stated order ---------------------------------------------------------------------------------------
def _err():
    return _lib.lib().nlml_last_error().decode()


def _grid_args(base=FAKE, I=2, ry=FAKE, ny=3, rp=FAKE, np_=3, rr=FAKE, nr=3, order=0, zero=(1, 1, 1), out=FAKE, out64=None):
    return (base, I, ry, ny, rp, np_, rr, nr, order, *zero, out, out64)


@pytest.mark.parametrize("case, kw, text", [
    ("null base before a negative extent", dict(base=None, ny=-1, order=7), "null buffer"),
    ("null table", dict(rp=None, order=7, zero=(9, 9, 9)), "null buffer"),
    ("null out", dict(out=None, out64=FAKE), "null buffer"),
    ("negative extent before an unknown order", dict(I=-2, order=7, zero=(9, 9, 9)), "negative extent"),
    ("negative bins", dict(nr=-1, zero=(1, 1, -1)), "negative extent"),
    ("unknown order before a bad zero index", dict(order=2, zero=(3, 1, 1)), "unknown order"),
    ("zero index too large", dict(zero=(3, 1, 1)), "zero index"),
    ("zero index below -1", dict(zero=(1, -2, 1)), "zero index"),
    ("bad zero index of an empty grid", dict(I=0, zero=(1, 1, 3)), "zero index"),
    ("misaligned base", dict(base=FAKE + 4), "16-byte"),
    ("misaligned out", dict(out=FAKE + 8), "16-byte"),
    ("misaligned out64", dict(out64=FAKE + 4), "8-byte"),
    ("misaligned table", dict(rr=FAKE + 4), "8-byte"),
    ("too large", dict(I=2 ** 62), "too large"),
])
def test_grid_entry_point_refuses(case, kw, text):
    assert _lib.lib().nlml_compose_rotation_tensor(*_grid_args(**kw), None) == BADARG, case
    assert text in _err() and "compose_rotation_tensor" in _err(), (case, _err())


def test_grid_entry_point_empty_extents_launch_nothing():
    L = _lib.lib()
    for kw in (dict(I=0), dict(ny=0, zero=(-1, 1, 1)), dict(np_=0, zero=(1, -1, 1)), dict(nr=0, zero=(1, 1, -1))):
        nothing = dict(base=None, ry=None, rp=None, rr=None, out=None)
        assert L.nlml_compose_rotation_tensor(*_grid_args(**{**nothing, **kw}), None) == 0, kw
        assert L.nlml_compose_rotation_tensor(*_grid_args(**{**kw, "base": FAKE + 4}), None) == 0, kw      # no buffer looked at
        assert L.nlml_compose_rotation_tensor_host(*_grid_args(**{**nothing, **kw})) == 0, kw


@pytest.mark.parametrize("case, args, text", [
    ("null lm before a negative B", (None, FAKE, FAKE, None, -4), "null buffer"),
    ("null rot", (FAKE, None, FAKE, None, 4), "null buffer"),
    ("neither out nor out64", (FAKE, FAKE, None, None, 4), "null buffer"),
    ("negative B", (FAKE, FAKE, FAKE, None, -4), "negative extent"),
    ("misaligned lm", (FAKE + 8, FAKE, FAKE, None, 4), "16-byte"),
    ("misaligned out", (FAKE, FAKE, FAKE + 4, None, 4), "16-byte"),
    ("misaligned rot", (FAKE, FAKE + 4, FAKE, None, 4), "8-byte"),
    ("misaligned out64", (FAKE, FAKE, None, FAKE + 4, 4), "8-byte"),
])
def test_face_entry_point_refuses(case, args, text):
    assert _lib.lib().nlml_rotate_landmarks(*args, None) == BADARG, case
    assert text in _err() and "rotate_landmarks" in _err(), (case, _err())


def test_face_entry_point_empty_and_host_refusals():
    L = _lib.lib()
    assert L.nlml_rotate_landmarks(None, None, None, None, 0, None) == 0
    assert L.nlml_rotate_landmarks(FAKE + 4, FAKE, FAKE, None, 0, None) == 0
    assert L.nlml_rotate_landmarks_host(None, None, None, None, 0) == 0
    buf = np.zeros((1404,), np.float32)
    m = np.zeros((27,), np.float64)
    assert L.nlml_rotate_landmarks_host(None, m.ctypes.data, buf.ctypes.data, None, 1) == BADARG and "null" in _err()
    assert L.nlml_rotate_landmarks_host(buf.ctypes.data, m.ctypes.data, None, None, 1) == BADARG and "null" in _err()
    assert L.nlml_rotate_landmarks_host(buf.ctypes.data, m.ctypes.data, buf.ctypes.data, None, -1) == BADARG and "negative" in _err()
    assert L.nlml_compose_rotation_tensor_host(*_grid_args(out=None)) == BADARG and "null" in _err()
    assert L.nlml_compose_rotation_tensor_host(*_grid_args(order=5)) == BADARG and "unknown order" in _err()


# ---- the layers above, as far as they go without a GPU --------------------------------------------------------------------------
def test_meta_kernel_shapes():
    base = torch.empty((5, 468, 3), dtype=torch.float32, device="meta")
    t = [torch.empty((n, 3, 3), dtype=torch.float64, device="meta") for n in (11, 9, 7)]
    out, out64 = torch.ops.nlml_hpe.compose_rotation_tensor(base, *t, 0, [5, 4, 3], True)
    assert tuple(out.shape) == (5, 11, 9, 7, 1404) == tuple(out64.shape) and out.dtype == torch.float32 and out64.dtype == torch.float64
    out, out64 = torch.ops.nlml_hpe.compose_rotation_tensor(base[:0], *t, 0, [5, 4, 3])
    assert tuple(out.shape) == (0, 11, 9, 7, 1404) and tuple(out64.shape) == (0,)
    rot = torch.empty((5, 3, 3, 3), dtype=torch.float64, device="meta")
    a, b = torch.ops.nlml_hpe.rotate_landmarks(base, rot, True, True)
    assert tuple(a.shape) == (5, 468, 3) == tuple(b.shape) and a.dtype == torch.float32 and b.dtype == torch.float64
    a, b = torch.ops.nlml_hpe.rotate_landmarks(base, rot)
    assert tuple(a.shape) == (5, 468, 3) and tuple(b.shape) == (0,)


def test_cpu_tensors_are_refused():
    base, t = torch.zeros((2, 468, 3)), torch.zeros((3, 3, 3), dtype=torch.float64)
    with pytest.raises(_lib.NlmlError, match="no CPU fallback"):
        ops.compose_rotation_tensor(base, t, t, t)
    with pytest.raises(_lib.NlmlError, match="no CPU fallback"):
        ops.rotate_landmarks(base, torch.zeros((2, 3, 3, 3), dtype=torch.float64))
    with pytest.raises(Exception):
        torch.ops.nlml_hpe.compose_rotation_tensor(base, t, t, t, 0, [-1, -1, -1])
    with pytest.raises(Exception):
        torch.ops.nlml_hpe.rotate_landmarks(base, torch.zeros((2, 3, 3, 3), dtype=torch.float64))


def test_compose_tensor_refusals():
    base = np.zeros((2, 468, 3), np.float32)
    bins = ([-10, 0, 10], [0], [0, 5])
    with pytest.raises(NotImplementedError, match="FaceMesh"):
        CT.Compose_Tensor(base, (2, 3, 1, 2, 1404), *bins, use_rotation_features=0)
    with pytest.raises(ValueError, match="disagrees"):
        CT.Compose_Tensor(base, (2, 3, 1, 3, 1404), *bins)
    with pytest.raises(ValueError, match="disagrees"):
        CT.Compose_Tensor(base, (3, 3, 1, 2, 1404), *bins)
    with pytest.raises(ValueError, match="identities"):
        CT.Compose_Tensor(base, (2, 3, 1, 2, 1404), *bins, identities=["a"])
    with pytest.raises(ValueError, match="value 0 2 times"):
        CT.Compose_Tensor(base, (2, 3, 1, 2, 1404), [-10, 0, 0.0], [0], [0, 5])
    with pytest.raises(TypeError, match="float32"):
        CT.Compose_Tensor(base.astype(np.float64), (2, 3, 1, 2, 1404), *bins)
    with pytest.raises(ValueError, match="468,3"):
        CT.Compose_Tensor(base[0], (2, 3, 1, 2, 1404), *bins)
    with pytest.raises(ValueError, match="468,3"):
        IR.apply_rotations(base, [1, 2, 3])
    with pytest.raises(ValueError, match="intrinsic"):
        IR.apply_rotations(base[0], [1, 2, 3], "euler")
    with pytest.raises(ValueError, match="angles_deg"):
        IR.apply_rotations_batch(base, np.zeros((3, 3)))


# ---- the stand-alone program under the sanitizers --------------------------------------------------------------------------------
def test_rotate_ref_under_asan_ubsan(tmp_path, repo_root):
    exe = tmp_path / "rotate_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-o", str(exe),
           os.path.join(repo_root, "tests", "native", "rotate_host.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "rotate host ok" in res.stdout
