"""Landmark rotation on the GPU (csrc/rotate_landmarks.hip): the kernel against the reference's recorded results (FX12) through every
layer, and against the host restatement of the same operation order, bit for bit.  Reads fixtures only, never the reference."""
import numpy as np
import pytest
import torch

from nlml_hpe_amd import CreateTensor as CT
from nlml_hpe_amd import IntrinsicRotation as IR
from nlml_hpe_amd import _lib, ops
from test_rotation_host import (NEG0_32, TYPES, bits, grid_tables, host_faces, host_grid, load_fx12, nonfinite_faces, random_poses,
                                same_nonfinite, sign_block, special_faces)

pytestmark = pytest.mark.gpu

CANARY32, CANARY64 = 0x7FC12345, 0x7FF8000012345678      # NaN patterns no computation here produces
GUARD = 4096                                              # elements behind each output that must stay untouched


def _filled(n, dtype, device):
    """n elements of the canary and GUARD more behind them -> (whole buffer as integers, the first n as floats)."""
    it, canary = (torch.int32, CANARY32) if dtype == torch.float32 else (torch.int64, CANARY64)
    whole = torch.full((n + GUARD,), canary, dtype=it, device=device)
    return whole, whole[:n].view(dtype)


def _guard_intact(whole, n):
    canary = CANARY32 if whole.dtype == torch.int32 else CANARY64
    return bool((whole[n:] == canary).all())


def device_grid(base_t, tables_t, order, zero, want64):
    """nlml_compose_rotation_tensor itself on torch's current stream -> (out, out64 | None, guards intact)."""
    I, (ny, np_, nr) = base_t.shape[0], (t.shape[0] for t in tables_t)
    n = I * ny * np_ * nr * 1404
    w32, out = _filled(n, torch.float32, base_t.device)
    w64, out64 = _filled(n, torch.float64, base_t.device) if want64 else (None, None)
    rc = _lib.lib().nlml_compose_rotation_tensor(base_t.data_ptr(), I, tables_t[0].data_ptr(), ny, tables_t[1].data_ptr(), np_,
                                                 tables_t[2].data_ptr(), nr, _lib.rot_order_from_name(order), *zero, out.data_ptr(),
                                                 out64.data_ptr() if want64 else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().nlml_last_error()
    shape = (I, ny, np_, nr, 1404)
    return out.view(shape), out64.view(shape) if want64 else None, lambda: _guard_intact(w32, n) and (not want64 or _guard_intact(w64, n))


def device_faces(lm_t, rot_t, want32, want64):
    B = lm_t.shape[0]
    n = B * 1404
    w32, out = _filled(n, torch.float32, lm_t.device) if want32 else (None, None)
    w64, out64 = _filled(n, torch.float64, lm_t.device) if want64 else (None, None)
    rc = _lib.lib().nlml_rotate_landmarks(lm_t.data_ptr(), rot_t.data_ptr(), out.data_ptr() if want32 else None,
                                          out64.data_ptr() if want64 else None, B, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib().nlml_last_error()
    ok = lambda: (not want32 or _guard_intact(w32, n)) and (not want64 or _guard_intact(w64, n))  # noqa: E731
    return (out.view(B, 468, 3) if want32 else None), (out64.view(B, 468, 3) if want64 else None), ok


def grid_case(I, ny, np_, nr, order, seed):
    """Random bins with a zero bin in the middle of every axis -> (base, tables, zero)."""
    g = np.random.default_rng(seed)
    zero = (ny // 2, np_ // 2, nr // 2)
    axes = []
    for n, z in zip((ny, np_, nr), zero):
        a = g.uniform(-170.0, 170.0, n)
        a[z] = 0.0
        if n > 3:
            a[0] = 90.0
        axes.append(a)
    return special_faces(I, seed), grid_tables(*axes, order), zero


def dev(arrays, device):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


# ---- the reference's bits through every layer ------------------------------------------------------------------------------------
def test_fx12_tensor_through_every_layer(device, golden_dir):
    g = load_fx12(golden_dir)
    base_t = torch.from_numpy(g["base"]).to(device)
    tabs = dev(grid_tables(g["yaw"], g["pitch"], g["roll"]), device)
    want = g["tensor_bits"]
    out, out64 = ops.compose_rotation_tensor(base_t, *tabs, order="intrinsic", zero_index=(1, 1, 1), return_f64=True)
    assert np.array_equal(bits(out.cpu().numpy()), want)
    assert np.array_equal(bits(out64.cpu().numpy().astype(np.float32)), want)
    assert np.array_equal(bits(ops.compose_rotation_tensor(base_t, *tabs, zero_index=(1, 1, 1)).cpu().numpy()), want)
    t_out, t_out64 = torch.ops.nlml_hpe.compose_rotation_tensor(base_t, *tabs, 0, [1, 1, 1], True)
    assert np.array_equal(bits(t_out.cpu().numpy()), want) and torch.equal(t_out64.view(torch.int64), out64.view(torch.int64))
    t_out, t_none = torch.ops.nlml_hpe.compose_rotation_tensor(base_t, *tabs, 0, [1, 1, 1])
    assert np.array_equal(bits(t_out.cpu().numpy()), want) and t_none.numel() == 0
    for base_in in (g["base"], base_t):                                    # host landmarks are uploaded, device landmarks used as they are
        tensor, flag = CT.Compose_Tensor(base_in, want.shape, g["yaw"], g["pitch"], g["roll"], identities=["0", "1"])
        assert flag is False and tensor.is_cuda and tensor.dtype == torch.float32
        assert np.array_equal(bits(tensor.cpu().numpy()), want)
    assert (bits(out.cpu().numpy())[1, 1, 1, 1, 900:903] == NEG0_32).all()   # landmark 300 of identity 1: copied, -0.0 kept
    # a strided view is made contiguous
    wide = torch.zeros((2, 468, 4), dtype=torch.float32, device=device)
    wide[:, :, :3] = base_t
    assert np.array_equal(bits(ops.compose_rotation_tensor(wide[:, :, :3], *tabs, zero_index=(1, 1, 1)).cpu().numpy()), want)
    assert np.array_equal(bits(torch.ops.nlml_hpe.compose_rotation_tensor(wide[:, :, :3], *tabs, 0, [1, 1, 1])[0].cpu().numpy()), want)


@pytest.mark.parametrize("k, rotation_type", list(enumerate(TYPES)))
def test_fx12_apply_rotations_through_every_layer(device, golden_dir, k, rotation_type):
    g = load_fx12(golden_dir)
    want = g["apply_f64_bits"][k]
    P = len(g["poses"])
    for j, pose in enumerate(g["poses"]):
        r = IR.apply_rotations(g["base"][1], list(pose), rotation_type)
        assert r.is_cuda and r.dtype == torch.float64 and tuple(r.shape) == (468, 3)
        assert np.array_equal(bits(r.cpu().numpy()), want[j]), (rotation_type, j)
    lm = np.ascontiguousarray(np.broadcast_to(g["base"][1], (P, 468, 3)))
    b64 = IR.apply_rotations_batch(lm, g["poses"], rotation_type)
    b32 = IR.apply_rotations_batch(lm, g["poses"], rotation_type, dtype=torch.float32)
    assert np.array_equal(bits(b64.cpu().numpy()), want)
    assert np.array_equal(bits(b32.cpu().numpy()), bits(want.view(np.float64).astype(np.float32)))
    lm_t, rot_t = dev([lm, IR.pose_matrices(g["poses"], rotation_type)], device)
    o32, o64 = ops.rotate_landmarks(lm_t, rot_t, return_f64=True)
    assert np.array_equal(bits(o64.cpu().numpy()), want) and torch.equal(o32.view(torch.int32), b32.view(torch.int32))
    t32, t64 = torch.ops.nlml_hpe.rotate_landmarks(lm_t, rot_t, True, True)
    assert torch.equal(t32.view(torch.int32), b32.view(torch.int32)) and torch.equal(t64.view(torch.int64), b64.view(torch.int64))
    t32, t_none = torch.ops.nlml_hpe.rotate_landmarks(lm_t, rot_t)
    assert torch.equal(t32.view(torch.int32), b32.view(torch.int32)) and t_none.numel() == 0
    # the signed-zero table
    sb = np.ascontiguousarray(np.broadcast_to(sign_block(g), (P, 468, 3)))
    s64 = IR.apply_rotations_batch(sb, g["poses"], rotation_type).cpu().numpy()
    assert np.array_equal(bits(s64[:, :64]), g["signs_f64_bits"][k])


# ---- the kernel against the host restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", TYPES)
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 1, 7), (5, 3, 2, 2), (2, 11, 9, 7), (65, 2, 1, 3)])
def test_grid_equals_host_restatement(device, shape, order):
    base, tables, zero = grid_case(*shape, order, seed=sum(shape))
    exp, exp64 = host_grid(base, tables, order, zero)
    exp_nocopy, _ = host_grid(base, tables, order, (-1, -1, -1), want64=False)
    side = torch.cuda.Stream(device=device)
    base_t, *tabs = dev([base, *tables], device)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(side):                   # a non-default stream
        with64 = device_grid(base_t, tabs, order, zero, True)
        without = device_grid(base_t, tabs, order, zero, False)
        nocopy = device_grid(base_t, tabs, order, (-1, -1, -1), False)
    side.synchronize()
    assert np.array_equal(bits(with64[0].cpu().numpy()), bits(exp)) and np.array_equal(bits(with64[1].cpu().numpy()), bits(exp64))
    assert np.array_equal(bits(without[0].cpu().numpy()), bits(exp)) and without[1] is None
    assert np.array_equal(bits(nocopy[0].cpu().numpy()), bits(exp_nocopy))
    assert with64[2]() and without[2]() and nocopy[2]()
    # the copied cell is the base and holds its -0.0; rotated, it does not
    cell = (slice(None),) + zero
    assert np.array_equal(bits(exp[cell]), bits(base).reshape(-1, 1404)) and (bits(exp[cell])[:, 33:36] == NEG0_32).all()
    assert (bits(exp_nocopy[cell])[:, 33:36] == 0).all()


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("rotation_type", TYPES)
def test_faces_equal_host_restatement(device, B, rotation_type):
    lm, rot = special_faces(B, seed=200 + B), IR.pose_matrices(random_poses(B, seed=300 + B), rotation_type)
    exp, exp64 = host_faces(lm, rot)
    lm_t, rot_t = dev([lm, rot], device)
    for want32, want64 in ((True, False), (False, True), (True, True)):
        out, out64, guards = device_faces(lm_t, rot_t, want32, want64)
        torch.cuda.synchronize(device)
        if want32:
            assert np.array_equal(bits(out.cpu().numpy()), bits(exp)), (B, want32, want64)
        if want64:
            assert np.array_equal(bits(out64.cpu().numpy()), bits(exp64)), (B, want32, want64)
        assert guards(), (B, want32, want64)


@pytest.mark.parametrize("order", TYPES)
def test_grid_and_face_modes_agree(device, order):
    I, ny, np_, nr = 3, 4, 3, 2
    base, tables, zero = grid_case(I, ny, np_, nr, order, seed=77)
    base_t, *tabs = dev([base, *tables], device)
    grid32, grid64 = ops.compose_rotation_tensor(base_t, *tabs, order=order, zero_index=zero, return_f64=True)
    # every cell as a face with its own three matrices in application order
    ry, rp, rr = tables
    idx = np.stack(np.meshgrid(np.arange(I), np.arange(ny), np.arange(np_), np.arange(nr), indexing="ij"), -1).reshape(-1, 4)
    stages = (rp[idx[:, 2]], ry[idx[:, 1]], rr[idx[:, 3]]) if order == "intrinsic" else (rr[idx[:, 3]], ry[idx[:, 1]], rp[idx[:, 2]])
    lm_t, rot_t = dev([base[idx[:, 0]], np.stack(stages, axis=1)], device)
    face32, face64 = ops.rotate_landmarks(lm_t, rot_t, return_f64=True)
    same32 = (grid32.reshape(-1, 1404).view(torch.int32) == face32.reshape(-1, 1404).view(torch.int32)).all(dim=1).cpu().numpy()
    same64 = (grid64.reshape(-1, 1404).view(torch.int64) == face64.reshape(-1, 1404).view(torch.int64)).all(dim=1).cpu().numpy()
    copied = (idx[:, 1:] == np.array(zero)).all(axis=1)
    assert copied.sum() == I and same32[~copied].all() and same64[~copied].all()
    assert not same32[copied].any() and not same64[copied].any()       # the copy keeps the -0.0 the rotation loses


@pytest.mark.parametrize("rotation_type", TYPES)
def test_nonfinite_inputs_on_the_device(device, rotation_type):
    lm = nonfinite_faces()
    rot = IR.pose_matrices([(31, 12, -7), (0, 0, 17), (90, 0, 0)], rotation_type)
    exp, exp64 = host_faces(lm, rot)
    lm_t, rot_t = dev([lm, rot], device)
    out, out64 = ops.rotate_landmarks(lm_t, rot_t, return_f64=True)
    assert same_nonfinite(out.cpu().numpy(), exp) and same_nonfinite(out64.cpu().numpy(), exp64)
    assert np.isnan(exp64).any() and np.isposinf(exp).any() and np.isneginf(exp).any()
    # grid mode: the copied cell carries the non-finite inputs through bit for bit
    tables = grid_tables([0, 31], [0, 12], [0, -7], rotation_type)
    g_out = ops.compose_rotation_tensor(lm_t, *dev(tables, device), order=rotation_type, zero_index=(0, 0, 0)).cpu().numpy()
    assert np.array_equal(bits(g_out[:, 0, 0, 0]), bits(lm).reshape(3, 1404))
    assert same_nonfinite(g_out, host_grid(lm, tables, rotation_type, (0, 0, 0), want64=False)[0])


def test_byte_offsets_beyond_4_gib(device):
    """(1104, 11, 9, 7, 1404) f32 = 4.297 GB: the smallest number of identities of the reference's grid whose last block crosses 2^32
    bytes.  Three identities with faces of their own are compared ON THE DEVICE with single-identity calls; the rest are copies of a
    fourth face.  (Element offsets beyond 2^31 are covered by reading: every row and byte offset in the kernel is int64_t.)"""
    I, ny, np_, nr = 1104, 11, 9, 7
    assert (I - 1) * ny * np_ * nr * 5616 < 2 ** 32 < I * ny * np_ * nr * 5616
    faces = special_faces(4, seed=5)
    own = (0, 551, 1103)
    base = np.broadcast_to(faces[3], (I, 468, 3)).copy()
    base[list(own)] = faces[:3]
    _, tables, zero = grid_case(1, ny, np_, nr, "intrinsic", seed=6)
    base_t, *tabs = dev([base, *tables], device)
    out = ops.compose_rotation_tensor(base_t, *tabs, zero_index=zero)
    assert out.numel() * 4 > 2 ** 32
    for k, i in enumerate(own):
        one = ops.compose_rotation_tensor(base_t[i:i + 1], *tabs, zero_index=zero)
        assert torch.equal(out[i].view(torch.int32), one[0].view(torch.int32)), i
        if k:
            assert not torch.equal(out[i].view(torch.int32), out[own[0]].view(torch.int32))
    filler = ops.compose_rotation_tensor(base_t[1:2], *tabs, zero_index=zero)
    assert torch.equal(out[I - 2].view(torch.int32), filler[0].view(torch.int32))
    del out
    torch.cuda.empty_cache()


def test_empty_extents(device):
    base = torch.zeros((2, 468, 3), dtype=torch.float32, device=device)
    t = lambda n: torch.zeros((n, 3, 3), dtype=torch.float64, device=device)  # noqa: E731
    for I, ny, np_, nr in ((0, 3, 2, 2), (2, 0, 2, 2), (2, 3, 0, 2), (2, 3, 2, 0)):
        out, out64 = ops.compose_rotation_tensor(base[:I], t(ny), t(np_), t(nr), return_f64=True)
        assert tuple(out.shape) == (I, ny, np_, nr, 1404) == tuple(out64.shape) and out.numel() == 0
        assert tuple(torch.ops.nlml_hpe.compose_rotation_tensor(base[:I], t(ny), t(np_), t(nr), 0, [-1, -1, -1])[0].shape) == tuple(out.shape)
    rot = torch.zeros((0, 3, 3, 3), dtype=torch.float64, device=device)
    o32, o64 = ops.rotate_landmarks(base[:0], rot, return_f64=True)
    assert tuple(o32.shape) == (0, 468, 3) == tuple(o64.shape)
    assert tuple(torch.ops.nlml_hpe.rotate_landmarks(base[:0], rot)[0].shape) == (0, 468, 3)
    tensor, _ = CT.Compose_Tensor(np.zeros((0, 468, 3), np.float32), (0, 2, 1, 1, 1404), [0, 5], [0], [0])
    assert tuple(tensor.shape) == (0, 2, 1, 1, 1404)
    assert tuple(IR.apply_rotations_batch(np.zeros((0, 468, 3), np.float32), np.zeros((0, 3))).shape) == (0, 468, 3)
