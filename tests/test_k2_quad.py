"""The strict-fast mode's four-tile kernel (csrc/encoder_heads_f16x2_w8.hip, encoder_heads_f16x2_w8q_kernel): a workgroup runs layers 0-2
over four 64-face tiles, parks each tile's layer-2 output in its own slice of a workspace and then runs the streamed tail once over its
256 faces.  Everything here is torch.equal on pose, latent and the "no face" mask against the FUSED kernel, reached through the plain C
entry points (nlml_landmarks_to_pose / nlml_encoder_heads_fwd: they take no workspace and cannot leave the fused kernel), with the strict
blob of synth.encoder_state_dict(1404, seed=0) plus the shipped heads unless a test says otherwise.  The split arithmetic of the
dispatcher is checked without a GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nlml_hpe_amd import _lib, ops, synth, weights
from oracle import encoder_heads as EH

F_REF = 1404


def _strict_blob(head_sds, device, F=F_REF, seed=0):
    return torch.from_numpy(weights.pack_blob(synth.encoder_state_dict(F, seed=seed), head_sds, _lib.MODE_F16X2S)).to(device)


@pytest.fixture(scope="module")
def blob(head_sds, device):
    return _strict_blob(head_sds, device)


def _call(symbol, head, B, blob, device, ws=None, want_latent=True, want_valid=True):
    """One call of a C forward: head = the arguments in front of the blob.  -> (rc, pose, latent, valid)."""
    L = _lib.lib()
    out = torch.full((B, 3), float("nan"), dtype=torch.float32, device=device)
    lat = torch.full((B, 9), float("nan"), dtype=torch.float32, device=device) if want_latent else None
    val = torch.full((B,), 7, dtype=torch.uint8, device=device) if want_valid else None
    tail = () if ws is None else (ws.data_ptr(), ws.numel())
    rc = getattr(L, symbol)(*head, blob.data_ptr(), blob.numel(), out.data_ptr(), lat.data_ptr() if want_latent else None,
                            val.data_ptr() if want_valid else None, *tail, torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize(device)
    return rc, out, lat, val


def _workspace(B, device, F=F_REF, fill=None):
    ws = torch.empty((max(16, _lib.lib().nlml_encoder_heads_workspace_bytes(B, F)),), dtype=torch.uint8, device=device)
    if fill is not None:
        ws.fill_(fill)
    return ws


def _same(a, b, what):
    for name, x, y in zip(("pose", "latent", "valid"), a, b):
        if x is None and y is None:
            continue
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), f"{what}: {name} differs from the fused kernel's"


# ---- 1. the explicit entry point, raw landmarks
RAW_SIZES = [1, 63, 64, 65, 255, 256, 257, 320, 511, 513, 1061]


@pytest.fixture(scope="module")
def raw_all(device):
    raw = synth.raw_landmarks(max(RAW_SIZES), seed=6)
    raw[7] = 0.0   # a "no face" row
    return torch.from_numpy(raw).to(device)


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B", RAW_SIZES)
def test_quad_entry_is_bit_identical_to_the_fused_kernel(B, normalize, blob, raw_all, device):
    """A lone partial tile (1, 63), a workgroup with three, two, one and no absent tiles (64, 65 .. 255, 256), a partial last block
    inside a present tile (65: one face of block 2; 320), more than one workgroup with a ragged end (257, 511, 513, 1061)."""
    raw = raw_all[:B].contiguous()
    rc, *want = _call("nlml_landmarks_to_pose", (raw.data_ptr(), B, int(normalize)), B, blob, device)
    assert rc == 0
    rc, *got = _call("nlml_landmarks_to_pose_quad", (raw.data_ptr(), B, int(normalize)), B, blob, device, ws=_workspace(B, device))
    assert rc == 0, _lib.lib().nlml_last_error()
    _same(got, want, f"B={B} normalize={normalize}")
    rc, o, _, _ = _call("nlml_landmarks_to_pose_quad", (raw.data_ptr(), B, int(normalize)), B, blob, device, ws=_workspace(B, device),
                        want_latent=False, want_valid=False)
    assert rc == 0 and torch.equal(o, want[0])   # (no latent, no mask asked for)


# ---- 2. feature rows: a padded row stride, another input width
@pytest.mark.gpu
@pytest.mark.parametrize("B", [257, 513])
def test_quad_entry_with_feature_rows_a_padded_stride_and_another_width(B, blob, head_sds, device):
    buf = torch.zeros((B, F_REF + 4), dtype=torch.float32, device=device)
    buf[:, :F_REF] = torch.from_numpy(synth.features(B, F_REF, seed=12)).to(device)
    rc, *want = _call("nlml_encoder_heads_fwd", (buf.data_ptr(), F_REF + 4, B, F_REF), B, blob, device)
    assert rc == 0
    rc, *got = _call("nlml_encoder_heads_fwd_quad", (buf.data_ptr(), F_REF + 4, B, F_REF), B, blob, device, ws=_workspace(B, device))
    assert rc == 0, _lib.lib().nlml_last_error()
    _same(got, want, f"ldx = F + 4, B={B}")
    got = ops.encoder_heads_fwd_quad(buf[:, :F_REF], blob, F_REF, return_latent=True, return_valid=True)      # the wrapper, same rows
    _same((got[0], got[1], got[2].to(torch.uint8)), want, f"ops.encoder_heads_fwd_quad, B={B}")
    F = 136   # 12 K steps of 16 in layer 0 instead of 88: every offset of the tail's units and bias table moves with it
    blob_f = _strict_blob(head_sds, device, F=F)
    x = torch.from_numpy(synth.features(B, F, seed=31)).to(device)
    rc, *want = _call("nlml_encoder_heads_fwd", (x.data_ptr(), F, B, F), B, blob_f, device)
    assert rc == 0
    rc, *got = _call("nlml_encoder_heads_fwd_quad", (x.data_ptr(), F, B, F), B, blob_f, device, ws=_workspace(B, device, F))
    assert rc == 0, _lib.lib().nlml_last_error()
    _same(got, want, f"F = 136, B={B}")


# ---- 3. flagged faces go to the re-evaluation launch
@pytest.mark.gpu
def test_quad_entry_flagged_faces_take_the_reevaluation_launch(blob, head_sds, device):
    """Rows scaled by 3.4e4 (the streamed-path tests' construction): features near 6.8e4 have no finite f16 hi piece, so the split-f16
    kernels leave a non-finite pose and the f32 re-evaluation launch rewrites those faces; in f32 the same rows are finite (CPU oracle).
    One flagged face in a workgroup's first tile, one in its last, one in the partial tile of the third workgroup, and an all-zero row."""
    B = 513
    sd = synth.encoder_state_dict(F_REF, seed=0)
    x = synth.features(B, F_REF, seed=78)
    flagged = np.zeros(B, bool)
    flagged[[5, 64 * 3 + 40, 512]] = True
    bad = x.copy()
    bad[flagged] *= 3.4e4
    bad[100] = 0.0
    with np.errstate(over="ignore"):
        assert np.isinf(bad[flagged].astype(np.float16)).any(axis=1).all()                        # beyond f16's range: non-finite in split-f16
    assert np.isfinite(EH.forward_numpy(bad[flagged], EH.Params(sd, head_sds), np.float32)).all()  # finite in f32
    xb = torch.from_numpy(bad).to(device)
    rc, *want = _call("nlml_encoder_heads_fwd", (xb.data_ptr(), F_REF, B, F_REF), B, blob, device)
    assert rc == 0
    rc, *got = _call("nlml_encoder_heads_fwd_quad", (xb.data_ptr(), F_REF, B, F_REF), B, blob, device, ws=_workspace(B, device))
    assert rc == 0, _lib.lib().nlml_last_error()
    _same(got, want, "flagged faces")
    assert torch.isfinite(got[0]).all()
    blob32 = torch.from_numpy(weights.pack_blob(sd, head_sds)).to(device)
    rc, o32, l32, _ = _call("nlml_encoder_heads_fwd", (xb.data_ptr(), F_REF, B, F_REF), B, blob32, device)
    fl = torch.from_numpy(flagged).to(device)
    assert rc == 0 and torch.equal(got[0][fl], o32[fl]) and torch.equal(got[1][fl], l32[fl])      # the strict parity kernel's bits
    assert got[2][100] == 0 and int(got[2].sum()) == B - 1


# ---- 4. the workspace: contents never matter, its size and alignment do
@pytest.mark.gpu
def test_quad_entry_workspace_contents_size_and_alignment(blob, raw_all, head_sds, device):
    """A dirty workspace gives the same bits; one of exactly nlml_encoder_heads_workspace_bytes works; what is refused is what the
    _streamed form refuses, with its code: a workspace one byte short of the hand-over (1 KB per face of whole tiles -- at 513 faces the
    documented size is larger, it also covers the layer-per-launch path), a misaligned one, a blob of another mode, unaligned rows."""
    L = _lib.lib()
    B = 513
    raw = raw_all[:B].contiguous()
    head = (raw.data_ptr(), B, 1)
    rc, *want = _call("nlml_landmarks_to_pose", head, B, blob, device)
    assert rc == 0
    for fill in (0x7F, 0xFF):   # 0x7f7f.. = f16 NaN bit patterns in every fragment; 0xff.. = NaN with the sign set
        ws = _workspace(B, device, fill=fill)
        rc, *got = _call("nlml_landmarks_to_pose_quad", head, B, blob, device, ws=ws)
        assert rc == 0, L.nlml_last_error()
        _same(got, want, f"workspace filled with {fill:#x}")
    need = L.nlml_encoder_heads_workspace_bytes(B, F_REF)
    assert need >= 9 * 65536                                       # covers the hand-over: 1 KB per face of whole 64-face tiles
    exact = torch.empty((need,), dtype=torch.uint8, device=device)
    rc, *got = _call("nlml_landmarks_to_pose_quad", head, B, blob, device, ws=exact)
    assert rc == 0
    _same(got, want, "a caller's workspace of exactly the documented size")
    rc, *_ = _call("nlml_landmarks_to_pose_quad", head, B, blob, device, ws=exact[:9 * 65536 - 1])     # one byte less than the hand-over
    assert rc == -1 and b"workspace" in L.nlml_last_error()
    rc_s, *_ = _call("nlml_landmarks_to_pose_streamed", head, B, blob, device, ws=exact[:9 * 65536 - 1])
    assert rc_s == rc                                              # the _streamed form's refusal
    big = torch.empty((need + 16,), dtype=torch.uint8, device=device)
    rc, *_ = _call("nlml_landmarks_to_pose_quad", head, B, blob, device, ws=big[4:])
    assert rc == -1 and b"aligned" in L.nlml_last_error()
    blob_fast = torch.from_numpy(weights.pack_blob(synth.encoder_state_dict(F_REF, seed=0), head_sds, _lib.MODE_F16X2)).to(device)
    rc, *_ = _call("nlml_landmarks_to_pose_quad", head, B, blob_fast, device, ws=exact)
    assert rc == -1 and b"F16X2S" in L.nlml_last_error()            # strict-fast blob only
    x = torch.from_numpy(synth.features(B + 1, F_REF, seed=2)).to(device)
    rc, *_ = _call("nlml_encoder_heads_fwd_quad", (x.data_ptr() + 4, F_REF, B, F_REF), B, blob, device, ws=exact)
    assert rc == -1 and b"aligned" in L.nlml_last_error()           # rows that cannot be read 16 bytes at a time
    assert L.nlml_landmarks_to_pose_quad(raw.data_ptr(), 0, 1, blob.data_ptr(), blob.numel(), None, None, None, None, 0, None) == 0
    got = ops.landmarks_to_pose_quad(raw, blob, True, return_latent=True, return_valid=True)         # the wrapper and its pooled buffer
    _same((got[0], got[1], got[2].to(torch.uint8)), want, "ops.landmarks_to_pose_quad")
    assert torch.equal(ops.landmarks_to_pose_quad(raw[:100], blob), want[0][:100])


# ---- 5. and 6. the dispatcher, one child process per environment (its variables are read once per process)
_CHILD = r"""
import ctypes as C, os, sys
sys.path.insert(0, %(root)r)
import torch
from nlml_hpe_amd import _lib, ops, synth, weights
dev = torch.device("cuda:0")
heads = weights.load_head_state_dicts(os.path.join(%(root)r, "models"))
blob = torch.from_numpy(weights.pack_blob(synth.encoder_state_dict(1404, seed=0), heads, _lib.MODE_F16X2S)).to(dev)
L = _lib.lib()
st = torch.cuda.current_stream().cuda_stream
B = int(sys.argv[1])
raw = torch.from_numpy(synth.raw_landmarks(B, seed=4)).to(dev)
raw[B // 2] = 0.0
def call(symbol, ws):
    out = torch.full((B, 3), float("nan"), dtype=torch.float32, device=dev)
    lat = torch.full((B, 9), float("nan"), dtype=torch.float32, device=dev)
    val = torch.full((B,), 7, dtype=torch.uint8, device=dev)
    tail = () if ws is None else (ws.data_ptr(), ws.numel())
    rc = getattr(L, symbol)(raw.data_ptr(), B, 1, blob.data_ptr(), blob.numel(), out.data_ptr(), lat.data_ptr(), val.data_ptr(), *tail, st)
    torch.cuda.synchronize()
    return rc, (out, lat, val)
def same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))
_, want = call("nlml_landmarks_to_pose", None)
n, need = C.c_int64(0), C.c_size_t(0)
assert L.nlml_k2_quad_faces(B, C.byref(n), C.byref(need)) == 0
full = torch.full((max(16, L.nlml_encoder_heads_workspace_bytes(B, 1404)),), 0xFF, dtype=torch.uint8, device=dev)
rc, got = call("nlml_landmarks_to_pose_ws", full)
# which bytes of the workspace the call wrote: the quad part's hand-over and nothing behind it
touched = int((full != 0xFF).any(dim=0)) and int(torch.nonzero(full != 0xFF).max()) + 1
tiny = torch.empty((int(sys.argv[2]),), dtype=torch.uint8, device=dev)
rc2, got2 = call("nlml_landmarks_to_pose_ws", tiny)
o = ops.landmarks_to_pose(raw, blob, True, return_latent=True, return_valid=True)
print("RESULT", n.value, need.value, rc, same(want, got) if rc == 0 else None, touched, rc2, same(want, got2) if rc2 == 0 else None,
      same(want, (o[0], o[1], o[2].to(torch.uint8))), L.nlml_last_error().decode()[:40] if rc2 else "-")
"""


def _child(repo_root, B, tiny_bytes, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("NLML_K2_QUAD_MIN", "NLML_K2_QUAD_CUS", "NLML_K2_STREAMED_MIN")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": repo_root}, str(B), str(tiny_bytes)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    f = [l for l in r.stdout.splitlines() if l.startswith("RESULT")][0].split(None, 9)
    return {"quad_faces": int(f[1]), "need": int(f[2]), "rc": int(f[3]), "same": f[4], "touched": int(f[5]), "rc_tiny": int(f[6]),
            "same_tiny": f[7], "ops_same": f[8], "err": f[9] if len(f) > 9 else ""}


@pytest.mark.gpu
def test_ws_dispatcher_takes_the_quad_path_from_the_size_the_environment_names(repo_root, device):
    """NLML_K2_QUAD_MIN=512: nlml_landmarks_to_pose_ws at 1,061 faces computes the fused kernel's bits through the four-tile kernel -- seen
    as the hand-over it leaves in the workspace (17 tiles x 64 KB) and as the refusal of a 64 KB workspace -- and ops.landmarks_to_pose
    follows."""
    r = _child(repo_root, 1061, 65536, {"NLML_K2_QUAD_MIN": "512"})
    assert r["quad_faces"] == 1061 and r["need"] == 17 * 65536
    assert r["rc"] == 0 and r["same"] == "True" and 16 * 65536 < r["touched"] <= 17 * 65536
    assert r["rc_tiny"] == -1 and "workspace" in r["err"]
    assert r["ops_same"] == "True"


@pytest.mark.gpu
def test_ws_dispatcher_without_the_variable_behaves_as_before_at_9000_faces(repo_root, device):
    """No whole round of 256-face workgroups on any device with more than 35 compute units: the fused kernel, whatever the workspace."""
    r = _child(repo_root, 9000, 1 << 20, {})
    assert r["quad_faces"] == 0 and r["need"] == 0
    assert r["rc"] == 0 and r["same"] == "True" and r["touched"] == 0
    assert r["rc_tiny"] == 0 and r["same_tiny"] == "True"
    assert r["ops_same"] == "True"


@pytest.mark.gpu
def test_a_negative_quad_min_switches_the_path_off(repo_root, device):
    """NLML_K2_QUAD_MIN=-1: no quad part at any size, even where every 256 faces would be a whole round (one compute unit): 4,708 faces
    go through the fused kernel, the workspace stays untouched, ops.landmarks_to_pose makes the plain call."""
    r = _child(repo_root, 4708, 65536, {"NLML_K2_QUAD_MIN": "-1", "NLML_K2_QUAD_CUS": "1"})
    assert r["quad_faces"] == 0 and r["touched"] == 0 and r["rc"] == 0 and r["same"] == "True" and r["ops_same"] == "True"


@pytest.mark.gpu
def test_mixed_launch_quad_part_and_fused_remainder_in_one_call(repo_root, device):
    """NLML_K2_QUAD_CUS=2 stands in for the device's compute-unit count: 4,708 = 2 * 256 * 9 + 100 faces (above the layer-per-launch
    path's 4,096) split into nine rounds of two workgroups through the four-tile kernel (4,608 faces, 72 tiles of hand-over) and 100
    faces through the fused kernel on offset pointers; every row, the latent and the mask against the fused kernel alone.  With a
    workspace too small for the quad part the call runs the fused kernel alone, as it would have before the path existed."""
    r = _child(repo_root, 4708, 65536, {"NLML_K2_QUAD_CUS": "2"})
    assert r["quad_faces"] == 4608 and r["need"] == 72 * 65536
    assert r["rc"] == 0 and r["same"] == "True" and 71 * 65536 < r["touched"] <= 72 * 65536
    assert r["rc_tiny"] == 0 and r["same_tiny"] == "True"
    assert r["ops_same"] == "True"


# ---- 6b. the hosts ask the library (nlml_k2_quad_part): what they then call, seen in ops' pooled workspaces
_CHILD_HOSTS = r"""
import os, sys
sys.path.insert(0, %(root)r)
import torch
from nlml_hpe_amd import _lib, ops, synth, weights
dev = torch.device("cuda:0")
heads = weights.load_head_state_dicts(os.path.join(%(root)r, "models"))
sd = synth.encoder_state_dict(1404, seed=0)
strict = torch.from_numpy(weights.pack_blob(sd, heads, _lib.MODE_F16X2S)).to(dev)
L = _lib.lib()
B, F = 4708, 1404
def plain(symbol, head, blob):
    out = torch.full((B, 3), float("nan"), dtype=torch.float32, device=dev)
    lat = torch.full((B, 9), float("nan"), dtype=torch.float32, device=dev)
    val = torch.full((B,), 7, dtype=torch.uint8, device=dev)
    rc = getattr(L, symbol)(*head, blob.data_ptr(), blob.numel(), out.data_ptr(), lat.data_ptr(), val.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, L.nlml_last_error()
    return out, lat, val
def same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))
def ws_pools():
    return [t.numel() for k, v in ops._k2_ws.items() if k[0] == "ws" for t in v]
if sys.argv[1] == "eligible":
    raw = torch.from_numpy(synth.raw_landmarks(B, seed=4)).to(dev)
    raw[B // 2] = 0.0
    want = plain("nlml_landmarks_to_pose", (raw.data_ptr(), B, 1), strict)
    o = ops.landmarks_to_pose(raw, strict, True, return_latent=True, return_valid=True)
    print("RESULT eligible", same(want, (o[0], o[1], o[2].to(torch.uint8))), [k[0] for k in ops._k2_ws], [len(v) for v in ops._k2_ws.values()], ws_pools())
else:
    feats = torch.from_numpy(synth.features(B, F, seed=12)).to(dev)
    feats[B // 2] = 0.0
    off = torch.zeros((B * F + 4,), dtype=torch.float32, device=dev)
    x_off = off[1:1 + B * F].view(B, F)                  # rows starting one float into an aligned buffer
    x_off.copy_(feats)
    pad = torch.zeros((B, F + 2), dtype=torch.float32, device=dev)
    x_pad = pad[:, :F]                                   # row stride F + 2
    x_pad.copy_(feats)
    fast = torch.from_numpy(weights.pack_blob(sd, heads, _lib.MODE_F16X2)).to(dev)
    assert off.data_ptr() %% 16 == 0 and x_off.data_ptr() %% 16 == 4 and x_pad.stride(0) == F + 2 and feats.data_ptr() %% 16 == 0
    for name, x, ld, blob in (("offset", x_off, F, strict), ("stride", x_pad, F + 2, strict), ("fast-blob", feats, F, fast)):
        want = plain("nlml_encoder_heads_fwd", (x.data_ptr(), ld, B, F), blob)
        o = ops.encoder_heads_fwd(x, blob, F, return_latent=True, return_valid=True)
        t = torch.ops.nlml_hpe.encoder_heads_fwd(x, blob, F)
        torch.cuda.synchronize()
        print("RESULT", name, same(want, (o[0], o[1], o[2].to(torch.uint8))), torch.equal(t.view(torch.uint8), want[0].view(torch.uint8)),
              [k[0] for k in ops._k2_ws])
"""


def _child_hosts(repo_root, which):
    env = {k: v for k, v in os.environ.items() if k not in ("NLML_K2_QUAD_MIN", "NLML_K2_QUAD_CUS", "NLML_K2_STREAMED_MIN")}
    env["NLML_K2_QUAD_CUS"] = "2"
    r = subprocess.run([sys.executable, "-c", _CHILD_HOSTS % {"root": repo_root}, which], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return [l.split(None, 2)[1:] for l in r.stdout.splitlines() if l.startswith("RESULT")]


@pytest.mark.gpu
def test_ops_takes_the_ws_form_with_the_quad_parts_workspace_for_eligible_rows(repo_root, device):
    """4,708 faces on a "two-unit device" (the mixed-launch test's split): ops.landmarks_to_pose on aligned raw rows pools exactly one
    workspace, under the "ws" form, of the quad part's 72 tiles, and computes the plain C call's bits."""
    (name, rest), = _child_hosts(repo_root, "eligible")
    assert name == "eligible" and rest == f"True ['ws'] [1] [{72 * 65536}]", rest


@pytest.mark.gpu
def test_hosts_make_the_plain_call_for_rows_and_blobs_the_rule_excludes(repo_root, device):
    """The same batch as feature rows one float into an aligned buffer, with row stride F + 2, and aligned with a fast-mode blob:
    ops.encoder_heads_fwd (pose, latent, mask) and torch.ops.nlml_hpe.encoder_heads_fwd (pose) equal nlml_encoder_heads_fwd on the same
    rows bit for bit, and ops pools no workspace."""
    got = _child_hosts(repo_root, "ineligible")
    assert [g[0] for g in got] == ["offset", "stride", "fast-blob"]
    for name, rest in got:
        assert rest == "True True []", f"{name}: {rest}"


@pytest.mark.gpu
def test_default_route_at_the_benchmark_size(blob, device):
    """65,536 faces: what bench.py times.  On a 256-unit device ops.landmarks_to_pose takes the four-tile kernel for the whole batch
    (one round); whatever the device, pose, latent and mask equal the plain C call's."""
    B = 65536
    g = torch.Generator(device=device).manual_seed(5)
    raw = torch.rand((B, 468, 3), generator=g, dtype=torch.float32, device=device)
    raw[12345] = 0.0
    rc, *want = _call("nlml_landmarks_to_pose", (raw.data_ptr(), B, 1), B, blob, device)
    assert rc == 0
    n = C.c_int64(0)
    assert _lib.lib().nlml_k2_quad_faces(B, C.byref(n), None) == 0
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    assert n.value == (B // 64) // (4 * cus) * cus * 256
    got = ops.landmarks_to_pose(raw, blob, True, return_latent=True, return_valid=True)
    _same((got[0], got[1], got[2].to(torch.uint8)), want, "ops.landmarks_to_pose at 65,536 faces")
    assert torch.equal(torch.ops.nlml_hpe.landmarks_to_pose(raw, blob, True), want[0])


# ---- 7. the split arithmetic, no GPU
def test_quad_split_arithmetic():
    L = _lib.lib()

    def split(B, cus):
        n = C.c_int64(-7)
        return L.nlml_k2_quad_split(B, cus, C.byref(n)), n.value

    for B, want in ((65535, 0), (65536, 65536), (65537, 65536), (131071, 65536), (131072, 131072), (0, 0)):
        assert split(B, 256) == (0, want), B
    assert split(255, 1) == (0, 0) and split(256, 1) == (0, 256) and split(700, 1) == (0, 512)     # one unit: every whole workgroup
    assert split(9000, 304) == (0, 0) and split(2 * 304 * 256 + 5, 304) == (0, 2 * 304 * 256)      # another unit count
    for cus in (0, -3):                                                                             # refused, and nothing handed out
        rc, n = split(70000, cus)
        assert rc == -1 and n == 0 and b"cus" in L.nlml_last_error()
    assert split(-1, 256)[0] == -1
    assert L.nlml_k2_quad_split(65536, 256, None) == -1
    for B in (1, 64, 65536, 65536 - 63, 10 ** 6):                                                   # the workspace function covers the hand-over
        assert L.nlml_encoder_heads_workspace_bytes(B, F_REF) >= (B + 63) // 64 * 65536
