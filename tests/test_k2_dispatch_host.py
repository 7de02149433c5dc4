"""The K2 dispatch rule as the hosts ask for it (nlml_k2_quad_part, nlml_k2_small_batch_max; csrc/abi.cpp), without a GPU: with
NLML_K2_QUAD_CUS set the library makes no HIP call, and the rows are looked at for their alignment only, so a made-up pointer stands in
for device memory.  The NLML_K2_* variables are read once per process: one child process per environment."""
import json
import os
import subprocess
import sys

import pytest

from nlml_hpe_amd import _lib

F_REF = 1404
FAKE = 4096          # an aligned "device" pointer; FAKE + 4 is the misaligned one
TILE_KB = 65536      # the hand-over of one 64-face tile
BADARG = -1

_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
from nlml_hpe_amd import _lib
L = _lib.lib()
res = []
for rows, ld, B, F, blob in json.loads(sys.argv[1]):
    blob_bytes = L.nlml_encoder_heads_packed_bytes(F, _lib.MODE_NAMES[blob]) if isinstance(blob, str) else \
        L.nlml_encoder_heads_packed_bytes(F, _lib.MODE_F16X2S) + blob
    n, need = C.c_int64(-7), C.c_size_t(7)
    rc = L.nlml_k2_quad_part(rows, ld, B, F, blob_bytes, C.byref(n), C.byref(need))
    err = L.nlml_last_error().decode() if rc else ""
    m, need_m = C.c_int64(-7), C.c_size_t(7)
    rc_m = L.nlml_k2_quad_faces(B, C.byref(m), C.byref(need_m))
    res.append([rc, n.value, need.value, err, rc_m, m.value, need_m.value])
# a NULL quad_faces: refused, the other output zeroed; a NULL ws_bytes is fine
need = C.c_size_t(7)
S = L.nlml_encoder_heads_packed_bytes(1404, _lib.MODE_F16X2S)
rc = L.nlml_k2_quad_part(4096, 1404, 4708, 1404, S, None, C.byref(need))
null_faces = [rc, need.value, L.nlml_last_error().decode()]
n = C.c_int64(-7)
null_bytes = [L.nlml_k2_quad_part(4096, 1404, 4708, 1404, S, C.byref(n), None), n.value]
print("RESULT", json.dumps({"rows": res, "null_faces": null_faces, "null_bytes": null_bytes}))
"""


def _child(repo_root, env_extra, rows):
    """rows: (rows, ld, B, F, blob) with blob a mode name or a number of bytes on top of the strict-fast blob's size.
    -> per row (rc, quad_faces, ws_bytes, error, and the same three of nlml_k2_quad_faces(B)), and the NULL-pointer calls."""
    env = {k: v for k, v in os.environ.items() if k not in ("NLML_K2_QUAD_MIN", "NLML_K2_QUAD_CUS", "NLML_K2_STREAMED_MIN")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": repo_root}, json.dumps(rows)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0].split(None, 1)[1])


def _check(got, want, what):
    """want: (rc, quad_faces, ws_bytes).  Where a quad part exists nlml_k2_quad_faces(B) gives the same pair."""
    assert tuple(got[:3]) == want, f"{what}: nlml_k2_quad_part gave {got[:3]}, expected {want}"
    if want[1] > 0:
        assert tuple(got[4:7]) == want, f"{what}: nlml_k2_quad_faces(B) gave {got[4:7]}, expected {want}"


def test_quad_part_on_a_two_unit_device(repo_root):
    """NLML_K2_QUAD_CUS=2: 4,708 faces = nine rounds of two 256-face workgroups + 100 (the split test_k2_quad.py's mixed-launch test
    pins on the GPU); the input-dependent half of the rule row by row; the refusals."""
    split = (0, 4608, 72 * TILE_KB)
    none = (0, 0, 0)
    cases = [
        ("whole rounds", (FAKE, F_REF, 4708, F_REF, "f16x2s"), split),
        ("the layer-per-launch sizes stay their own", (FAKE, F_REF, 4096, F_REF, "f16x2s"), none),
        ("misaligned rows", (FAKE + 4, F_REF, 4708, F_REF, "f16x2s"), none),
        ("ld % 4", (FAKE, 1406, 4708, F_REF, "f16x2s"), none),
        ("a padded stride is fine", (FAKE, 1408, 4708, F_REF, "f16x2s"), split),
        ("f32 blob", (FAKE, F_REF, 4708, F_REF, "f32"), none),
        ("bf16 blob", (FAKE, F_REF, 4708, F_REF, "bf16"), none),
        ("fast-mode blob", (FAKE, F_REF, 4708, F_REF, "f16x2"), none),
        ("no blob of width F", (FAKE, F_REF, 4708, F_REF, 16), none),
        ("one row, ld = F", (FAKE, F_REF, 1, F_REF, "f16x2s"), none),
        ("F % 4", (FAKE, 1406, 4708, 1406, "f16x2s"), none),
        ("B = -1", (FAKE, F_REF, -1, F_REF, "f16x2s"), (BADARG, 0, 0)),
        ("F = 0", (FAKE, F_REF, 4708, 0, 0), (BADARG, 0, 0)),
    ]
    r = _child(repo_root, {"NLML_K2_QUAD_CUS": "2"}, [c[1] for c in cases])
    for (what, _, want), got in zip(cases, r["rows"]):
        _check(got, want, what)
        if want[0]:
            assert "k2_quad_part" in got[3], f"{what}: the error does not name the function: {got[3]!r}"
    rc, need, err = r["null_faces"]
    assert rc == BADARG and need == 0 and "k2_quad_part" in err
    assert r["null_bytes"] == [0, 4608]


@pytest.mark.parametrize("env, row, want", [
    ({"NLML_K2_QUAD_CUS": "2", "NLML_K2_QUAD_MIN": "512"}, (FAKE, F_REF, 1061, F_REF, "f16x2s"), (0, 1061, 17 * TILE_KB)),
    ({"NLML_K2_QUAD_CUS": "1", "NLML_K2_QUAD_MIN": "-1"}, (FAKE, F_REF, 4708, F_REF, "f16x2s"), (0, 0, 0)),
    ({"NLML_K2_QUAD_CUS": "2", "NLML_K2_STREAMED_MIN": "4000"}, (FAKE, F_REF, 4708, F_REF, "f16x2s"), (0, 0, 0)),
], ids=["quad_min_512", "quad_min_negative", "streamed_min_wins"])
def test_quad_part_under_the_environment(repo_root, env, row, want):
    """NLML_K2_QUAD_MIN: from that size on the whole batch (17 tiles at 1,061 faces), negative = never; NLML_K2_STREAMED_MIN: the
    streamed path was asked for and wins.  The refusals do not depend on the environment."""
    r = _child(repo_root, env, [row, (FAKE, F_REF, -1, F_REF, "f16x2s"), (FAKE, F_REF, 4708, 0, 0)])
    _check(r["rows"][0], want, str(env))
    for got in r["rows"][1:]:
        assert tuple(got[:3]) == (BADARG, 0, 0) and "k2_quad_part" in got[3]
    rc, need, err = r["null_faces"]
    assert rc == BADARG and need == 0 and "k2_quad_part" in err


def test_small_batch_max_is_the_librarys():
    L = _lib.lib()
    assert L.nlml_k2_small_batch_max(_lib.MODE_F16X2) == 4096 and L.nlml_k2_small_batch_max(_lib.MODE_F16X2S) == 4096
    for mode in (_lib.MODE_F32, _lib.MODE_BF16, 7, -1):
        assert L.nlml_k2_small_batch_max(mode) == 0
    from nlml_hpe_amd.model import HIPPoseModel
    assert [HIPPoseModel.small_batch_max(m) for m in ("f16x2", "f16x2s", "f32", "bf16")] == [4096, 4096, 0, 0]
