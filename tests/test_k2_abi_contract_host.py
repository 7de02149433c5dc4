"""CPU: the argument contract of the K2 forward entry points (include/nlml_hpe.h, "K2 argument checks"), driven through ctypes.

Every case here is refused, or has B == 0 and returns 0: no kernel is launched, no buffer is read, so made-up addresses stand in for
device memory.  A host may match on which of two errors it gets, so the ORDER of the checks is part of the contract:
    (nlml_landmarks_to_pose_ws alone: null raw) -> the blob (negative B or bad F, null blob / out, its alignment, its size) -> the form's
    mode -> the null input -> B == 0 returns 0 -> the workspace (presence and size, then alignment) -> rows readable 16 bytes at a time.
The return code and the condition's wording are pinned; where two rungs share their wording only the code is.  What the _ws forms refuse
past the null input depends on the path the dispatcher picks, which depends on the NLML_K2_* variables (read once per process): those
cases run in a child process per environment."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nlml_hpe_amd import _lib

E_BADARG, E_BADBLOB = -1, -2
F_REF = 1404
FORMS = ("", "_small", "_streamed", "_quad", "_ws")
FORWARDS = [head + form for form in FORMS for head in ("nlml_encoder_heads_fwd", "nlml_landmarks_to_pose")]
DEBUG = "nlml_encoder_heads_fwd_debug"
# the explicit workspace forms: (what their messages call the path, the blob modes they take)
PATH = {"_small": ("small-batch path", ("f16x2", "f16x2s")), "_streamed": ("streamed-tail path", ("f16x2s",)),
        "_quad": ("quad path", ("f16x2s",))}
WITH_WS = [n for n in FORWARDS if n.endswith(tuple(PATH))]
WIDE = [n for n in FORWARDS if n.endswith(("_streamed", "_quad"))]          # rows must be readable 16 bytes at a time
AUTO = [n for n in FORWARDS if n.endswith("_ws")]

NEG_B, NULL_BUF, BLOB_ALIGN, BLOB_SIZE = "negative B or bad F", "null buffer", "blob must be 16-byte aligned", "blob size does not match"
WS_SMALL, WS_ALIGN, ROWS = "workspace too small", "workspace must be 16-byte aligned", "x must be 16-byte aligned with F and ldx multiples of 4"

# real memory behind every address handed over (nothing may read it, but nothing could fault on it either)
_mem = np.zeros(256, np.uint8)
_A16 = (_mem.ctypes.data + 15) & ~15
ADDR = {"a16": _A16, "a4": _A16 + 4, None: None}


def is_landmarks(name):
    return "landmarks" in name


def form_of(name):
    return next((f for f in FORMS[1:] if name.endswith(f)), "")


def null_input(name):
    return "landmarks_to_pose: null raw" if is_landmarks(name) else "encoder_heads: null x or ldx < F"


def ws_need(name, B, F=F_REF):
    """The bytes the form's own path needs: the layer-per-launch path's buffers, or 1 KiB per face of whole 64-face tiles."""
    if form_of(name) == "_small":
        return _lib.lib().nlml_encoder_heads_small_workspace_bytes(B, F)
    return (B + 63) // 64 * 65536


def call(name, B=5, F=F_REF, mode="f16x2s", blob_extra=0, rows="a16", ldx=None, blob="a16", out="a16", ws="a16", ws_bytes="enough",
         pre_tanh=None):
    """One call, every buffer at a 16-byte aligned address and the workspace large enough unless an argument says otherwise
    -> (rc, message).  Addresses are named ("a16", "a4", None) so that a case can travel to a child process as JSON.  The landmarks
    forms take no F and no ldx; ws_bytes: "enough", or a number."""
    L = _lib.lib()
    lm = is_landmarks(name)
    width = F_REF if lm else F
    blob_bytes = (L.nlml_encoder_heads_packed_bytes(width, _lib.MODE_NAMES[mode]) if width > 0 else 0) + blob_extra
    args = [ADDR[rows], B, 1] if lm else [ADDR[rows], F if ldx is None else ldx, B, F]
    args += [ADDR[blob], blob_bytes, ADDR[out], None]
    if name == DEBUG:
        args += [ADDR[pre_tanh], None]
    else:
        args.append(None)                         # valid
    if form_of(name):
        args += [ADDR[ws], L.nlml_encoder_heads_workspace_bytes(max(B, 0), width) if ws_bytes == "enough" else ws_bytes]
    args.append(None)                             # stream
    rc = getattr(L, name)(*args)
    return rc, L.nlml_last_error().decode()


def refused(name, code, wording, **kw):
    rc, msg = call(name, **kw)
    assert rc == code, (name, kw, rc, msg)
    if wording:
        assert wording in msg, (name, kw, msg)


# ---- rung by rung ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FORWARDS + [DEBUG])
def test_blob_checks_in_their_order(name):
    """negative B or bad F -> null blob / out -> the blob's alignment -> its size; all but the null buffers at B == 0 as well."""
    refused(name, E_BADARG, NEG_B, B=-1)
    if not is_landmarks(name):
        refused(name, E_BADARG, NEG_B, F=0)
        refused(name, E_BADARG, NEG_B, F=-4, B=0)
    refused(name, E_BADARG, NULL_BUF, blob=None)
    refused(name, E_BADARG, NULL_BUF, out=None)
    for B in (0, 5):
        refused(name, E_BADARG, BLOB_ALIGN, blob="a4", B=B)
        refused(name, E_BADBLOB, BLOB_SIZE, blob_extra=16, B=B)
    # two at once: the earlier one's message
    refused(name, E_BADARG, NEG_B, B=-1, blob=None, blob_extra=16)
    refused(name, E_BADARG, NULL_BUF, out=None, blob="a4")
    refused(name, E_BADARG, BLOB_ALIGN, blob="a4", blob_extra=16)


@pytest.mark.parametrize("name", FORWARDS + [DEBUG])
def test_the_blob_comes_before_the_null_input_except_in_landmarks_to_pose_ws(name):
    if name == "nlml_landmarks_to_pose_ws":
        refused(name, E_BADARG, null_input(name), rows=None, blob_extra=16)
        refused(name, E_BADARG, null_input(name), rows=None, blob=None)
        refused(name, E_BADARG, NEG_B, rows=None, B=-1)          # (no input is missing from an empty or negative batch)
    else:
        refused(name, E_BADBLOB, BLOB_SIZE, rows=None, blob_extra=16)
        refused(name, E_BADARG, NULL_BUF, rows=None, blob=None)
        refused(name, E_BADARG, BLOB_ALIGN, rows=None, blob="a4")


@pytest.mark.parametrize("name", WITH_WS)
def test_mode_restriction(name):
    """After the blob checks, before the null input and everything about the workspace; at B == 0 as well."""
    path, modes = PATH[form_of(name)]
    for mode in ("f32", "bf16", "f16x2", "f16x2s"):
        if mode in modes:
            continue
        for B in (0, 5):
            refused(name, E_BADARG, path + ": NLML_MODE_F16X2", mode=mode, B=B)
        refused(name, E_BADARG, path + ": NLML_MODE_F16X2", mode=mode, rows=None)
        refused(name, E_BADARG, path + ": NLML_MODE_F16X2", mode=mode, ws=None, ws_bytes=0)             # wrong-mode blob and no workspace
        refused(name, E_BADARG, path + ": NLML_MODE_F16X2", mode=mode, ws="a4", ws_bytes=16, rows="a4")
        refused(name, E_BADBLOB, BLOB_SIZE, mode=mode, blob_extra=16)                                   # the blob's size comes first


def test_debug_mode_restriction():
    for mode in ("bf16", "f16x2", "f16x2s"):
        for B in (0, 5):
            refused(DEBUG, E_BADARG, "debug build: f32 blob only", mode=mode, B=B)
        refused(DEBUG, E_BADARG, "debug build: f32 blob only", mode=mode, rows=None)
        refused(DEBUG, E_BADBLOB, BLOB_SIZE, mode=mode, blob_extra=16)


@pytest.mark.parametrize("name", FORWARDS + [DEBUG])
def test_null_input(name):
    """Before B == 0 would matter (it is no error there) and before the workspace."""
    mode = "f32" if name == DEBUG else "f16x2s"
    refused(name, E_BADARG, null_input(name), rows=None, mode=mode)
    if not is_landmarks(name):
        refused(name, E_BADARG, null_input(name), ldx=1403, mode=mode)
        refused(name, E_BADARG, null_input(name), ldx=0, mode=mode)
    if form_of(name):
        refused(name, E_BADARG, null_input(name), rows=None, ws=None, ws_bytes=0)
        refused(name, E_BADARG, null_input(name), rows=None, ws="a4", ws_bytes=16)


@pytest.mark.parametrize("name", FORWARDS + [DEBUG])
def test_b_zero_needs_no_input_and_no_workspace(name):
    """B == 0 with a blob that passes: 0, whatever input, output, workspace and alignment are -- there is no launch."""
    modes = ("f32",) if name == DEBUG else PATH[form_of(name)][1] if form_of(name) in PATH else ("f32", "bf16", "f16x2", "f16x2s")
    for mode in modes:
        assert call(name, B=0, mode=mode)[0] == 0
        assert call(name, B=0, mode=mode, rows=None, out=None, ws=None, ws_bytes=0)[0] == 0
        assert call(name, B=0, mode=mode, rows="a4", ws="a4", ws_bytes=1)[0] == 0
        assert call(name, B=0, mode=mode, blob=None)[0] == 0                  # (a NULL blob is 16-byte aligned and B == 0 needs none)
        if not is_landmarks(name):
            assert call(name, B=0, mode=mode, ldx=3)[0] == 0
            assert call(name, B=0, mode=mode, F=1406, ldx=1406)[0] == 0
    if name == DEBUG:
        assert call(name, B=0, mode="f32", rows="a4", pre_tanh="a16")[0] == 0


@pytest.mark.parametrize("name", WITH_WS)
def test_workspace_presence_and_size_then_alignment(name):
    path, modes = PATH[form_of(name)]
    for mode in modes:
        for B in (1, 5, 64, 65):
            need = ws_need(name, B)
            assert need > 0
            refused(name, E_BADARG, path + ": " + WS_SMALL, mode=mode, B=B, ws=None, ws_bytes=0)
            refused(name, E_BADARG, path + ": " + WS_SMALL, mode=mode, B=B, ws=None)                    # the bytes without the buffer
            refused(name, E_BADARG, path + ": " + WS_SMALL, mode=mode, B=B, ws_bytes=need - 1)
            refused(name, E_BADARG, path + ": " + WS_SMALL, mode=mode, B=B, ws_bytes=0)
            refused(name, E_BADARG, path + ": " + WS_SMALL, mode=mode, B=B, ws="a4", ws_bytes=need - 1)  # short and misaligned
            refused(name, E_BADARG, path + ": " + WS_ALIGN, mode=mode, B=B, ws="a4", ws_bytes=need)
            refused(name, E_BADARG, path + ": " + WS_ALIGN, mode=mode, B=B, ws="a4")


@pytest.mark.parametrize("name", WIDE)
def test_rows_readable_16_bytes_at_a_time(name):
    """The streamed and the quad forms, last of all: after a short and after a misaligned workspace."""
    path = PATH[form_of(name)][0]
    bad_rows = [dict(rows="a4")]
    if not is_landmarks(name):
        bad_rows += [dict(ldx=1405), dict(ldx=1406), dict(F=1406, ldx=1408), dict(F=1406, ldx=1406)]
    for kw in bad_rows:
        refused(name, E_BADARG, path + ": " + ROWS, **kw)
        refused(name, E_BADARG, path + ": " + WS_SMALL, ws_bytes=ws_need(name, 5) - 1, **kw)          # misaligned rows and short workspace
        refused(name, E_BADARG, path + ": " + WS_SMALL, ws=None, **kw)
        refused(name, E_BADARG, path + ": " + WS_ALIGN, ws="a4", **kw)


def test_debug_rows():
    """The debug kernel exists for aligned feature rows with F % 4 == 0 only: refused once there is something to write (and B > 0)."""
    what = "debug build: features input, F % 4 == 0 only"
    refused(DEBUG, E_BADARG, what, mode="f32", rows="a4", pre_tanh="a16")
    refused(DEBUG, E_BADARG, what, mode="f32", ldx=1406, pre_tanh="a16")
    refused(DEBUG, E_BADARG, what, mode="f32", F=1406, ldx=1408, pre_tanh="a16")
    refused(DEBUG, E_BADARG, null_input(DEBUG), mode="f32", rows=None, pre_tanh="a16")


# ---- the _ws forms past the null input: whatever path the dispatcher picks refuses in its own words -----------------------------

_CHILD = r"""
import json, sys
sys.path[:0] = [%(root)r, %(tests)r]
from test_k2_abi_contract_host import call
print("RESULT", json.dumps([call(name, **kw) for name, kw in json.loads(sys.argv[1])]))
"""


def _child(repo_root, env_extra, cases):
    env = {k: v for k, v in os.environ.items() if k not in ("NLML_K2_QUAD_MIN", "NLML_K2_QUAD_CUS", "NLML_K2_STREAMED_MIN")}
    env.update(env_extra)
    src = _CHILD % {"root": repo_root, "tests": os.path.join(repo_root, "tests")}
    r = subprocess.run([sys.executable, "-c", src, json.dumps(cases)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][0].split(None, 1)[1])


def _check_child(repo_root, env, cases):
    """cases: (name, kwargs, rc, wording)"""
    got = _child(repo_root, env, [c[:2] for c in cases])
    for (name, kw, rc, wording), (got_rc, msg) in zip(cases, got):
        assert got_rc == rc, (env, name, kw, got_rc, msg)
        if wording:
            assert wording in msg, (env, name, kw, msg)


def test_ws_forms_small_batches_meet_the_small_paths_refusals(repo_root):
    """A split-f16 batch of up to nlml_k2_small_batch_max faces goes to the layer-per-launch path, whose refusals the caller then gets;
    that path reads rows of any alignment, so rows are no reason of its own."""
    cases = []
    for name in AUTO:
        for mode in ("f16x2", "f16x2s"):
            for B in (5, 4096):
                need = _lib.lib().nlml_encoder_heads_small_workspace_bytes(B, F_REF)
                cases += [
                    (name, dict(mode=mode, B=B, ws=None, ws_bytes=0), E_BADARG, "small-batch path: " + WS_SMALL),
                    (name, dict(mode=mode, B=B, ws_bytes=need - 1), E_BADARG, "small-batch path: " + WS_SMALL),
                    (name, dict(mode=mode, B=B, ws="a4", ws_bytes=need - 1), E_BADARG, "small-batch path: " + WS_SMALL),
                    (name, dict(mode=mode, B=B, ws="a4"), E_BADARG, "small-batch path: " + WS_ALIGN),
                    (name, dict(mode=mode, B=B, ws=None, rows="a4"), E_BADARG, "small-batch path: " + WS_SMALL),
                    (name, dict(mode=mode, B=B, rows=None, ws=None), E_BADARG, null_input(name)),
                ]
        cases += [(name, dict(B=0, ws=None, ws_bytes=0, mode=m), 0, None) for m in ("f32", "bf16", "f16x2", "f16x2s")]
    _check_child(repo_root, {"NLML_K2_QUAD_CUS": "2"}, cases)


def test_ws_forms_quad_refusals_through_quad_min(repo_root):
    """NLML_K2_QUAD_MIN=512: a strict-fast batch from 512 faces on with rows readable 16 bytes at a time goes through the four-tile
    kernel WHOLE, and then a small workspace is refused (without the variable the call would fall back to the other paths).  Rows that
    are not so readable never reach the quad path: up to 4,096 faces the layer-per-launch path's refusals answer instead."""
    B = 1061
    quad_need = (B + 63) // 64 * 65536
    cases = []
    for name in AUTO:
        cases += [
            (name, dict(B=B, ws=None, ws_bytes=0), E_BADARG, "quad path: " + WS_SMALL),
            (name, dict(B=B, ws_bytes=quad_need - 1), E_BADARG, "quad path: " + WS_SMALL),
            (name, dict(B=B, ws="a4", ws_bytes=quad_need - 1), E_BADARG, "quad path: " + WS_SMALL),
            (name, dict(B=B, ws="a4", ws_bytes=quad_need), E_BADARG, "quad path: " + WS_ALIGN),
            (name, dict(B=B, ws="a4"), E_BADARG, "quad path: " + WS_ALIGN),
            (name, dict(B=B, rows="a4", ws=None), E_BADARG, "small-batch path: " + WS_SMALL),
            (name, dict(B=B, rows="a4", ws="a4"), E_BADARG, "small-batch path: " + WS_ALIGN),
            (name, dict(B=511, ws=None), E_BADARG, "small-batch path: " + WS_SMALL),                   # below the variable's size
            (name, dict(B=B, mode="f16x2", ws=None), E_BADARG, "small-batch path: " + WS_SMALL),       # no strict-fast blob
            (name, dict(B=B, rows=None, ws=None), E_BADARG, null_input(name)),
            (name, dict(B=0, ws=None, ws_bytes=0), 0, None),
        ]
        if not is_landmarks(name):
            cases += [(name, dict(B=B, ldx=1406, ws=None), E_BADARG, "small-batch path: " + WS_SMALL),
                      (name, dict(B=B, F=1406, ldx=1408, ws=None), E_BADARG, "small-batch path: " + WS_SMALL)]
    # the explicit quad forms do not depend on the variable
    for name in ("nlml_encoder_heads_fwd_quad", "nlml_landmarks_to_pose_quad"):
        cases += [(name, dict(B=100, ws=None), E_BADARG, "quad path: " + WS_SMALL),
                  (name, dict(B=100, rows="a4"), E_BADARG, "quad path: " + ROWS)]
    _check_child(repo_root, {"NLML_K2_QUAD_CUS": "2", "NLML_K2_QUAD_MIN": "512"}, cases)


def test_ws_forms_streamed_refusals_through_streamed_min(repo_root):
    """NLML_K2_STREAMED_MIN=5000: strict-fast batches from that size on with rows readable 16 bytes at a time go through the streamed
    path (it wins over the quad path), whose refusals the caller then gets."""
    B = 6000
    need = (B + 63) // 64 * 65536
    cases = []
    for name in AUTO:
        cases += [
            (name, dict(B=B, ws=None, ws_bytes=0), E_BADARG, "streamed-tail path: " + WS_SMALL),
            (name, dict(B=B, ws_bytes=need - 1), E_BADARG, "streamed-tail path: " + WS_SMALL),
            (name, dict(B=B, ws="a4", ws_bytes=need - 1), E_BADARG, "streamed-tail path: " + WS_SMALL),
            (name, dict(B=B, ws="a4"), E_BADARG, "streamed-tail path: " + WS_ALIGN),
            (name, dict(B=B, rows=None, ws=None), E_BADARG, null_input(name)),
            (name, dict(B=0, ws=None, ws_bytes=0), 0, None),
        ]
    _check_child(repo_root, {"NLML_K2_QUAD_CUS": "2", "NLML_K2_STREAMED_MIN": "5000"}, cases)
