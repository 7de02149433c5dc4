"""CPU: the packed blob's header and the two workspace sizes against a restatement of the K2 layout written out here.

The library computes the layout once (nlml_hpe_amd/csrc/layout.h: the packer fills the header from it, the split-f16 kernels compute
their offsets from it instead of reading the header); this file states it a second time, from stage tables typed in below, so that an
edit to the one definition that moves a weight, a bias or a buffer shows up on the host, in all four modes."""
import numpy as np
import pytest

from nlml_hpe_amd import _lib, synth, weights

# (neuron blocks per job, jobs, K steps; layer 0's K steps depend on F) for E0..E5, H0..H4
STAGES_F32 = [(4, 8, None), (4, 4, 128), (2, 4, 64), (1, 4, 32), (1, 2, 16), (1, 1, 8),
              (1, 12, 1), (2, 12, 16), (1, 12, 32), (1, 6, 16), (1, 3, 8)]
STAGES_BF16 = [(8, 4, None), (4, 4, 64), (2, 4, 32), (1, 4, 16), (1, 2, 8), (2, 1, 4),
               (1, 12, 1), (2, 12, 8), (1, 12, 16), (1, 6, 8), (1, 3, 4)]
STAGES_F16X2 = [(4, 8, None), (4, 4, 64), (2, 4, 32), (1, 4, 16), (1, 2, 8), (2, 1, 4),
                (1, 12, 1), (2, 12, 8), (1, 12, 16), (1, 6, 8), (1, 3, 4)]
# mode name -> (stage table, 16-byte pieces per weight fragment, K steps of layer 0 for F)
FAMILIES = {
    "f32": (STAGES_F32, 1, lambda F: -(-F // 64) * 8),
    "bf16": (STAGES_BF16, 1, lambda F: -(-F // 128) * 8),
    "f16x2": (STAGES_F16X2, 2, lambda F: -(-F // 64) * 4),
}
FS = [10, 13, 64, 65, 136, 1404, 1407]


def _restated(mode, F):
    """k of layer 0, total units, and per stage (w_off, b_off, job_w16), all in 16-byte units; the f32 image not counted."""
    stages, pieces, k_e0 = FAMILIES["f16x2" if mode == "f16x2s" else mode]
    units, w_off, b_off, job_w16 = 16, [], [], []                  # the header
    for nb, jobs, k in stages:
        k = k_e0(F) if k is None else k
        job = k * nb * 64 * pieces
        w_off.append(units)
        b_off.append(units + jobs * job)
        job_w16.append(job)
        units += jobs * (job + nb * 8)
    return k_e0(F), units + 4096, w_off, b_off, job_w16           # the tail pad


@pytest.fixture(scope="module")
def state_dicts(head_sds):
    return {F: synth.encoder_state_dict(F, seed=0) for F in FS}, head_sds


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16x2", "f16x2s"])
def test_blob_header_is_the_restated_layout(mode, F, state_dicts):
    sds, head_sds = state_dicts
    m = _lib.mode_from_name(mode)
    blob = weights.pack_blob(sds[F], head_sds, m)
    k_e0, total, w_off, b_off, job_w16 = _restated(mode, F)
    if mode == "f16x2s":                                            # + 256 bytes + a complete f32 image
        total += 16 + _restated("f32", F)[1]
    assert blob.nbytes == total * 16
    assert _lib.lib().nlml_encoder_heads_packed_bytes(F, m) == total * 16
    hdr = blob.view(np.uint32)[:64]
    assert hdr[2] == F and hdr[3] == m
    assert hdr[4] == k_e0 and hdr[5] == total
    assert hdr[6:17].tolist() == w_off
    assert hdr[17:28].tolist() == b_off
    assert hdr[28:39].tolist() == job_w16
    if mode == "f16x2s":                                            # the f32 image behind it carries its own header
        off = (_restated("f16x2", F)[1] + 16) * 16
        k32, total32, w32, b32, j32 = _restated("f32", F)
        h32 = blob[off:off + 256].view(np.uint32)
        assert h32[3] == _lib.MODE_F32 and h32[4] == k32 and h32[5] == total32
        assert h32[6:17].tolist() == w32 and h32[17:28].tolist() == b32 and h32[28:39].tolist() == j32


@pytest.mark.parametrize("F", [13, 136, 1404])
@pytest.mark.parametrize("B", [0, 1, 64, 65, 4096, 4133, 65536])
def test_workspace_sizes_are_the_restated_buffers(B, F):
    L = _lib.lib()
    tiles = -(-B // 64)
    k16 = -(-F // 64) * 4
    small = 2 * tiles * max(k16, 64) * 4096                        # two buffers of [tile][K16 step] x 4 KiB
    assert L.nlml_encoder_heads_small_workspace_bytes(B, F) == small
    assert L.nlml_encoder_heads_workspace_bytes(B, F) == max(small, tiles * 65536)   # the streamed hand-over: 1 KiB per face of whole tiles


def test_workspace_sizes_of_an_empty_call_are_zero():
    L = _lib.lib()
    for B, F in ((0, 1404), (-1, 1404), (64, 0), (64, -5)):
        assert L.nlml_encoder_heads_small_workspace_bytes(B, F) == 0
        assert L.nlml_encoder_heads_workspace_bytes(B, F) == 0
