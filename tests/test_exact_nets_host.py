"""CPU tests of the exactly summable networks (tests/exact_nets.py) and of the bf16 blob: the certificate means what it says, the host
packer's bf16 image walked with the kernel's index arithmetic gives the model's bits, and the padded K region holds zeros."""
import numpy as np
import pytest

import blob_emulator as BE
import exact_nets as XN
from nlml_hpe_amd import _lib, synth, weights
from oracle import encoder_heads as EH
from oracle import feature_norm as FN

FORMS = ["saturated", "live"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("F", [1404, 136, 13])
def test_bf16_blob_walk_is_bit_exact_on_exact_nets(F, form):
    """pack.cpp's bf16 image, decoded as the kernel decodes it (job offsets, [k16 step][block][lane] x 8 fragments, bias in accumulator
    order, E5 as two blocks with latent 3g+c on row 16g+c, H0's K padded to 16), summed in f64 and rounded where the kernel rounds
    == oracle.encoder_heads.forward_bf16_emulated on the certified faces: pose and latent, every bit."""
    p = XN.pool(F, form)
    blob = weights.pack_blob(p["enc"], p["heads"], _lib.MODE_BF16)
    assert blob.nbytes == _lib.lib().nlml_encoder_heads_packed_bytes(F, _lib.MODE_BF16)
    out, lat = BE.forward_bf16(blob, p["x"])
    assert np.array_equal(_bits(out), _bits(p["pose"])) and np.array_equal(out, p["pose"].astype(np.float64))
    assert np.array_equal(_bits(lat), _bits(p["latent"])) and np.array_equal(lat, p["latent"].astype(np.float64))
    assert len(np.unique(p["pose"], axis=0)) >= 0.9 * len(p["x"]), "the faces must tell each other apart"


@pytest.mark.parametrize("F", [1404, 136, 13])
def test_bf16_blob_walk_matches_the_model_on_dense_random_weights(F, head_sds):
    sd = synth.encoder_state_dict(F, seed=0)
    blob = weights.pack_blob(sd, head_sds, _lib.MODE_BF16)
    x = synth.features(40, F, seed=5)
    out, lat = BE.forward_bf16(blob, x)
    emu, emu_lat = EH.forward_bf16_emulated(x, EH.Params(sd, head_sds))
    assert np.abs(lat - emu_lat).max() <= 2e-3          # the bar of test_bf16_throughput_mode; both sum in f64, so far inside it
    assert np.degrees(np.abs(out - emu).max()) <= 0.25


@pytest.mark.parametrize("F", [1404, 1407, 136, 16, 13])
def test_bf16_blob_padded_k_and_unused_rows_hold_zeros(F):
    """The kernel's K loops run over the padded K (E0: whole pairs of 64-column slabs, H0: 16) and its `kc` clamp re-reads real columns
    of x there, so the weights of k >= K must be zero; rows that carry no neuron (E5 beyond 16g+c, H4 beyond row 0) hold zero weights
    AND zero bias, because the heads read them as K padding."""
    p = XN.pool(F, "saturated")
    enc = {k: (np.where(v == 0, np.float32(3.0), v) if k.endswith("weight") else v) for k, v in p["enc"].items()}   # no zero weight left
    heads = {n: {k: (np.where(v == 0, np.float32(3.0), v) if k.endswith("weight") else v + np.float32(5.0)) for k, v in sd.items()}
             for n, sd in p["heads"].items()}
    enc["encoder.10.bias"] = enc["encoder.10.bias"] + np.float32(5.0)
    blob = weights.pack_blob(enc, heads, _lib.MODE_BF16)
    hdr = BE._header(blob)
    k16 = hdr["k8_e0"]
    assert k16 % 8 == 0 and 16 * k16 >= F and 16 * k16 - F < 128
    for job in range(4):
        A, _ = BE.bf16_job_matrix(blob, hdr, 0, job, k16, 8)
        assert (A[:, :F] != 0).all() and not A[:, F:].any()
    A, b = BE.bf16_job_matrix(blob, hdr, 5, 0, 4, 2)
    real = np.array([16 * g + c for g in range(3) for c in range(3)])
    pad = np.setdiff1d(np.arange(64), real)
    assert (A[real] != 0).all() and (b[real] != 0).all() and not A[pad].any() and not b[pad].any()
    for job in range(12):
        A, _ = BE.bf16_job_matrix(blob, hdr, 6, job, 1, 1)
        assert (A[:, :3] != 0).all() and not A[:, 3:].any()
    for g in range(3):
        A, b = BE.bf16_job_matrix(blob, hdr, 10, g, 4, 1)
        assert (A[0] != 0).all() and b[0] != 0 and not A[1:].any() and not b[1:].any()
    tail = blob[(int(hdr["b_off"][10]) + 3 * 8) * 16:]
    assert tail.nbytes >= 65536 and not tail.any(), "the prefetch pad behind the last job"


def _f32_chain(a, w, b, reverse):
    """bias + sum over k in f32, one product at a time, k ascending or descending."""
    acc = np.broadcast_to(b.astype(np.float32)[None, :], (a.shape[0], w.shape[0])).copy()
    a32, w32 = a.astype(np.float32), w.astype(np.float32)
    ks = range(a.shape[1] - 1, -1, -1) if reverse else range(a.shape[1])
    for k in ks:
        acc += a32[:, k, None] * w32[None, :, k]
    return acc


@pytest.mark.parametrize("form,rounded", [("saturated", True), ("live", True), ("saturated", False)])
def test_certificate_means_every_f32_order_is_exact(form, rounded):
    """On certified faces an f32 accumulation equals the f64 value bit for bit at each of the 21 stages, whatever the order: a chain
    with k ascending, a chain with k descending, and the BLAS order of an f32 matrix product."""
    p = XN.pool(1404, form, rounded)
    x = p["x"][:24]
    ok, _, stages = XN.certify(x, p["enc"], p["heads"], rounded, return_stages=True)
    assert ok.all() and len(stages) == 21
    for st in stages:
        z = st["z"]
        z32 = z.astype(np.float32)
        assert np.array_equal(z32.astype(np.float64), z), st["name"]
        for got in (_f32_chain(st["a"], st["w"], st["b"], False), _f32_chain(st["a"], st["w"], st["b"], True),
                    st["a"].astype(np.float32) @ st["w"].astype(np.float32).T + st["b"].astype(np.float32)):
            assert np.array_equal(_bits(got), _bits(z32)), st["name"]
    # the walk the certificate is computed on IS the model the kernels are compared with
    pose, lat, _ = XN.reference(x, p["enc"], p["heads"], rounded)
    assert np.array_equal(lat.astype(np.float64), stages[5]["z"])
    assert np.array_equal(pose.astype(np.float64), np.concatenate([stages[10]["z"], stages[15]["z"], stages[20]["z"]], axis=1))


def test_certified_unrounded_nets_are_exact_end_to_end_in_f32_and_in_the_c_oracle():
    """Saturated Tanh, f32 activations (what the f32 and split-f16 modes keep): numpy's f32 forward and the C oracle's three fmaf-chain
    orders give the f64 answer bit for bit -- pose, latent and the pre-Tanh activations."""
    from oracle import c_oracle as CO
    p = XN.pool(1404, "saturated", rounded=False)
    x, P = p["x"][:64], EH.Params(p["enc"], p["heads"])
    assert np.array_equal(_bits(EH.forward_numpy(x, P, np.float32)), _bits(p["pose"][:64]))
    assert np.array_equal(_bits(EH.encoder_latent_numpy(x, P, np.float32)), _bits(p["latent"][:64]))
    pre = XN._walk(x, p["enc"], p["heads"], False, upto=5)[4]["z"]
    for order in (0, 1, 2):
        out, lat, pre_c = CO.encoder_heads(x, P, order=order, want_latent=True, want_pre_tanh=True)
        assert np.array_equal(_bits(out), _bits(p["pose"][:64])) and np.array_equal(_bits(lat), _bits(p["latent"][:64])), order
        assert np.array_equal(pre_c.astype(np.float64), pre), order


def test_an_over_dense_net_is_refused():
    """Dense +-1 rows in E2, E3 and E4 sum hundreds of activations of 1e4 .. 1e5 against a bias quantum of 1: beyond 2^20 q from E3
    on (measured: 21.1 bits at E3, 23.7 at E4).  certify() must say so for every face but the all-zero one."""
    enc, heads, x = XN.make(1404, 3, "saturated", B=48, nnz={"E2": None, "E3": None, "E4": None})
    ok, worst = XN.certify(x, enc, heads)
    assert ok[0] and not ok[1:].any()
    wb = XN.worst_bits(worst)
    assert wb["E3"] > 20 and wb["E4"] > 20 and max(wb[k] for k in ("E0", "E1", "E2")) < 20
    # with the default density the same seed passes
    enc2, heads2, x2 = XN.make(1404, 3, "saturated", B=48)
    assert XN.certify(x2, enc2, heads2)[0].all()
    # and a bound of 2^12 refuses the default net too: the answer depends on `bits`, not on the net alone
    assert not XN.certify(x2, enc2, heads2, bits=12)[0][1:].any()


@pytest.mark.parametrize("F", [1404, 136, 64, 16, 13, 1407])
def test_live_form_leaves_out_at_most_15_percent(F):
    """Faces left out of the live-Tanh comparison (certificate missed, or a Tanh output within the margin of a bf16 tie) with the
    seeds the GPU tests use; the margin is derived in tests/exact_nets.py from the device's measured tanhf error."""
    assert XN.LIVE_TIE_MARGIN_ULPS >= 8 * XN.TANHF_MEASURED_ULPS and np.log2(XN.LIVE_TIE_MARGIN_ULPS) % 1 == 0
    p = XN.pool(F, "live")
    assert p["excluded"] <= XN.MAX_EXCLUDED_SHARE, p["excluded"]
    z = XN.e4_preactivations(p["x"], p["enc"], p["heads"])
    assert 0.5 <= np.abs(z).max() <= 2.0 and len(np.unique(z)) > 100, "the Tanh is live: neither saturated nor linear"
    assert XN.pool(F, "saturated")["excluded"] == 0.0


def test_tie_distance():
    one_ulp = 2.0 ** -23                                   # f32 ulp in [1, 2); bf16 values there are k * 2^-7, ties at odd multiples of 2^-8
    t = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 3 * one_ulp, 1.0 + 2.0 ** -7, 0.0, -(0.5 + 2.0 ** -9 - 2.0 ** -24)])
    assert np.array_equal(XN.tie_distance_ulps(t), [2.0 ** 15, 0.0, 3.0, 2.0 ** 15, np.inf, 1.0])


def test_raw_landmarks_normalise_to_the_certified_integers():
    """The fused path's input: coordinates in eighths, IPD a power of two, so the f64 subtract and divide of the normalisation are
    exact and the features are the integers the certificate was computed on; the all-zero face is the "no face" row."""
    from oracle import c_oracle as CO
    p = XN.pool(1404, "saturated")
    raw = XN.raw_landmarks(p["x"], seed=11)
    assert np.array_equal(raw * 8, np.round(raw * 8)) and not raw[0].any() and raw[1:].any(axis=(1, 2)).all()
    d = raw[:, 33].astype(np.float64) - raw[:, 263].astype(np.float64)
    ipd = np.sqrt((d * d).sum(axis=1))[1:]
    assert np.array_equal(np.log2(ipd), np.round(np.log2(ipd))) and len(np.unique(ipd)) == 5
    for feats in (FN.normalize_ipd(raw, True), CO.normalize_ipd(raw, True)):
        assert np.array_equal(feats, p["x"])
    assert np.array_equal(~FN.no_face_mask(FN.normalize_ipd(raw, True)), p["valid"]) and not p["valid"][0] and p["valid"][1:].all()
    # un-normalised: the raw coordinates themselves are the features; they certify too (quantum 1/8)
    flat = raw.reshape(len(raw), 1404)
    assert XN.certify(flat, p["enc"], p["heads"])[0].mean() >= 0.9


# ---- networks with live lo pieces (the split-f16 modes) -----------------------------------------------------------------------------
MIN_KEPT = 128
MIN_COVER = 0.10
WIDTHS = [1404, 136, 64, 16, 13, 1407]
LAYER0_POOLS = ("E0w", "E0x", "E0wx")
SPLIT_CASES = [(n, 1404) for n in sorted(XN.SPLIT_POOLS)] + [(n, F) for n in LAYER0_POOLS for F in WIDTHS[1:]]


@pytest.mark.parametrize("name,F", SPLIT_CASES)
def test_split_pool_conditions(name, F):
    """At most 15 % of the candidates left out, at least 128 faces kept, row 0 the all-zero "no face" row.  Pool E0wx: at least 10 %
    of the certified E0 accumulators receive a non-zero product of EACH of the three kinds, a_lo w_lo is live there and the model's
    bits differ from the f64 forward's.  The other pools: a_hi w_lo at every bumped stage (E0x: a_lo w_hi at E0); their a_lo w_hi
    lies behind the bump, because a hidden stage with both lo pieces does not certify (tests/exact_nets.py has the measurement), and
    test_split_pools_together_cover_every_stage_kind asserts the sum over the pools."""
    p = XN.split_pool(name, F)
    assert p["excluded"] <= XN.MAX_EXCLUDED_SHARE and len(p["x"]) >= MIN_KEPT, (p["excluded"], len(p["x"]))
    assert not p["x"][0].any() and not p["valid"][0] and p["valid"][1:].all()
    assert max(p["bits"].values()) < 20
    for st in p["bump"]:
        assert p["cover"][st]["hi_lo"] >= MIN_COVER and p["cover"][st]["hi_hi"] >= MIN_COVER, (st, p["cover"][st])
    if name == "E0wx":
        assert min(p["cover"]["E0"].values()) >= MIN_COVER, p["cover"]["E0"]
        assert not XN.lo_lo_is_zero(XN._split_walk(p["x"], p["enc"], p["heads"])[:1], np.ones(len(p["x"]), bool))
        f64 = EH.encoder_latent_numpy(p["x"], EH.Params(p["enc"], p["heads"]), np.float64)
        differ = (f64 != p["latent"].astype(np.float64)).any(axis=1)
        assert differ.sum() >= 8, "the dropped a_lo w_lo must show in the answer"
        print(f"{name} F={F}: {differ.sum()} faces whose latent is not the f64 forward's")
    elif name == "E0x":
        assert p["cover"]["E0"]["lo_hi"] >= MIN_COVER and np.any(p["x"] * 2.0 ** 10 % 1 != 0)
    else:
        assert np.array_equal(p["x"], np.round(p["x"]))
    assert len(np.unique(p["pose"], axis=0)) >= 0.9 * len(p["x"]), "the faces must tell each other apart"
    print(f"{name} F={F}: kept {len(p['x'])} of {p['n_all']}, excluded {p['excluded']:.3f}, worst bits {max(p['bits'].values()):.1f}, "
          + ", ".join(f"{st} lo_hi {c['lo_hi']:.2f} hi_lo {c['hi_lo']:.2f}" for st, c in p["cover"].items()))


def test_split_pools_together_cover_every_stage_kind():
    """Non-zero w_lo AND non-zero a_lo products under each of the eleven stage kinds, on >= 10 % of the accumulators of some pool.
    The one exception is a_lo under E5: its input is the saturated Tanh (-1, 0, 1), whose lo piece is identically zero."""
    pools = [XN.split_pool(n) for n in sorted(XN.SPLIT_POOLS)]
    for st in ("E0", "E1", "E2", "E3", "E4", "E5", "H0", "H1", "H2", "H3", "H4"):
        assert max(p["cover"][st]["hi_lo"] for p in pools) >= MIN_COVER, st
        if st == "E5":
            assert all(p["cover"][st]["lo_hi"] == 0.0 for p in pools)
        else:
            assert max(p["cover"][st]["lo_hi"] for p in pools) >= MIN_COVER, st


@pytest.mark.parametrize("name,F", SPLIT_CASES)
def test_reference_split_is_the_blob_walk_bit_for_bit(name, F):
    """The dense piece model on the state dicts == pack.cpp's split-f16 image walked with the kernel's index arithmetic
    (blob_emulator.forward_f16x2), pose and latent, every bit, on ALL certified faces of every pool and width the GPU tests run: ties
    the packer (scale, hi/lo planes, fragment order, the padded K tail) to the model the GPU tests compare with.  The f16x2 blob is the
    strict-fast blob's split image byte for byte (the header's mode and size apart), so one walk covers both."""
    p = XN.split_pool(name, F)
    blob = weights.pack_blob(p["enc"], p["heads"], _lib.MODE_F16X2S)
    fast = weights.pack_blob(p["enc"], p["heads"], _lib.MODE_F16X2)
    for b, mode in ((blob, _lib.MODE_F16X2S), (fast, _lib.MODE_F16X2)):
        assert b.nbytes == _lib.lib().nlml_encoder_heads_packed_bytes(F, mode)
    assert np.array_equal(fast[256:], blob[256:fast.nbytes])
    differ = np.flatnonzero(fast[:256].view(np.uint32) != blob[:256].view(np.uint32))
    assert differ.tolist() == [3, 5], "header words: mode and total size"
    out, lat = BE.forward_f16x2(blob, p["x"])
    assert np.array_equal(out, p["pose"].astype(np.float64)) and np.array_equal(lat, p["latent"].astype(np.float64))
    hdr = BE._header(blob)
    stages = XN._split_walk(p["x"][:2], p["enc"], p["heads"])
    assert np.array_equal(hdr["inv_scale"], [1.0 / stages[i]["s"] for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)])


def test_rescue_pool_is_the_blob_walk_on_its_unrescued_faces():
    p = XN.rescue_pool()
    calm = ~p["rescued"]
    out, lat = BE.forward_f16x2(weights.pack_blob(p["enc"], p["heads"], _lib.MODE_F16X2S), p["x"][calm])
    assert np.array_equal(out, p["pose"][calm].astype(np.float64)) and np.array_equal(lat, p["latent"][calm].astype(np.float64))


def test_reference_split_is_the_f64_forward_where_lo_lo_is_zero():
    """The model drops a_lo w_lo and nothing else: where no accumulator has such a product (integer x under a bumped E0, +-1 weights
    behind it; the old all-integer pool) it equals the plain f64 forward; where some have, it differs."""
    for p in (XN.split_pool("E0w"), XN.pool(1404, "saturated", rounded=False), XN.rescue_pool()):
        stages = XN._split_walk(p["x"], p["enc"], p["heads"])
        rescued = p.get("rescued", np.zeros(len(p["x"]), bool))
        assert XN.lo_lo_is_zero(stages, ~rescued)
        pose, lat, valid, over = XN.reference_split(p["x"], p["enc"], p["heads"])
        assert np.array_equal(over, rescued)
        want_pose, want_lat, want_valid = XN.reference(p["x"], p["enc"], p["heads"], rounded=False)
        assert np.array_equal(_bits(pose), _bits(want_pose)) and np.array_equal(_bits(lat), _bits(want_lat)) and np.array_equal(valid, want_valid)
        assert np.array_equal(_bits(pose), _bits(p["pose"])) and np.array_equal(_bits(lat), _bits(p["latent"]))
    # bumped at E0 AND E1: E1 meets a_lo with w_lo, the dropped product shows, and the certificate refuses the net (E1 needs
    # 26.5 bits: E0's outputs such as 1 + 3 2^-11 have an 11-bit hi against w_lo's 2^-4)
    enc, heads, x = XN.make_split(1404, 5, ("E0", "E1"), "int", XN.SPLIT_POOLS["E0w"]["nnz"], B=32)
    stages = XN._split_walk(x, enc, heads)
    assert not XN.lo_lo_is_zero(stages, np.ones(32, bool))
    lat = XN.reference_split(x, enc, heads)[1]
    assert (lat.astype(np.float64) != EH.encoder_latent_numpy(x, EH.Params(enc, heads), np.float64)).any()
    ok, worst, _, _ = XN.certify_split(x, enc, heads)
    assert not ok[1:].any() and XN.worst_bits(worst)["E1"] > 24


def test_old_unrounded_pool_is_unchanged():
    import hashlib
    p = XN.pool(1404, "saturated", rounded=False)
    h = hashlib.sha256()
    for k in ("x", "pose", "latent"):
        h.update(np.ascontiguousarray(p[k], np.float32).tobytes())
    assert len(p["x"]) == 256 and p["excluded"] == 0.0
    assert h.hexdigest() == "c135bc8e8c1ae2b9b0324ac11d02950e77f265aa0adc2ce271c71245fbbe4543"


def test_rescue_pool():
    """Rows times 2^k around f16's range: just inside (not rescued), over in a hidden layer only, over in the input; each with the
    unscaled row's latent and pose bits, each certified for the arithmetic that evaluates it."""
    p = XN.rescue_pool()
    kind, x = p["kind"], p["x"]
    assert p["excluded"] <= XN.MAX_EXCLUDED_SHARE and all((kind == i).sum() >= 64 for i in range(4))
    assert np.array_equal(p["rescued"], kind >= 2) and not x[0].any() and kind[0] == 0
    assert np.array_equal(_bits(p["pose"]), _bits(p["pose"][p["base"]])) and np.array_equal(_bits(p["latent"]), _bits(p["latent"][p["base"]]))
    assert (np.abs(x[kind == 2]).max(axis=1) <= 32768).all() and (np.abs(x[kind == 3]).max(axis=1) >= XN.F16_OVER).all()
    stages = XN._split_walk(x[kind == 1], p["enc"], p["heads"])
    m = np.max([np.abs(st["a"]).max(axis=1) for st in stages], axis=0)
    assert (m < XN.F16_MAX).all() and (m >= XN.F16_MAX / 2 - 1).all(), "just inside: one more doubling leaves f16's range"
    assert XN.certify_split(x[~p["rescued"]], p["enc"], p["heads"])[0].all()
    assert XN.certify(x[p["rescued"]], p["enc"], p["heads"], rounded=False)[0].all()
    print(f"rescue pool: {np.bincount(kind).tolist()} rows (plain, inside, hidden, input), excluded {p['excluded']:.3f}")


def test_raw_landmarks_normalise_to_the_fractional_features():
    """x = k + j 2^-11 through raw_landmarks(): coordinates in 2^-14ths, still exact in f32, and the f64 normalisation gives x back."""
    for name in ("E0x", "E0w"):
        p = XN.split_pool(name)
        raw = XN.raw_landmarks(p["x"], seed=11)
        assert np.array_equal(FN.normalize_ipd(raw, True), p["x"]) and not raw[0].any()
