"""CPU: the C oracle's order model of K9 (oracle/csrc/oracle.c "K9", chained by tests/encoder_train_order_cases.py) before the device
is held to it bit for bit in tests/test_encoder_train_order_gpu.py:
  - the Python statement of the workspace layout gives the library's byte count for every (F, batch);
  - the model chained over one whole step equals the host form (nlml_encoder_train_steps_host) in VALUE on every word of the loss,
    the norm, the gradients and the parameters -- the two were written apart from the same prose, so a misreading in either shows;
  - every model GEMM element lies within the derived chain bound of numpy float64;
  - every deliberately wrong order changes at least one word on the inputs the GPU tests use;
  - small-integer operands give the exact integer answer in every variant (no term dropped or doubled).
"""
import functools

import numpy as np
import pytest

import encoder_train_cases as EC
import encoder_train_order_cases as OC
from nlml_hpe_amd import _lib
from oracle import c_oracle as CO

HYPERS = {"no clip": OC.NO_CLIP, "clip and decay": dict(lr=1e-2, weight_decay=1e-2, max_norm=0.1, zero_grad=False)}


@functools.lru_cache(maxsize=None)
def _chained(F, B, hyper_name="no clip"):
    cs = EC.case(F, B)
    rows, _ = OC.resolve_rows(None, 0, B, B)
    return OC.model_step(cs["x"], rows, OC.targets(cs, rows), cs["params"], np.zeros_like(cs["params"]), F, HYPERS[hyper_name])


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
def test_layout_total_equals_the_workspace_query():
    for F in (136, 1404):
        d = OC.dims(F)
        assert d["total"] == EC.case(F, 33)["params"].size
        assert d["n_partials"] == CO.et_n_partials(F)
        for batch in range(1, 257):
            assert OC.layout(F, batch)["bytes"] == _lib.lib().nlml_encoder_train_workspace_bytes(F, batch), (F, batch)


def test_layout_regions_are_disjoint_and_aligned():
    for F, batch in ((136, 1), (136, 33), (1404, 33), (1404, 256)):
        lay = OC.layout(F, batch)
        starts = [lay["partials"], lay["rows"]] + lay["act"] + lay["delta"] + [lay["bytes"]]
        sizes = [lay["n_partials"] * 8, 1024] + [batch * ld * 4 for ld in lay["ld"]] * 2
        assert all(a + s <= b for a, s, b in zip(starts, sizes, starts[1:]))
        assert all(o % 16 == 0 for o in lay["act"] + lay["delta"]) and lay["rows"] % 16 == 0


# ---- the model against the host form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F, B", OC.SHAPES)
def test_chained_model_equals_the_host_form_in_value(F, B):
    """== on values: -0 and +0 count as equal, because the host form skips k >= K where the model (and the device) run fmaf(0, 0, p).
    Nothing looser: any other difference in any word fails."""
    cs = EC.case(F, B)
    for name, hyper in HYPERS.items():
        m = _chained(F, B, name)
        host = EC.host_train(cs, None, B, **hyper)
        assert host["loss"][0] == m["loss"] and host["norm"][0] == m["norm"], (name, host["loss"], m["loss"], host["norm"], m["norm"])
        assert np.array_equal(host["flat"][1], m["g_out"]), f"{name}: {(host['flat'][1] != m['g_out']).sum()} gradient words differ"
        assert np.array_equal(host["flat"][0], m["p_out"]), f"{name}: {(host['flat'][0] != m['p_out']).sum()} parameter words differ"
    assert _chained(F, B, "clip and decay")["c"] < 1.0, "the second setting clips"


def test_two_chained_steps_accumulate_as_the_host_form_does():
    F, B = 136, 33
    cs = EC.case(F, 2 * B)
    hyper = dict(lr=1e-2, weight_decay=1e-2, max_norm=0.3, zero_grad=False)
    p, g = cs["params"].copy(), np.zeros_like(cs["params"])
    for s in range(2):
        rows, _ = OC.resolve_rows(None, s * B, B, 2 * B)
        m = OC.model_step(cs["x"], rows, OC.targets(cs, rows), p, g, F, hyper)
        p, g = m["p_out"], m["g_out"]
    host = EC.host_train(cs, None, B, **hyper)
    assert host["norm"][1] == m["norm"] and host["loss"][1] == m["loss"]
    assert np.array_equal(host["flat"][0], p) and np.array_equal(host["flat"][1], g)


# ---- element-wise accuracy -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F, B", OC.SHAPES)
def test_every_model_gemm_element_within_the_chain_bound(F, B):
    cs, m, d = EC.case(F, B), _chained(F, B), OC.dims(F)
    p = cs["params"]
    for l in range(6):
        W = p[d["w_off"][l]:d["b_off"][l]].reshape(d["out"][l], d["in"][l])
        a_prev = cs["x"] if l == 0 else m["act"][l - 1]
        checks = [(f"Z_{l}", m["z"][l], OC.chain_bound(a_prev, W.T, p[d["b_off"][l]:d["b_off"][l] + d["out"][l]])),
                  (f"dW_{l}", m["g_pre"][d["w_off"][l]:d["b_off"][l]].reshape(W.shape), OC.chain_bound(m["delta"][l].T, a_prev))]
        if l:
            checks.append((f"dgrad_{l}", m["dsum"][l], OC.chain_bound(m["delta"][l], W)))
        for what, got, (ref, bound) in checks:
            over = np.abs(got.astype(np.float64) - ref) > bound
            assert not over.any(), f"{what}: {over.sum()} elements beyond (K + 2) 2^-24 (sum |a b| + |start|)"


# ---- the wrong orders show on the GPU tests' inputs ------------------------------------------------------------------------------------
def _shows(F, B, variant, hyper_name="no clip"):
    """The quantities of one step that the wrong order changes, each launch fed the RIGHT model's outputs (so nothing is inherited)."""
    cs, right = EC.case(F, B), _chained(F, B, hyper_name)
    rows, _ = OC.resolve_rows(None, 0, B, B)
    feed = {"act": right["act"], "delta": right["delta"], "partials": right["partials"]}
    args = (cs["x"], rows, OC.targets(cs, rows), cs["params"], np.zeros_like(cs["params"]), F, HYPERS[hyper_name])
    base = OC.model_step(*args, observed=feed)
    wrong = OC.model_step(*args, observed=feed, variant=variant)
    keys = [("z", l) for l in range(6)] + [("delta", l) for l in range(6)] + ["loss", "g_pre", "partials", "p_out", "g_out"]
    get = lambda m, k: m[k[0]][k[1]] if isinstance(k, tuple) else m[k]
    return {k for k in keys if OC.mismatches(np.asarray(get(base, k)), np.asarray(get(wrong, k)))}


# where a variant can NOT show, and why:
#   5  runs of 16 rows are the order itself once ceil(B / 16) = 16 (B >= 241), and for B <= 16 one run of B rows adds the rows in
#      the same sequence as B runs of one row; it shows from B = 17 on (B = 17, 33, 129 below)
#   6  a tree that folds the upper half of B slots onto the lower is the 256-slot tree whenever every fold is by a power of two,
#      i.e. for B = 2^k and 2^k - 1 (1, 15, 16, 255, 256: the 256-slot tree only adds exact zeros more); it shows on 17, 33, 129, 241
#   8  with c = 1 or weight_decay = 0 the contraction has nothing to contract; it shows in the clip-and-decay run
#      variant 6 moves ONE word of a step, the loss, and two trees over the same addends often round alike; so it is held to show
#      on at least one of those four cases, and the test prints on which
CANNOT = {5: {1, 15, 16, 241, 255, 256}, 6: {1, 15, 16, 255, 256}}


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5, 7])
@pytest.mark.parametrize("F, B", [s for s in OC.SHAPES if s[1] <= 33] + [(136, 129)])
def test_wrong_variant_changes_a_word(F, B, variant):
    changed = _shows(F, B, variant)
    if B in CANNOT.get(variant, ()):
        assert not changed, f"variant {variant} ({OC.VARIANTS[variant]}) is the order itself at B={B}, yet {changed} changed"
    else:
        assert changed, f"variant {variant} ({OC.VARIANTS[variant]}) changes no word at F={F} B={B}"
        print(f"variant {variant} F={F} B={B}: changes {sorted(map(str, changed))}")


def test_loss_tree_over_B_slots_shows_on_a_gpu_case():
    shows = []
    for F, B in OC.SHAPES:
        pred, tgt = _chained(F, B)["act"][5], OC.targets(EC.case(F, B), np.arange(B))
        right, wrong = CO.et_loss(pred, tgt), CO.et_loss(pred, tgt, variant=6)
        assert OC.mismatches(right["q"], wrong["q"]) == 0 and OC.mismatches(right["delta6"], wrong["delta6"]) == 0
        if OC.mismatches(right["loss"], wrong["loss"]):
            shows.append((F, B))
    print("variant 6 changes the loss word on", shows)
    assert shows and not {B for _, B in shows} & CANNOT[6]


@pytest.mark.parametrize("B", [241, 255, 256])
def test_bias_runs_of_16_rows_are_the_order_at_the_large_batches(B):
    m = _chained(136, B)
    for l in range(6):
        assert OC.mismatches(CO.et_bias_grad(m["delta"][l]), CO.et_bias_grad(m["delta"][l], variant=5)) == 0


def test_contracted_update_shows_only_with_clip_and_decay():
    assert _shows(136, 33, 8) == set()
    assert "p_out" in _shows(136, 33, 8, "clip and decay")


# ---- exact inputs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("M, N, K", [(1, 1, 1), (3, 5, 9), (33, 9, 64), (5, 40, 136), (2, 33, 257), (4, 28, 1404)])
def test_small_integer_gemm_is_exact_in_every_variant(M, N, K, variant):
    g = np.random.default_rng(K)
    A, Bm, start = g.integers(-8, 9, (M, K)), g.integers(-8, 9, (K, N)), g.integers(-8, 9, N)
    want = A @ Bm + start                      # int64; every partial sum is below 2^24
    for a_kc in (True, False):
        for b_kc in (True, False):
            got = CO.et_gemm(A if a_kc else A.T, Bm.T if b_kc else Bm, K, start=start, a_kc=a_kc, b_kc=b_kc, variant=variant)
            assert np.array_equal(got.astype(np.int64), want), (a_kc, b_kc)
    rows = g.permutation(K + 3)[:K].astype(np.int32)   # a gathered k-outer operand and a gathered k-contiguous one
    big = np.zeros((K + 3, N), np.float32)
    big[rows] = Bm
    assert np.array_equal(CO.et_gemm(A, big, K, start=start, b_rows=rows, variant=variant).astype(np.int64), want)
    mrows = g.permutation(M + 2)[:M].astype(np.int32)
    bigA = np.zeros((M + 2, K), np.float32)
    bigA[mrows] = A
    assert np.array_equal(CO.et_gemm(bigA, Bm, K, start=start, a_rows=mrows, M=M, variant=variant).astype(np.int64), want)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 129, 241, 255, 256])
def test_small_integer_sums_are_exact_in_every_variant(B):
    g = np.random.default_rng(B)
    delta = g.integers(-8, 9, (B, 9)).astype(np.float32)
    for variant in (0, 5):
        assert np.array_equal(CO.et_bias_grad(delta, variant).astype(np.int64), delta.astype(np.int64).sum(axis=0))
    pred, tgt = g.integers(-8, 9, (B, 9)).astype(np.float32), g.integers(-8, 9, (B, 9)).astype(np.float32)
    for variant in (0, 6):
        ls = CO.et_loss(pred, tgt, variant)
        d = (pred - tgt).astype(np.int64)
        assert np.array_equal(ls["q"].astype(np.int64), (d * d).sum(axis=1)) and int(ls["slots"][0]) == int((d * d).sum())
        assert ls["loss"] == np.float32(ls["slots"][0]) / np.float32(3 * B)
        assert np.array_equal(ls["delta6"], (pred - tgt) * np.float32(2.0 / (3.0 * B)))


def test_small_integer_norm_and_update_are_exact_in_every_variant():
    F = 136
    n = OC.dims(F)["total"]
    g = np.random.default_rng(7)
    G = g.integers(-3, 4, n).astype(np.float32)     # sum of squares < 2^24: exact in f32 too
    for variant in (0, 7):
        nm = CO.et_norm(F, G=G, max_norm=8.0, variant=variant)
        assert nm["partials"].sum() == float((G.astype(np.int64) ** 2).sum()) == nm["tree"][0] == nm["chains"].sum()
        assert nm["norm"] == np.sqrt(nm["tree"][0]) and nm["c"] == min(1.0, 8.0 / (nm["norm"] + 1e-6))
    again = CO.et_norm(F, partials=nm["partials"], max_norm=8.0)
    assert again["norm"] == nm["norm"] and np.array_equal(again["chains"], nm["chains"])
    p = g.integers(-8, 9, n).astype(np.float32)
    for variant in (0, 8):                          # c, lr, wd powers of two: every product and sum is exact
        p2, g2 = CO.et_update(p, G, 0.5, 0.25, 2.0, variant)
        assert np.array_equal(g2, 0.5 * G) and np.array_equal(p2, p - 0.25 * (0.5 * G + 2.0 * p))


# ---- the checker itself ------------------------------------------------------------------------------------------------------------------
def _fake_workspace(F, batch, B, m):
    """The workspace a device that IS the chained model would leave: NaN fill, then the model's rows, A, delta and partials."""
    lay = OC.layout(F, batch)
    ws = np.full(lay["bytes"] // 4, OC.FILL, np.uint32).view(np.uint8)
    v = OC.workspace_views(ws, F, batch, B)
    v["partials"][:] = m["partials"]
    v["rows"][:] = np.arange(B)
    for l in range(6):
        v["act"][l][:], v["delta"][l][:] = m["act"][l], m["delta"][l]
    return ws


@pytest.mark.parametrize("batch", [33, 256])
def test_pin_accepts_the_models_own_step_and_sees_one_changed_bit(batch):
    F, B = 136, 33
    cs, m = EC.case(F, B), _chained(F, B)
    before, after = (cs["params"], np.zeros_like(cs["params"])), (m["p_out"], m["g_out"])
    ws = _fake_workspace(F, batch, B, m)
    args = (cs, np.arange(B, dtype=np.int32), before, after)
    bad, info = OC.pin_step(*args, ws, batch, m["loss"], m["norm"], OC.NO_CLIP)
    assert not any(bad.values()) and info["tanh_ulp"] <= OC.TANH_ULP, bad
    lay = OC.layout(F, batch)
    for what, at in (("A_2", lay["act"][1] + 4 * 700), ("delta_6", lay["delta"][5] + 4 * 13), ("delta_3", lay["delta"][2] + 4 * 5),
                     ("partials", 8 * 100), ("padding words overwritten", lay["delta"][5] + 4 * 9), ("padding words overwritten", lay["bytes"] - 4 if batch == 33 else lay["act"][0] + 4 * 1024 * 40)):
        hurt = ws.copy()
        hurt[at] ^= 1
        bad, _ = OC.pin_step(*args, hurt, batch, m["loss"], m["norm"], OC.NO_CLIP)
        assert bad[what] >= 1, (what, bad)
    flipped = m["g_out"].copy()
    flipped.view(np.uint32)[123456] ^= 1
    bad, _ = OC.pin_step(cs, args[1], before, (m["p_out"], flipped), ws, batch, m["loss"], m["norm"], OC.NO_CLIP)
    assert bad["G_out"] == 1 and bad["p_out"] == 0
    bad, _ = OC.pin_step(*args, ws, batch, np.nextafter(m["loss"], np.float32(9)), m["norm"], OC.NO_CLIP)
    assert bad["loss"] == 1
