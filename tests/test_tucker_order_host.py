"""CPU: the host statements of the summation orders of the Tucker decomposition's four primitives (oracle_mode_gram,
oracle_pose_grams, oracle_project_identity, oracle_project_pose in oracle/csrc/oracle.c) -- the yardsticks of
tests/test_tucker_order_gpu.py -- tied to what is already established, on the inputs of tests/tucker_order_cases.py:

  1  against numpy f64    each model, at variant 0, within the accumulation bound tests/test_tucker_decompose_gpu.py holds the device to;
  2  the slice rule       the model's K7a plan against nlml_mode_gram_workspace_bytes: slices x pairs x 131,072 bytes for every tested (I, K);
  3  the inputs work      every deliberately wrong order changes at least one output word wherever it can differ by construction (the
                          counts are printed), and the 32- and 16-column forms of K7b differ on f32-representable inputs: the header's
                          "same sums" does not extend to the bits of K7b's f64 form;
  4  exact inputs         on integer-valued inputs variant 0 and every wrong order return the int64 answer exactly, results above 2^24
                          rounded once to f32 included.
"""
import numpy as np
import pytest

import tucker_cases as TC
import tucker_order_cases as OC
from nlml_hpe_amd import _lib
from oracle import c_oracle as CO

U53, U24 = 2.0 ** -53, 2.0 ** -24


def gram_bound(A64):
    return 2 * A64.shape[1] * U53 * (np.abs(A64) @ np.abs(A64).T)


def null_name(nulls):
    return "".join("-" if z else c for z, c in zip(nulls, "ypr"))


# ---- 2: the slice rule ------------------------------------------------------------------------------------------------------------
def test_slice_rule_is_the_librarys():
    L = _lib.lib()
    cases = dict(OC.K7A_EXACT)
    cases.update(OC.K7A_RANDOM)
    cases[OC.K7A_UNALIGNED] = (1, 2)
    cases[(1620, 11 * 9 * 7 * 1404)] = (91, 11)          # the reference's own shape: 11 slices of 88,480
    cases[(1104, 11 * 9 * 7 * 1404)] = (45, 22)          # test_offsets_beyond_4_gib's
    for (I, K), (pairs, splits) in cases.items():
        got = CO.mode_gram_plan(I, K)
        assert (got[0], got[2]) == (pairs, splits), (I, K, got)
        assert got[1] % 32 == 0 and got[1] >= OC.KCH and (got[2] - 1) * got[1] < K <= got[2] * got[1]
        assert L.nlml_mode_gram_workspace_bytes(I, K) == splits * pairs * OC.TILE_BYTES, (I, K)
    assert CO.mode_gram_plan(1620, 11 * 9 * 7 * 1404)[1] == 88480 and CO.mode_gram_plan(1104, 11 * 9 * 7 * 1404)[1] == 44256
    assert CO.mode_gram_plan(2049, 24600)[1] == 4128 and CO.mode_gram_plan(4096, 4100)[1] == 4128
    # a sweep of small shapes around the tile and slice edges
    for I in (1, 128, 129, 256, 257, 1409, 4096):
        for K in (1, 4095, 4096, 4097, 8192, 8193, 100003):
            pairs, slice_, splits = CO.mode_gram_plan(I, K)
            assert L.nlml_mode_gram_workspace_bytes(I, K) == splits * pairs * OC.TILE_BYTES, (I, K)


def test_pose_grams_partial_counts():
    """What the exact cases are there for: workgroups that take two and three slabs, and the workspace that holds the f64 form's count."""
    s = OC.K7B_EXACT[0]
    assert OC.slabs(s, 32) == 1300 and OC.slabs(s, 16) == 2340
    assert _lib.lib().nlml_pose_grams_workspace_bytes(*s) == 1024 * (9 + 4 + 4) * 8
    assert [int(np.prod(x[1:4])) for x in OC.K7B_EXACT[1:]] == [768, 768, 680, 765]
    assert all(int(np.prod(x[1:4])) <= _lib.POSE_GRAMS_MAX_CELLS for x in OC.K7B_EXACT + OC.K7B_RANDOM)


# ---- 1 and 3: K7a -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(OC.K7A_RANDOM), ids=str)
def test_mode_gram_model(shape):
    A = OC.random_matrix(shape)
    A64 = A.astype(np.float64)
    G = CO.mode_gram(A)
    assert np.array_equal(G, G.T)
    assert np.all(np.abs(G - A64 @ A64.T) <= gram_bound(A64))
    assert OC.mismatches(CO.mode_gram(A64), G) == 0, "f64 input of f32-representable values: the same chain"
    splits = OC.K7A_RANDOM[shape][1]
    for v, what in OC.K7A_VARIANTS.items():
        n = OC.mismatches(CO.mode_gram(A, variant=v), G)
        print(f"K7a {shape} ({splits} slices) variant {v} ({what}): {n} of {G.size} words change")
        # "no slices" needs more than one slice; adding the slices descending needs three: 0.0 + a + b is 0.0 + b + a
        if v == 3:
            assert splits > 1 and n > 0
        elif v == 4:
            assert n > 0 if splits >= 3 else n == 0
        elif v == 2:
            assert n == 0                          # the product of two f32 values is exact in f64: fused or not, one rounding
        else:
            assert n > 0
    assert any(s >= 3 for _, s in OC.K7A_RANDOM.values()), "one input family can tell the slices' order"
    # ... so the fused step is told apart on the f64 form's unrounded values, which the GPU test runs as well
    B = OC.random_matrix64(shape)
    GB = CO.mode_gram(B)
    assert np.all(np.abs(GB - B @ B.T) <= gram_bound(B))
    n = OC.mismatches(CO.mode_gram(B, variant=2), GB)
    print(f"K7a {shape} unrounded f64 in, variant 2 ({OC.K7A_VARIANTS[2]}): {n} of {GB.size} words change")
    assert n > 0


# ---- K7b --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OC.K7B_RANDOM, ids=str)
def test_pose_grams_model(shape):
    X = OC.random_tensor(shape)[0]
    X64 = X.astype(np.float64)
    G32, G64 = CO.pose_grams(X), CO.pose_grams(X64)
    for m, (g32, g64) in enumerate(zip(G32, G64), start=1):
        A = TC.unfold(X64, m)
        for g in (g32, g64):
            assert np.array_equal(g, g.T)
            assert np.all(np.abs(g - A @ A.T) <= gram_bound(A))
    for which in OC.K7B_WHICH[1:]:
        part = CO.pose_grams(X, which=which)
        assert all((p is None) != w and (p is None or OC.mismatches(p, g) == 0) for p, g, w in zip(part, G32, which))
    # the 32-column model against the 16-column model: the header's corrected sentence
    n = sum(OC.mismatches(a, b) for a, b in zip(G32, G64))
    print(f"K7b {shape}: the f32 form's 32-column slabs and the f64 form's 16-column slabs differ in {n} words")
    assert n > 0
    assert all(OC.mismatches(a, b) == 0 for a, b in zip(CO.pose_grams(X64, variant=2), G32)), "variant 2 IS the 32-column order"
    parts = {32: min(OC.slabs(shape, 32), 1024), 16: min(OC.slabs(shape, 16), 1024)}
    Xu = OC.random_tensor(shape)[1]                # the unrounded draws, as a projection kept in f64 holds them
    Gu = CO.pose_grams(Xu)
    for m, g in enumerate(Gu, start=1):
        assert np.all(np.abs(g - TC.unfold(Xu, m) @ TC.unfold(Xu, m).T) <= gram_bound(TC.unfold(Xu, m)))
    for v, what in OC.K7B_VARIANTS.items():
        for name, Xin, want in (("f32", X, G32), ("f64", X64, G64), ("f64 unrounded", Xu, Gu)):
            got = CO.pose_grams(Xin, variant=v)
            n = sum(OC.mismatches(a, b) for a, b in zip(got, want))
            print(f"K7b {shape} {name} in, variant {v} ({what}): {n} words change")
            if v == 2 and name == "f32":
                assert n == 0                      # the f32 form's slabs are 32 columns wide already
            elif v == 3 and parts[32 if name == "f32" else 16] < 3:
                assert n == 0                      # fewer than three partials: their sum has one order
            else:
                assert n > 0


# ---- K7c --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OC.K7C_RANDOM, ids=str)
@pytest.mark.parametrize("R", OC.K7C_RANKS)
def test_project_identity_model(shape, R):
    I, K = shape
    A = OC.random_matrix(shape)
    A64 = A.astype(np.float64)
    U = OC.random_factor(I, R, seed=I + R)
    ref = U.T @ A64
    spread = np.abs(U).T @ np.abs(A64)
    z64, z32 = CO.project_identity(A, U, np.float64), CO.project_identity(A, U)
    assert np.all(np.abs(z64 - ref) <= 2 * I * U53 * spread)          # the chain's I terms and the reference's own
    assert np.all(np.abs(z32.astype(np.float64) - ref) <= U24 * np.abs(ref) + I * U53 * spread)
    assert OC.mismatches(z64.astype(np.float32), z32) == 0, "one cast"
    for v, what in OC.K7C_VARIANTS.items():
        n64 = OC.mismatches(CO.project_identity(A, U, np.float64, variant=v), z64)
        n32 = OC.mismatches(CO.project_identity(A, U, variant=v), z32)
        print(f"K7c {shape} R={R} variant {v} ({what}): f64 out {n64} of {z64.size} words change, f32 out {n32}")
        assert n64 > 0                             # the f32 output hides most of it behind its one rounding: printed, not required


# ---- K7d --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OC.K7D_RANDOM, ids=str)
@pytest.mark.parametrize("ranks", OC.K7D_RANKS, ids=str)
def test_project_pose_model(shape, ranks):
    X32, X64 = OC.random_tensor(shape)
    for nulls in OC.NULLS:
        Us = OC.random_pose_factors(shape, ranks, nulls)
        given = 3 - sum(nulls)
        depth = sum(n for n, z in zip(shape[1:4], nulls) if not z)
        terms = int(np.prod([n for n, z in zip(shape[1:4], nulls) if not z]))
        for tin, tout in OC.DTYPES:
            X = X32 if tin == np.float32 else X64
            Xd = X.astype(np.float64)
            ref = OC.contract_pose(Xd, Us)
            spread = OC.contract_pose(np.abs(Xd), [None if u is None else np.abs(u) for u in Us])
            out = CO.project_pose(X, *Us, out_dtype=tout)
            assert out.shape == ref.shape and out.dtype == tout
            err = np.abs(out.astype(np.float64) - ref)
            if tout == np.float64:
                assert np.all(err <= 2 * depth * U53 * spread), (nulls, tin, tout)
            else:
                assert np.all(err <= U24 * np.abs(ref) + terms * U53 * spread), (nulls, tin, tout)
            if tout != np.float64:
                continue
            for v, what in OC.K7D_VARIANTS.items():
                n = OC.mismatches(CO.project_pose(X, *Us, out_dtype=tout, variant=v), out)
                print(f"K7d {shape} ranks {ranks} factors {null_name(nulls)} {np.dtype(tin).name} in, variant {v} ({what}): "
                      f"{n} of {out.size} words change")
                # no factor: a copy.  One factor: the nest is one chain, which the Kronecker form and the other nesting share.
                if given == 0 or (given == 1 and v in (3, 4)):
                    assert n == 0
                else:
                    assert n > 0


# ---- 4: exactly summable inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OC.K7A_EXACT_HOST, ids=str)
def test_mode_gram_exact_on_the_host(shape):
    A = OC.exact_tensor(shape)
    want = OC.exact_gram(A)
    for v in [0] + list(OC.K7A_VARIANTS):
        assert np.array_equal(CO.mode_gram(A, variant=v), want), v
    assert np.array_equal(CO.mode_gram(A.astype(np.float64)), want)


@pytest.mark.parametrize("shape", OC.K7B_EXACT + [OC.K7B_UNALIGNED], ids=str)
def test_pose_grams_exact_on_the_host(shape):
    X = OC.exact_tensor(shape)
    want = OC.exact_pose_grams(X)
    for Xin in (X, X.astype(np.float64)):
        for v in [0] + list(OC.K7B_VARIANTS):
            assert all(np.array_equal(g, w) for g, w in zip(CO.pose_grams(Xin, variant=v), want)), v


def test_project_identity_exact_on_the_host():
    I, K = OC.K7C_EXACT
    A = OC.exact_tensor(OC.K7C_EXACT)
    for R in range(1, 17):
        U = OC.exact_factor(I, R, seed=R)
        for tout in (np.float32, np.float64):
            want = OC.exact_identity(A, U, tout)
            for v in [0] + list(OC.K7C_VARIANTS):
                assert OC.mismatches(CO.project_identity(A, U, tout, variant=v), want) == 0, (R, tout, v)


def test_project_pose_exact_on_the_host():
    shape = OC.K7D_EXACT
    X = OC.exact_tensor(shape)
    biggest = 0
    for ranks in ((3, 3, 3), (2, 1, 3), (1, 2, 2)):
        for nulls in OC.NULLS:
            Us = OC.exact_pose_factors(shape, ranks, nulls)
            for tin, tout in OC.DTYPES:
                want = OC.exact_pose(X, Us, tout)
                if tout == np.float32:
                    biggest = max(biggest, float(np.abs(OC.exact_pose(X, Us, np.float64)).max()))
                for v in [0] + list(OC.K7D_VARIANTS):
                    assert OC.mismatches(CO.project_pose(X.astype(tin), *Us, out_dtype=tout, variant=v), want) == 0, (ranks, nulls, v)
    print(f"K7d exact: largest result {biggest:.4g} (2^24 = {2 ** 24})")
    assert biggest > 2 ** 24, "some f32 outputs are rounded: the single rounding is exercised"
    full = OC.exact_pose(X, OC.exact_pose_factors(shape, (3, 3, 3), (0, 0, 0)), np.float64)
    assert np.any(full.astype(np.float32).astype(np.float64) != full), "... and the rounding is not exact for some of them"
