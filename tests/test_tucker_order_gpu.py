"""GPU: the four primitives of the Tucker decomposition (csrc/tucker_decompose.hip, K7a..K7d) on the paths that
tests/test_tucker_decompose_gpu.py does not reach with a known answer, and their SUMMATION ORDER.  Every comparison is on the bits.

Exact answers (integer-valued inputs, tests/tucker_order_cases.py): K7a with three and more tile rows, at NLML_GRAM_I_MAX, and with
slices longer than NLML_GRAM_KCHUNK together with split-K; K7b where a workgroup takes two and three slabs, and its n > 16 branch for
pitch, for roll, with 16 < n < 32 and at the LDS limit of 768 cells; every rank instance of K7c; every rank triple of K7d against every
pattern of NULL factors and the four in/out dtype forms; the scalar-load forms through a base pointer 4 bytes past 16-byte alignment.

The order (standard normal inputs): each kernel against its host model (oracle/csrc/oracle.c, "K7", written from the header's
prose; tests/test_tucker_order_host.py shows on the CPU that these inputs tell the order from wrong ones), and the driver's own HOSVD
projection replayed on the host from the device's factors."""
import numpy as np
import pytest
import torch

import tucker_cases as TC
import tucker_order_cases as OC
from nlml_hpe_amd import _lib, ops
from nlml_hpe_amd import tucker_decompose as TD
from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TORCH_OF = {np.float32: F32, np.float64: F64}


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def host(t):
    return t.cpu().numpy()


def words(got, want, what):
    """Mismatching words of a device result against a host array, printed before anyone asserts on them."""
    n = OC.mismatches(host(got), want)
    print(f"{what}: {n} of {want.size} words differ")
    return n


def one_past(a, device):
    """-> (the contiguous view of `a` one element into a larger device buffer, the buffer): NaN before and after the view."""
    buf = dev(OC.one_past(a, a.size), device)
    view = buf[1:1 + a.size].view(a.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-1]))
    return view, buf


def tiles_of(I, K):
    return _lib.lib().nlml_mode_gram_workspace_bytes(I, K) // OC.TILE_BYTES


# ---- exact answers on the unreached paths: K7a -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(OC.K7A_EXACT), ids=str)
def test_mode_gram_exact_on_unreached_paths(device, shape):
    pairs, splits = OC.K7A_EXACT[shape]
    assert tiles_of(*shape) == pairs * splits, "the slice count, through the workspace query"
    assert CO.mode_gram_plan(*shape)[::2] == (pairs, splits)
    A = OC.exact_tensor(shape)
    want = OC.exact_gram(A)
    At = dev(A, device)
    G = ops.mode_gram(At)
    assert G.shape == (shape[0], shape[0]) and G.dtype == F64
    assert torch.equal(G.view(torch.int64), G.T.contiguous().view(torch.int64)), "the mirror half equals the upper half bit for bit"
    assert torch.equal(G.view(torch.int64), ops.mode_gram(At).view(torch.int64)), "two runs give the same bits"
    assert words(G, want, f"K7a exact {shape} f32 in") == 0
    if shape in OC.K7A_EXACT_F64:
        assert words(ops.mode_gram(At.double()), want, f"K7a exact {shape} f64 in") == 0


# ---- K7b --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OC.K7B_EXACT, ids=str)
def test_pose_grams_exact_on_unreached_paths(device, shape):
    X = OC.exact_tensor(shape)
    want = OC.exact_pose_grams(X)
    Xt = dev(X, device)
    for Xin, name in ((Xt, "f32"), (Xt.double(), "f64")):
        for which in OC.K7B_WHICH:
            G = ops.pose_grams(Xin, which=which)
            bad = 0
            for g, w, on in zip(G, want, which):
                assert (g is None) == (not on)
                if on:
                    bad += words(g, w, f"K7b exact {shape} {name} in, which {which}")
            assert bad == 0


# ---- K7c --------------------------------------------------------------------------------------------------------------------------
def test_project_identity_every_rank_instance(device):
    I, K = OC.K7C_EXACT
    A = OC.exact_tensor(OC.K7C_EXACT)
    At = dev(A, device)
    bad = 0
    for R in range(_lib.TUCKER_RANK_MIN, _lib.TUCKER_RANK_MAX + 1):
        U = OC.exact_factor(I, R, seed=R)
        Ut = dev(U, device)
        for tout in (np.float32, np.float64):
            out = ops.project_identity(At, Ut, out_dtype=TORCH_OF[tout])
            assert out.shape == (R, K) and out.dtype == TORCH_OF[tout]
            bad += words(out, OC.exact_identity(A, U, tout), f"K7c exact R={R} {np.dtype(tout).name} out")
    assert (_lib.TUCKER_RANK_MIN, _lib.TUCKER_RANK_MAX) == (1, 16) and bad == 0


# ---- K7d --------------------------------------------------------------------------------------------------------------------------
def test_project_pose_every_rank_null_and_dtype_instance(device):
    shape = OC.K7D_EXACT
    X = OC.exact_tensor(shape)
    Xt = {np.float32: dev(X, device), np.float64: dev(X.astype(np.float64), device)}
    bad = launches = 0
    biggest = 0.0
    for ranks in np.ndindex(3, 3, 3):
        ranks = tuple(r + 1 for r in ranks)
        for nulls in OC.NULLS:
            Us = OC.exact_pose_factors(shape, ranks, nulls)
            Ut = [None if u is None else dev(u, device) for u in Us]
            want = {t: OC.exact_pose(X, Us, t) for t in (np.float32, np.float64)}
            biggest = max(biggest, float(np.abs(want[np.float64]).max()))
            for tin, tout in OC.DTYPES:
                out = ops.project_pose(Xt[tin], *Ut, out_dtype=TORCH_OF[tout])
                launches += 1
                n = OC.mismatches(host(out), want[tout])
                if n:
                    print(f"K7d exact ranks {ranks} nulls {nulls} {np.dtype(tin).name} in {np.dtype(tout).name} out: {n} words differ")
                bad += n
    print(f"K7d exact: {launches} launches, {bad} words differ; largest result {biggest:.4g}")
    assert launches == 864 and bad == 0
    assert biggest > 2 ** 24, "some f32 outputs are rounded: the single rounding is exercised"


# ---- the unaligned base -----------------------------------------------------------------------------------------------------------
def test_mode_gram_from_an_unaligned_base(device):
    """K % 4 == 0 but the base pointer is 4 bytes past 16-byte alignment: the scalar-load form, which must read neither the element
    before the view nor the one after it (both NaN)."""
    shape = OC.K7A_UNALIGNED
    assert shape[1] % 4 == 0 and tiles_of(*shape) == 2
    A = OC.exact_tensor(shape)
    view, buf = one_past(A, device)
    assert words(ops.mode_gram(view), OC.exact_gram(A), f"K7a unaligned {shape}, exact") == 0
    R = OC.random_matrix(shape)
    view, buf = one_past(R, device)
    G = ops.mode_gram(view)
    assert bool(torch.isfinite(G).all()), "the NaN on either side of the view shows in no output"
    assert words(G, host(ops.mode_gram(dev(R, device))), f"K7a unaligned {shape}, random, against the aligned call") == 0
    assert words(G, CO.mode_gram(R), f"K7a unaligned {shape}, random, against the model") == 0


def test_pose_grams_from_an_unaligned_base(device):
    shape = OC.K7B_UNALIGNED
    assert shape[4] % 4 == 0
    X = OC.exact_tensor(shape)
    view, buf = one_past(X, device)
    assert sum(words(g, w, f"K7b unaligned {shape}, exact") for g, w in zip(ops.pose_grams(view), OC.exact_pose_grams(X))) == 0
    R = OC.random_tensor(shape)[0]
    view, buf = one_past(R, device)
    G = ops.pose_grams(view)
    assert all(bool(torch.isfinite(g).all()) for g in G), "the NaN on either side of the view shows in no output"
    aligned = ops.pose_grams(dev(R, device))
    assert sum(words(g, host(a), f"K7b unaligned {shape}, random, against the aligned call") for g, a in zip(G, aligned)) == 0
    assert sum(words(g, m, f"K7b unaligned {shape}, random, against the model") for g, m in zip(G, CO.pose_grams(R))) == 0


# ---- the order, on random inputs against the models ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(OC.K7A_RANDOM), ids=str)
def test_mode_gram_order(device, shape):
    pairs, splits = OC.K7A_RANDOM[shape]
    assert tiles_of(*shape) == pairs * splits
    A = OC.random_matrix(shape)
    want = CO.mode_gram(A)
    At = dev(A, device)
    bad = words(ops.mode_gram(At), want, f"K7a order {shape} f32 in")
    bad += words(ops.mode_gram(one_past(A, device)[0]), want, f"K7a order {shape} f32 in, unaligned base")
    bad += words(ops.mode_gram(At.double()), want, f"K7a order {shape} f64 in of f32 values")
    B = OC.random_matrix64(shape)                  # unrounded: here the products are not exact and the fused step shows
    bad += words(ops.mode_gram(dev(B, device)), CO.mode_gram(B), f"K7a order {shape} f64 in, unrounded")
    assert bad == 0


@pytest.mark.parametrize("shape", OC.K7B_RANDOM, ids=str)
def test_pose_grams_order(device, shape):
    X32, Xu = OC.random_tensor(shape)
    X64 = X32.astype(np.float64)
    m32, m64 = CO.pose_grams(X32), CO.pose_grams(X64)
    assert sum(OC.mismatches(a, b) for a, b in zip(m32, m64)) > 0, "the 32- and the 16-column orders differ on these inputs"
    bad = 0
    for Xin, model, name in ((X32, m32, "f32 in, 32-column model"), (X64, m64, "f64 in of f32 values, 16-column model"),
                             (Xu, CO.pose_grams(Xu), "f64 in, unrounded, 16-column model")):
        Xt = dev(Xin, device)
        for which in OC.K7B_WHICH:
            for g, m, on in zip(ops.pose_grams(Xt, which=which), model, which):
                if on:
                    bad += words(g, m, f"K7b order {shape} {name}, which {which}")
    assert bad == 0


@pytest.mark.parametrize("shape", OC.K7C_RANDOM, ids=str)
def test_project_identity_order(device, shape):
    A = OC.random_matrix(shape)
    At = dev(A, device)
    bad = 0
    for R in OC.K7C_RANKS:
        U = OC.random_factor(shape[0], R, seed=shape[0] + R)
        for tout in (np.float32, np.float64):
            out = ops.project_identity(At, dev(U, device), out_dtype=TORCH_OF[tout])
            bad += words(out, CO.project_identity(A, U, tout), f"K7c order {shape} R={R} {np.dtype(tout).name} out")
    assert bad == 0


@pytest.mark.parametrize("shape", OC.K7D_RANDOM, ids=str)
def test_project_pose_order(device, shape):
    X32, X64 = OC.random_tensor(shape)
    Xh = {np.float32: X32, np.float64: X64}
    Xt = {t: dev(x, device) for t, x in Xh.items()}
    bad = 0
    for ranks in OC.K7D_RANKS:
        for nulls in OC.NULLS:
            Us = OC.random_pose_factors(shape, ranks, nulls)
            Ut = [None if u is None else dev(u, device) for u in Us]
            for tin, tout in OC.DTYPES:
                out = ops.project_pose(Xt[tin], *Ut, out_dtype=TORCH_OF[tout])
                bad += words(out, CO.project_pose(Xh[tin], *Us, out_dtype=tout),
                             f"K7d order {shape} ranks {ranks} nulls {nulls} {np.dtype(tin).name} in {np.dtype(tout).name} out")
    assert bad == 0


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def test_driver_hosvd_projection_replayed_on_the_host(device):
    """tucker(n_iter_max=0) projects X on the HOSVD factors: K7c with f64 out, then K7d with f64 in and out, then one rounding.  The
    same two steps through the models, from the device's own factors, must give W's bits: the models state the calls the driver
    really makes."""
    Xh = np.array(TC.noisy_case())
    X = dev(Xh, device)
    W, U = TD.tucker(X, TC.full_rank(X), n_iter_max=0, backend="device")
    Uh = [host(u) for u in U]
    assert [u.shape for u in Uh] == [(n, r) for n, r in zip(Xh.shape[:4], TC.RANK)] and all(u.dtype == np.float64 for u in Uh)
    A = Xh.reshape(Xh.shape[0], -1)
    Z = CO.project_identity(A, Uh[0], np.float64)
    assert words(ops.project_identity(X.reshape(A.shape), U[0], out_dtype=F64), Z, "driver: K7c, f64 out") == 0
    Z = Z.reshape((TC.RANK[0],) + Xh.shape[1:])
    Wm = CO.project_pose(Z, Uh[1], Uh[2], Uh[3], out_dtype=np.float64).astype(np.float32)
    assert W.dtype == F32 and words(W, Wm, "driver: W") == 0
