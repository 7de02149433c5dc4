"""GPU: K3g (nlml_tucker_gradient_r / ops.tucker_gradient): objective value and analytic gradient in the reference's operation order.
The yardstick is nlml_tucker_gradient_host, the host restatement that tests/test_td_gradient_host.py pins to the reference's fixtures
and numpy calls bit for bit; the device must return ITS bits for every component, and the fixtures' directly."""
import math

import numpy as np
import pytest
import torch

import rank_fixture as RF
import td_gradient_common as GC
from nlml_hpe_amd import _lib, ops, synth
from oracle import tucker as OT

pytestmark = pytest.mark.gpu


def _dev_gradient(W, X, P, cp, device, x_index=None):
    Wm = torch.from_numpy(np.ascontiguousarray(W, np.float32).reshape(-1, 1404)).to(device)
    xi = None if x_index is None else torch.from_numpy(np.asarray(x_index, np.int32)).to(device)
    err, grad = ops.tucker_gradient(Wm, torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(device),
                                    torch.from_numpy(np.ascontiguousarray(P)).to(device), torch.from_numpy(cp).to(device), x_index=xi)
    return err.cpu().numpy(), grad.cpu().numpy()


N_WIDE = 130                       # two full 64-evaluation workgroups of the second launch and a partial third
WIDE_RANKS = (1, 5, 16)


@pytest.fixture(scope="module")
def host_draws(tucker_art):
    """Per rank: the draws and the host restatement's (err, grad) on them -- computed once, sliced by the size cases.  130 draws for
    the ranks 1, 5 and 16, 17 for the others."""
    out = {}
    cp = GC.cos_block(tucker_art)
    for R in (1, 3, 5, 8, 16):
        W, P, X = GC.draws(tucker_art, R, N_WIDE if R in WIDE_RANKS else 17)
        out[R] = (W, P, X) + GC.gradient_host(W, X, P, cp)
    return out


@pytest.mark.parametrize("R", [1, 3, 5, 8, 16])
@pytest.mark.parametrize("N", [1, 2, 3, 8, 9, 17])
def test_device_gradient_is_the_host_restatement_bit_for_bit(N, R, host_draws, tucker_art, device):
    """N crosses the pass grouping: one and two gradients per pass, a partial last workgroup, more than one workgroup."""
    W, P, X, e_h, g_h = host_draws[R]
    err, grad = _dev_gradient(W, X[:N], P[:N], GC.cos_block(tucker_art), device)
    print(f"N={N} R={R}: err mismatches {int((err != e_h[:N]).sum())}, gradient mismatches {int((grad != g_h[:N]).sum())} of {grad.size}")
    assert np.array_equal(err, e_h[:N])
    assert np.array_equal(grad, g_h[:N])


@pytest.mark.parametrize("R", WIDE_RANKS)
@pytest.mark.parametrize("N", [63, 64, 65, 128, N_WIDE])
def test_device_gradient_past_one_workgroup_of_the_second_launch(N, R, host_draws, tucker_art, device):
    """The second launch takes 64 evaluations per workgroup and reads t transposed with a row stride of N: one lane short of a full
    workgroup, a full one, one evaluation into the second, two full ones, a partial third."""
    W, P, X, e_h, g_h = host_draws[R]
    err, grad = _dev_gradient(W, X[:N], P[:N], GC.cos_block(tucker_art), device)
    print(f"N={N} R={R}: err mismatches {int((err != e_h[:N]).sum())}, gradient mismatches {int((grad != g_h[:N]).sum())} of {grad.size}")
    assert np.array_equal(err, e_h[:N])
    assert np.array_equal(grad, g_h[:N])


@pytest.fixture(scope="module")
def scaled_draws(tucker_art):
    """Per rank 1 and 5: six draws whose x columns are scaled by 10 ** uniform(-6, 6), the host restatement's (err, grad) on them, and
    the products r * e_a (f64[6, 3, 1404]) formed with numpy as the reference forms them (TD_Tester.py:60-102)."""
    out = {}
    cp = GC.cos_block(tucker_art)
    rows = RF.cos_rows(tucker_art)
    for R in (1, 5):
        W, P, X = GC.draws(tucker_art, R, 6)
        X = (X * 10.0 ** synth.rng(60 + R, 0).uniform(-6, 6, 1404)).astype(np.float32)
        prods = np.empty((6, 3, 1404))
        for n in range(6):
            f = OT.f_vectors(P[n], *rows)
            r = X[n] - np.einsum('ijklm,i,j,k,l->m', W, P[n, 3:], *f)
            for a in range(3):
                w, p = P[n, a], rows[a]
                df = np.array([-q[0] * q[1] * np.sin(q[1] * w + q[2]) for q in p]).flatten().astype(np.float32)
                prods[n, a] = r * np.einsum('ijklm,i,j,k,l->m', W, P[n, 3:], *(df if b == a else f[b] for b in range(3)))
        out[R] = (W, P, X, prods) + GC.gradient_host(W, X, P, cp)
    return out


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("N", [1, 3, 4, 6])
def test_angle_components_with_an_order_sensitive_residual(N, R, scaled_draws, tucker_art, device):
    """The pairwise tree over r * e_a where its order shows: one gradient alone, an odd count in a workgroup (the tree on three rows),
    a full workgroup, a second workgroup with two."""
    W, P, X, prods, e_h, g_h = scaled_draws[R]
    # the input does its job: the host's angle components are numpy's pairwise sums of these products, and added left to right
    # (np.cumsum) at least one of them would be another double
    pairwise, in_sequence = -np.sum(prods[:N], axis=2), -np.cumsum(prods[:N], axis=2)[:, :, -1]
    assert np.array_equal(pairwise, g_h[:N, :3])
    assert (in_sequence != pairwise).any()
    err, grad = _dev_gradient(W, X[:N], P[:N], GC.cos_block(tucker_art), device)
    print(f"N={N} R={R}: err mismatches {int((err != e_h[:N]).sum())}, gradient mismatches {int((grad != g_h[:N]).sum())} of {grad.size}; "
          f"{int((in_sequence != pairwise).sum())} of {3 * N} angle components depend on the order")
    assert np.array_equal(err, e_h[:N])
    assert np.array_equal(grad, g_h[:N])


@pytest.mark.parametrize("R", WIDE_RANKS)
def test_wide_batch_with_shared_rows_without_err_and_through_a_used_workspace(R, host_draws, tucker_art, device):
    W, P, X, e_h, g_h = host_draws[R]
    cp = GC.cos_block(tucker_art)
    N = N_WIDE
    # x_index over 7 shared rows
    idx = (np.arange(N) * 5 % 7).astype(np.int32)
    e_i, g_i = GC.gradient_host(W, X[:7], P, cp, x_index=idx)
    err, grad = _dev_gradient(W, X[:7], P, cp, device, x_index=idx)
    assert np.array_equal(err, e_i) and np.array_equal(grad, g_i)
    assert not np.array_equal(g_i, g_h)                                       # the index is used: other faces, another gradient
    # the gradient alone
    Wm, Xd = torch.from_numpy(W.reshape(-1, 1404)).to(device), torch.from_numpy(X).to(device)
    Pd, cpd = torch.from_numpy(P).to(device), torch.from_numpy(cp).to(device)
    g_only = ops.tucker_gradient(Wm, Xd, Pd, cpd, return_err=False)
    assert np.array_equal(g_only.cpu().numpy(), g_h)
    # the C ABI on a workspace filled with NaN, then on the same workspace as another call (the shared rows) left it
    L = _lib.lib()
    nb = L.nlml_tucker_gradient_workspace_bytes(N, R)
    ws = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device=device)
    X7, idx_d = torch.from_numpy(X[:7].copy()).to(device), torch.from_numpy(idx).to(device)
    stream = torch.cuda.current_stream().cuda_stream

    def run(x, xi):
        e = torch.full((N,), float("nan"), dtype=torch.float64, device=device)
        g = torch.full((N, 3 + R), float("nan"), dtype=torch.float64, device=device)
        _lib.check(L.nlml_tucker_gradient_r(Wm.data_ptr(), x.data_ptr(), 1404, None if xi is None else xi.data_ptr(), Pd.data_ptr(),
                                            cpd.data_ptr(), N, e.data_ptr(), g.data_ptr(), R, ws.data_ptr(), nb, stream), "gradient")
        torch.cuda.synchronize()
        return e.cpu().numpy(), g.cpu().numpy()
    e1, g1 = run(Xd, None)                                                     # workspace: NaN
    e2, g2 = run(X7, idx_d)                                                    # a different call
    e3, g3 = run(Xd, None)                                                     # workspace: that call's contents
    assert np.array_equal(e1, e_h) and np.array_equal(g1, g_h)
    assert np.array_equal(e2, e_i) and np.array_equal(g2, g_i)
    assert np.array_equal(e3, e_h) and np.array_equal(g3, g_h)


def test_device_gradient_with_shared_rows_and_a_padded_stride(host_draws, tucker_art, device):
    W, P, X, _, _ = host_draws[5]
    cp = GC.cos_block(tucker_art)
    idx = np.array([2, 2, 0, 1, 1, 1, 2, 0, 0], np.int32)
    e_h, g_h = GC.gradient_host(W, X[:3], P[:9], cp, x_index=idx)
    err, grad = _dev_gradient(W, X[:3], P[:9], cp, device, x_index=idx)
    assert np.array_equal(err, e_h) and np.array_equal(grad, g_h)
    # ldx = 1408 through the C ABI itself
    Xp = torch.zeros((9, 1408), dtype=torch.float32, device=device)
    Xp[:, :1404] = torch.from_numpy(X[:9]).to(device)
    Wm = torch.from_numpy(W.reshape(-1, 1404)).to(device)
    Pd, cpd = torch.from_numpy(P[:9].copy()).to(device), torch.from_numpy(cp).to(device)
    e2, g2 = torch.empty(9, dtype=torch.float64, device=device), torch.empty((9, 8), dtype=torch.float64, device=device)
    nb = _lib.lib().nlml_tucker_gradient_workspace_bytes(9, 5)
    ws = torch.empty(nb // 8, dtype=torch.float64, device=device)
    _lib.check(_lib.lib().nlml_tucker_gradient_r(Wm.data_ptr(), Xp.data_ptr(), 1408, None, Pd.data_ptr(), cpd.data_ptr(), 9, e2.data_ptr(),
                                                 g2.data_ptr(), 5, ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream), "gradient")
    torch.cuda.synchronize()
    e_h9, g_h9 = GC.gradient_host(W, X[:9], P[:9], cp)
    assert np.array_equal(e2.cpu().numpy(), e_h9) and np.array_equal(g2.cpu().numpy(), g_h9)


def test_err_is_the_reference_order_objective(host_draws, tucker_art, device):
    W, P, X, _, _ = host_draws[8]
    cp = GC.cos_block(tucker_art)
    err, _ = _dev_gradient(W, X, P, cp, device)
    want = ops.tucker_objective(torch.from_numpy(W.reshape(-1, 1404)).to(device), torch.from_numpy(X).to(device),
                                torch.from_numpy(P).to(device), torch.from_numpy(cp).to(device), order="reference").cpu().numpy()
    assert np.array_equal(err, want)


def test_device_gradient_is_fx9_bit_for_bit(tucker_art, golden_dir, device):
    W, P, X, g, e = GC.fx9_inputs(tucker_art, golden_dir)
    err, grad = _dev_gradient(W, X, P, GC.cos_block(tucker_art), device)
    assert np.array_equal(grad[:, :3], g[:, :3]) and np.array_equal(err, e)
    assert np.array_equal(grad[:, 3:], g[:, 3:])


@pytest.mark.parametrize("R", [1, 3, 8])
def test_device_gradient_is_fx10_bit_for_bit(R, tucker_art, golden_dir, device):
    W, P, X, g, e = GC.fx10_inputs(tucker_art, golden_dir, R)
    err, grad = _dev_gradient(W, X, P, GC.cos_block(tucker_art), device)
    assert np.array_equal(grad[:, :3], g[:, :3]) and np.array_equal(err, e)
    assert np.array_equal(grad[:, 3:], g[:, 3:])


def test_every_public_form_returns_the_same_bits(host_draws, tucker_art, device):
    from nlml_hpe_amd import TD_Tester as HT
    W, P, X, e_h, g_h = host_draws[3]
    Py, Pp, Pr = RF.cos_rows(tucker_art)
    assert np.array_equal(HT.compute_gradient_batch(P, W, X, Py, Pp, Pr, impl="native"), g_h)
    e, g = HT.value_and_gradient_batch(P, W, X, Py, Pp, Pr)
    assert np.array_equal(e, e_h) and np.array_equal(g, g_h)
    assert np.array_equal(HT.compute_gradient(P[4], W, torch.from_numpy(X[4]), Py, Pp, Pr, impl="native"), g_h[4])
    with pytest.raises(ValueError):
        HT.compute_gradient_batch(P, W, X, Py, Pp, Pr, impl="other")
    lib_path = HT.compute_gradient_batch(P, W, X, Py, Pp, Pr)                 # the default stays the library path
    assert np.abs(lib_path[:, :3] - g_h[:, :3]).max() <= 1e-10 * np.abs(g_h[:, :3]).max()
    cp = GC.cos_block(tucker_art)
    te, tg = torch.ops.nlml_hpe.tucker_gradient(torch.from_numpy(W.reshape(-1, 1404)).to(device), torch.from_numpy(X).to(device),
                                                torch.from_numpy(P).to(device), torch.from_numpy(cp).to(device))
    assert np.array_equal(te.cpu().numpy(), e_h) and np.array_equal(tg.cpu().numpy(), g_h)
    g_only = ops.tucker_gradient(torch.from_numpy(W.reshape(-1, 1404)).to(device), torch.from_numpy(X).to(device),
                                 torch.from_numpy(P).to(device), torch.from_numpy(cp).to(device), return_err=False)
    assert np.array_equal(g_only.cpu().numpy(), g_h)


def test_meta_kernel_shapes():
    m = dict(device="meta")
    e, g = torch.ops.nlml_hpe.tucker_gradient(torch.empty(27 * 8, 1404, **m), torch.empty(7, 1404, **m),
                                              torch.empty(7, 11, dtype=torch.float64, **m), torch.empty(3, 3, 4, dtype=torch.float64, **m))
    assert e.shape == (7,) and g.shape == (7, 11) and e.dtype == g.dtype == torch.float64 and e.device.type == "meta"


def test_device_df_entries_against_libm_over_a_sweep(tucker_art, device):
    """df = float32(((-a) b) sin(b w + c)) on the device (correctly rounded sin) against the host libm's over 1e6 angles and the nine
    shipped cosine rows.  The entry is read out through the gradient itself: rank 1, u = 1, W = 1 at (row 0, column 0) only, pitch and
    roll rows (0, 1, 0, 1) -- f = 1 exactly -- and x[0] = 2^60, so r[0] = 2^60 exactly, every other product is zero and
    grad_w_y = -(2^60 df) with no rounding.  Two libms cannot be forced to agree: the flips are COUNTED; each must be one f32 ulp."""
    rows = GC.cos_block(tucker_art).reshape(9, 4)
    n = 1_000_000 // 9 + 1
    w = np.linspace(-1.6, 1.6, n)
    Wm = torch.zeros((27, 1404), dtype=torch.float32, device=device)
    Wm[0, 0] = 1.0
    x = torch.zeros((1, 1404), dtype=torch.float32, device=device)
    x[0, 0] = 2.0 ** 60
    P = np.zeros((n, 4))
    P[:, 0], P[:, 3] = w, 1.0
    Pd = torch.from_numpy(P).to(device)
    idx = torch.zeros(n, dtype=torch.int32, device=device)
    flips, total = 0, 0
    for row in rows:
        cp = np.zeros((3, 3, 4))
        cp[0, 0] = row
        cp[1, 0] = cp[2, 0] = (0.0, 1.0, 0.0, 1.0)
        got = np.empty(n, np.float32)
        for s in range(0, n, 16384):                                          # (the workspace is ~56 KB per evaluation)
            g = ops.tucker_gradient(Wm, x, Pd[s:s + 16384], torch.from_numpy(cp).to(device), x_index=idx[s:s + 16384], return_err=False)
            g0 = -g[:, 0].cpu().numpy() / 2.0 ** 60
            assert np.array_equal(g0, g0.astype(np.float32).astype(np.float64))   # the read-out is exact
            got[s:s + 16384] = g0
        arg = row[1] * w + row[2]
        ref = ((-row[0] * row[1]) * np.fromiter((math.sin(v) for v in arg), dtype=np.float64, count=n)).astype(np.float32)
        bad = np.nonzero(got != ref)[0]
        flips += len(bad)
        total += n
        assert (np.abs(got[bad].astype(np.float64) - ref[bad]) <= np.spacing(np.abs(ref[bad]))).all()
    print(f"device df against libm: {flips} f32 roundings differ of {total}")
