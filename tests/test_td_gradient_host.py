"""CPU: K3g's host restatement (nlml_tucker_gradient_host, csrc/tucker_grad_ref.h) against the reference's compute_gradient
(TD_Tester.py:60-102): FX9 (the FX4 inputs, rank 5), FX10 (ranks 1, 3, 8) and oracle.tucker.compute_gradient -- the reference's own
numpy calls -- on 200 draws per rank in {1, 5, 16}.  EVERY component is held to equal bits, the identity part included: the order of
numpy's two-operand reduction 'ijklm,m->i' was established (buffered iterator, chunks of 8192 elements, two-lane inner loop; the header
has it), so there is no tolerance anywhere in this file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import td_gradient_common as GC
from nlml_hpe_amd import _lib
from oracle import tucker as TK

E_BADARG, E_SHAPE = -1, -3


def test_host_gradient_is_fx9_bit_for_bit(tucker_art, golden_dir):
    W, P, X, g, e = GC.fx9_inputs(tucker_art, golden_dir)
    err, grad = GC.gradient_host(W, X, P, GC.cos_block(tucker_art))
    print(f"FX9: {len(P)} sets; angle mismatches {int((grad[:, :3] != g[:, :3]).sum())}, identity mismatches "
          f"{int((grad[:, 3:] != g[:, 3:]).sum())}, err mismatches {int((err != e).sum())}")
    assert np.array_equal(grad[:, :3], g[:, :3])
    assert np.array_equal(err, e)                       # FX4's objective bits
    assert np.array_equal(grad[:, 3:], g[:, 3:])


@pytest.mark.parametrize("R", [1, 3, 8])
def test_host_gradient_is_fx10_bit_for_bit(R, tucker_art, golden_dir):
    W, P, X, g, e = GC.fx10_inputs(tucker_art, golden_dir, R)
    err, grad = GC.gradient_host(W, X, P, GC.cos_block(tucker_art))
    assert np.array_equal(grad[:, :3], g[:, :3])
    assert np.array_equal(err, e)
    assert np.array_equal(grad[:, 3:], g[:, 3:])


@pytest.mark.parametrize("R", GC.DRAW_RANKS)
def test_host_gradient_equals_the_oracle_on_200_draws(R, tucker_art):
    """oracle.tucker.compute_gradient is the reference's numpy calls; the f32 einsum v of the identity term is pinned on its own."""
    W, P, X = GC.draws(tucker_art, R)
    cp = GC.cos_block(tucker_art)
    err, grad, v = GC.gradient_host(W, X, P, cp, want_v=True)
    G = np.stack([TK.compute_gradient(p, W, x, cp[0], cp[1], cp[2]) for p, x in zip(P, X)])
    V = np.stack([np.einsum('ijklm,j,k,l->m', W, *TK.f_vectors(p, cp[0], cp[1], cp[2])) for p in P])
    E = np.array([TK.objective(p, W, x, cp[0], cp[1], cp[2]) for p, x in zip(P[:16], X[:16])])
    print(f"R={R}: angle mismatches {int((grad[:, :3] != G[:, :3]).sum())}, identity {int((grad[:, 3:] != G[:, 3:]).sum())}, "
          f"v {int((v != V).sum())} of {v.size}")
    assert V.dtype == np.float32 and np.array_equal(v, V)          # step 5: numpy runs 'ijklm,j,k,l->m' in f32
    assert np.array_equal(grad[:, :3], G[:, :3])
    assert np.array_equal(err[:16], E)
    assert np.array_equal(grad[:, 3:], G[:, 3:])


def test_host_gradient_takes_x_index_and_a_padded_row_stride(tucker_art):
    W, P, X = GC.draws(tucker_art, 5, 6)
    cp = GC.cos_block(tucker_art)
    want = GC.gradient_host(W, X, P, cp)
    Xp = np.zeros((3, 1408), np.float32)
    Xp[:, :1404] = X[[4, 0, 2]]
    idx = np.array([1, 1, 2, 2, 0, 0], np.int32)
    got = GC.gradient_host(W, Xp, P, cp, x_index=idx, ldx=1408)
    sel = GC.gradient_host(W, X[[0, 0, 2, 2, 4, 4]], P, cp)
    assert np.array_equal(got[0], sel[0]) and np.array_equal(got[1], sel[1])
    assert np.array_equal(want[1][[0, 2, 4]], got[1][[0, 2, 4]])


def _build(tmp_path, repo_root):
    so = tmp_path / "crsin.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so),
                    os.path.join(repo_root, "tests", "native", "cr_sin_host.cpp")], check=True, capture_output=True, text=True)
    return C.CDLL(str(so))


def test_cr_sin_is_correctly_rounded(tmp_path, repo_root):
    """cr_sin (csrc/cr_cos.h) as tests/test_abi_and_host.py checks cr_cos: never more than one ulp from libm; where the two differ,
    60-digit decimal arithmetic says cr_sin is the closer one; a random sample is within half an ulp of the exact value."""
    import math
    from decimal import Decimal, getcontext
    lib = _build(tmp_path, repo_root)
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(-10, 10, 400_000), rng.uniform(-1e5, 1e5, 40_000),
                        np.array([0.0, 1e-300, -1e-9, np.pi / 2, np.pi, 1.5 * np.pi, -np.pi / 2, 7.0, np.inf, np.nan])])
    y = np.empty_like(x)
    lib.cr_sin_array(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), C.c_long(len(x)))
    ref = np.fromiter((math.sin(v) for v in x[:-2]), dtype=np.float64, count=len(x) - 2)
    assert np.isnan(y[-2:]).all()
    y = y[:-2]
    assert (np.abs(y - ref) <= np.spacing(np.abs(ref))).all()
    differ = np.nonzero(y != ref)[0]
    assert len(differ) <= 5e-3 * len(ref)
    from cr_reference import decimal_sin as exact_sin                               # the 70-digit series (tests/cr_reference.py)
    getcontext().prec = 70

    for i in differ[:100]:
        t = exact_sin(float(x[i]))
        assert abs(Decimal(float(y[i])) - t) <= abs(Decimal(float(ref[i])) - t), x[i]
    for i in rng.integers(0, len(y), 300):
        t = exact_sin(float(x[i]))
        assert abs(Decimal(float(y[i])) - t) <= Decimal(float(np.spacing(abs(y[i])))) / 2, x[i]


def test_derivative_entry_fast_form_equals_the_correctly_rounded_one(tmp_path, repo_root):
    """cr_f32_nab_sin returns float32(((-a) b) sin(t)) from the library sin wherever the float cannot depend on the sin's last bits
    and from the double-double sin otherwise: the same float as the slow path alone on 2 M values."""
    lib = _build(tmp_path, repo_root)
    rng = np.random.default_rng(6)
    n = 1_000_000
    a = np.concatenate([rng.uniform(-12, 12, n), rng.uniform(-12, 12, n)])
    b = np.concatenate([rng.uniform(-3, 3, n), rng.uniform(0.4, 3, n)])
    t = np.concatenate([rng.uniform(-10, 10, n), rng.uniform(-3.5, 3.5, n)])
    fast, slow = np.empty(len(a), np.float32), np.empty(len(a), np.float32)
    P = lambda v: v.ctypes.data_as(C.c_void_p)
    lib.cr_dfvalue_arrays(P(a), P(b), P(t), P(fast), P(slow), C.c_long(len(a)))
    assert np.array_equal(fast.view(np.uint32), slow.view(np.uint32))


def test_gradient_entry_points_refuse_bad_arguments():
    """The K3 error codes, checked before any launch (fake device addresses do on the CPU)."""
    lib = _lib.lib()
    A = 0x1000
    ws = lib.nlml_tucker_gradient_workspace_bytes(5, 5)
    assert ws > 0 and lib.nlml_tucker_gradient_workspace_bytes(0, 5) == 0
    assert lib.nlml_tucker_gradient_workspace_bytes(5, 0) == 0 and lib.nlml_tucker_gradient_workspace_bytes(5, 17) == 0
    assert lib.nlml_tucker_gradient_workspace_bytes(9, 5) > ws

    def dev(r_id=5, ldx=1404, grad=A, ws_ptr=A, ws_bytes=ws, N=5, Wm=A):
        return lib.nlml_tucker_gradient_r(Wm, A, ldx, None, A, A, N, A, grad, r_id, ws_ptr, ws_bytes, None)

    def host(r_id=5, ldx=1404, grad=A, N=5):
        return lib.nlml_tucker_gradient_host(A, A, ldx, None, A, A, N, A, grad, r_id, None)

    for f in (dev, host):
        assert f(r_id=0) == E_SHAPE and f(r_id=17) == E_SHAPE
        assert b"identity rank" in lib.nlml_last_error()
        assert f(ldx=1403) == E_BADARG
        assert f(grad=None) == E_BADARG
        assert f(N=-1) == E_BADARG
    assert dev(ws_bytes=ws - 8) == E_BADARG and b"workspace" in lib.nlml_last_error()
    assert dev(ws_ptr=None) == E_BADARG
    assert dev(Wm=None) == E_BADARG
    assert dev(N=0, ws_bytes=0, ws_ptr=None) == 0 and host(N=0) == 0
    assert lib.nlml_abi_version() == 2
