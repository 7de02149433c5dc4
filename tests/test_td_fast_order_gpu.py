"""GPU: the TD path's matrix-core ("fast") order -- the default of TD_Inference and the order bench.py times -- pinned bit for bit at
every identity rank against the host statement of that order (oracle_tucker_objective_fast; tests/test_td_fast_order_host.py ties it to
the established rank-5 order and shows that the inputs used here tell wrong orders apart).  There is no tolerance in this file.

  a  objective, every rank   ranks 1, 2, 3, 4 (3, 2, 1, 0 zero-coefficient padding rows; 7, 14, 21, 27 K steps through the three-slot ring),
                             5 (the tuned kernel), 8, 16 (the full 54 KB table) x batches of 1, 15, 16, 17, 37: err and all of x_hat;
  b  the C entry points      shared rows through x_index, ldx = 1408 with NaN pads, a spare row that must survive, x_hat = NULL;
  c  exactly summable data   integers on which any correct kernel returns the int64 answer whatever its summation order: both orders,
                             through x_index -- rests on no model of the order at all;
  d  Powell                  the device minimiser in fast order replays on the host (powell_cases.host_run on the model) at run-time
                             ranks 1, 3, 8 and, at rank 5, in every machine slot and from a far start.
"""
import numpy as np
import pytest
import torch

import cr_reference as CR
import powell_cases as PC
import td_fast_cases as FC
from nlml_hpe_amd import _lib, ops

pytestmark = pytest.mark.gpu
ORDERS = ("reference", "fast")
MARK = -7.25


def _t(a, device):
    return torch.from_numpy(np.array(a, order="C")).to(device)     # (a copy: the shared cases are read-only)


@pytest.fixture(scope="module")
def dev_case(tucker_art, device):
    """R -> (case of td_fast_cases.objective_case, its Wm / X / P / cos_params on the device), made once per rank."""
    memo = {}

    def get(R):
        if R not in memo:
            c = FC.objective_case(tucker_art, R)
            _assert_f_vectors(c)
            memo[R] = (c, {k: _t(c[k], device) for k in ("Wm", "X", "P", "cp")})
        return memo[R]
    return get


# ---- a. the objective at every rank ------------------------------------------------------------------------------------------------

def _assert_f_vectors(c):
    """The model takes its f-vectors from numpy's cos (oracle.tucker.f_vectors), the device from csrc/cr_cos.h.  On these draws the two
    give the same float32s -- checked against tests/cr_reference.py before anything is compared, so that a mismatch below points at
    the order and not at the f-vectors."""
    cp = c["cp"]
    w = c["P"][:, :3, None]
    want = CR.f_entry(cp[None, :, :, 0], cp[None, :, :, 1], w, cp[None, :, :, 2], cp[None, :, :, 3])
    assert want.dtype == np.float32 and want.shape == (FC.N_MAX, 3, 3)
    assert np.array_equal(c["fvec"].astype(np.float32).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(c["fvec"], want.astype(np.float64))


@pytest.mark.parametrize("R", FC.RANKS)
def test_f_vectors_of_the_cases_are_the_correctly_rounded_ones(R, tucker_art):
    _assert_f_vectors(FC.objective_case(tucker_art, R))


@pytest.mark.parametrize("N", FC.BATCHES)
@pytest.mark.parametrize("R", FC.RANKS)
def test_fast_objective_is_the_host_model_bit_for_bit(R, N, dev_case):
    c, d = dev_case(R)
    err, xh = ops.tucker_objective(d["Wm"], d["X"][:N], d["P"][:N], d["cp"], order="fast", return_xhat=True)
    err, xh = err.cpu().numpy(), xh.cpu().numpy()
    ne, nx = FC.mismatches(err, c["err"][:N]), FC.mismatches(xh, c["x_hat"][:N])
    print(f"R={R} N={N}: err mismatches {ne} of {N}, x_hat mismatches {nx} of {xh.size}")
    assert err.shape == (N,) and xh.shape == (N, FC.F)
    assert ne == 0, np.flatnonzero(FC.bits(err) != FC.bits(c["err"][:N]))
    assert nx == 0, np.argwhere(FC.bits(xh) != FC.bits(c["x_hat"][:N]))[:8]


# ---- b. shared rows, stride, untouched memory --------------------------------------------------------------------------------------

def _objective_c(d, device, R, xbuf, ldx, x_index, N, with_xhat, use_r):
    """nlml_tucker_objective_r (or nlml_tucker_objective_ex at rank 5) in fast order on the default stream; err and x_hat have one spare
    row and are pre-filled with MARK -> (err f64[N+1], x_hat f64[N+1,1404] -- all MARK when x_hat is passed as NULL)."""
    err = torch.full((N + 1,), MARK, dtype=torch.float64, device=device)
    xh = torch.full((N + 1, FC.F), MARK, dtype=torch.float64, device=device)
    a = (d["Wm"].data_ptr(), xbuf.data_ptr(), ldx, x_index.data_ptr(), d["P"].data_ptr(), d["cp"].data_ptr(), N, err.data_ptr(),
         xh.data_ptr() if with_xhat else None)
    torch.cuda.synchronize(device)
    L = _lib.lib()
    rc = L.nlml_tucker_objective_r(*a, R, _lib.TD_ORDER_FAST, None) if use_r else L.nlml_tucker_objective_ex(*a, _lib.TD_ORDER_FAST, None)
    assert rc == 0, L.nlml_last_error()
    torch.cuda.synchronize(device)
    return err.cpu().numpy(), xh.cpu().numpy()


@pytest.mark.parametrize("R", [3, 5])
def test_c_entry_point_shared_rows_stride_and_spare_rows(R, tucker_art, dev_case, device):
    s = FC.shared_rows(tucker_art, R)
    _, d = dev_case(R)
    N = FC.N_MAX
    xbuf = _t(FC.padded(s["X7"], 1408, spare_rows=1), device)
    xi = _t(s["x_index"], device)
    for use_r in ((True, False) if R == 5 else (True,)):
        err, xh = _objective_c(d, device, R, xbuf, 1408, xi, N, True, use_r)
        ne, nx = FC.mismatches(err[:N], s["err"]), FC.mismatches(xh[:N], s["x_hat"])
        print(f"R={R} {'_r' if use_r else '_ex'}: err mismatches {ne} of {N}, x_hat mismatches {nx} of {N * FC.F}")
        assert ne == 0 and nx == 0
        assert err[N] == MARK and (xh[N] == MARK).all()
        err0, xh0 = _objective_c(d, device, R, xbuf, 1408, xi, N, False, use_r)
        assert FC.mismatches(err0[:N], s["err"]) == 0 and err0[N] == MARK and (xh0 == MARK).all()


# ---- c. exactly summable inputs, both orders ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", FC.EXACT_RANKS)
@pytest.mark.parametrize("order", ORDERS)
def test_exactly_summable_inputs_give_the_integer_answer(order, R, device):
    """Every product and partial sum is an integer below 2^23, x below 2^24, the sum of squares below 2^53 (asserted from the data): no
    operation rounds, in any order.  A wrong row, column, (j, k, l) decoding, padding row, ring slot, dead-column mask or clamped tail
    row gives another integer."""
    c = FC.exact_case(R)
    assert c["abs_sum"].max() < 2 ** 23 and np.abs(c["X_int"]).max() < 2 ** 24 and c["ss"].max() < 2 ** 53
    assert np.array_equal(c["X"].astype(np.int64), c["X_int"]) and np.array_equal(c["Wm"].astype(np.int64), np.rint(c["Wm"]).astype(np.int64))
    assert np.array_equal(c["err"] * 2, c["ss"].astype(np.float64)) and c["err"].max() <= 0.5 * FC.F * 1000 ** 2
    Wm, cp = _t(c["Wm"], device), _t(c["cp"], device)
    for N in FC.EXACT_BATCHES:
        buf, xi = FC.exact_batch(c, N)
        err, xh = ops.tucker_objective(Wm, _t(buf, device), _t(c["P"][:N], device), cp, x_index=_t(xi, device), order=order, return_xhat=True)
        err, xh = err.cpu().numpy(), xh.cpu().numpy()
        ne, nx = FC.mismatches(err, c["err"][:N]), FC.mismatches(xh, c["x_hat"][:N])
        print(f"{order} R={R} N={N}: err mismatches {ne} of {N}, x_hat mismatches {nx} of {xh.size}; largest err {c['err'][:N].max():.4g}")
        assert ne == 0, (N, err, c["err"][:N])
        assert nx == 0, (N, np.argwhere(FC.bits(xh) != FC.bits(c["x_hat"][:N]))[:8])


# ---- d. Powell in fast order replays on the host -----------------------------------------------------------------------------------

def _powell(Wm, faces, cp, x0, device):
    res = ops.tucker_powell(Wm, _t(faces, device), cp, x0=_t(x0, device), order="fast")
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("R", FC.POWELL_RANKS)
def test_fast_powell_replays_on_the_host_at_run_time_ranks(R, tucker_art, dev_case, device):
    """tucker_powell_kernel<FAST, TdRankDyn>: two grid faces from zeros and one from a start, each replayed by the host machine on the
    model objective: x, fun, nfev, nit and status bit for bit."""
    c, d = dev_case(R)
    faces, x0 = FC.powell_runs(tucker_art, R)
    res = _powell(d["Wm"], faces, d["cp"], x0, device)
    for i in range(len(faces)):
        want = PC.host_run(FC.model_objective(c["Wm"], c["cp"], faces[i]), x0[i])
        got = PC.row(res, i)
        print(f"R={R} face {i}: device nfev {got['nfev']} nit {got['nit']} status {got['status']}; host nfev {want['nfev']} nit {want['nit']}; "
              f"differing outputs {PC.differing(got, want)}")
        assert PC.same_outputs(got, want), (i, PC.differing(got, want), got, want)
        assert int(got["status"]) == 1


def test_fast_powell_at_rank_five_replays_in_every_machine_slot(tucker_art, dev_case, device):
    """17 faces with x0 = one workgroup + 1, three (face, start) pairs in turn: each pair is replayed once on the host and every one of
    the 17 machines is held to it."""
    c, d = dev_case(5)
    faces, x0, pairs = FC.powell_rank5_batch(tucker_art)
    res = _powell(d["Wm"], faces, d["cp"], x0, device)
    host = [PC.host_run(FC.model_objective(c["Wm"], c["cp"], faces[j]), x0[j]) for j in range(3)]
    print(f"host nfev {[int(h['nfev']) for h in host]}, device nfev {res['nfev'].tolist()}")
    for i in range(len(faces)):
        got, want = PC.row(res, i), host[pairs[i]]
        assert PC.same_outputs(got, want), (i, PC.differing(got, want), got, want)
    assert (res["status"] == 1).all()


def test_fast_powell_at_rank_five_replays_from_a_far_start(tucker_art, dev_case, device):
    """x0 = (3e4, -2e4, 1e5, 0...): one live machine, so the run goes through the one-evaluation pass (tucker_few<1>) with the f-vectors'
    arguments up to 2.9e5."""
    c, d = dev_case(5)
    face = PC.base_face(tucker_art, 5)
    x0 = PC.bad_starts(5)["far_start"]
    got = PC.row(_powell(d["Wm"], face[None], d["cp"], x0[None], device), 0)
    want = PC.host_run(FC.model_objective(c["Wm"], c["cp"], face), x0)
    print(f"device nfev {got['nfev']} nit {got['nit']} status {got['status']}; host nfev {want['nfev']} nit {want['nit']}")
    assert PC.same_outputs(got, want), (PC.differing(got, want), got, want)
    assert int(got["status"]) == 1 and np.abs(got["x"][:3]).min() > 1.9e4
