"""CPU: the host statement of the TD path's matrix-core ("fast") order for every identity rank (oracle_tucker_objective_fast,
oracle/csrc/oracle.c) -- the yardstick of tests/test_td_fast_order_gpu.py -- tied to what is already established, and the inputs of
tests/td_fast_cases.py shown to tell wrong orders apart:

  1  rank 5 anchor      on FX4's inputs and on rank_fixture's, err and x_hat are the bits of oracle_tucker_objective(device_order=1), the
                        rank-5 model that the device has matched on hardware since tests/test_gpu_parity.py pinned it;
  2  every rank         within the project's 1e-12 of scale of numpy's einsum (oracle.tucker);
  3  the inputs work    at every rank the model's x_hat differs in bits from the einsum's in at least a quarter of the entries, and each
                        deliberately wrong order (variants 1..5) changes the result on the very inputs the GPU test runs;
  4  stride and index   ldx = 1408 with NaN pads and shared rows through x_index: the bits of the gathered contiguous call.
"""
import os

import numpy as np
import pytest

import rank_fixture as RF
import td_fast_cases as FC
from oracle import c_oracle as CO
from oracle import tucker as TK


@pytest.fixture(scope="module")
def einsum(tucker_art):
    """R -> (err f64[37], x_hat f64[37,1404]) of numpy's own einsum on objective_case's draws, made once per rank."""
    memo = {}

    def get(R):
        if R not in memo:
            c = FC.objective_case(tucker_art, R)
            Py, Pp, Pr = c["cp"]
            memo[R] = (np.array([TK.objective(p, c["W"], x, Py, Pp, Pr) for p, x in zip(c["P"], c["X"])]),
                       np.stack([TK.x_hat(p, c["W"], Py, Pp, Pr) for p in c["P"]]))
        return memo[R]
    return get


def test_rank_five_is_the_established_device_order(tucker_art, golden_dir):
    f4 = np.load(os.path.join(golden_dir, "fx4_td_objective.npz"))
    cp = FC.cos_params(tucker_art)
    Wm5 = np.ascontiguousarray(tucker_art["W"]).reshape(135, FC.F)
    c = FC.objective_case(tucker_art, 5)
    assert np.array_equal(c["Wm"], Wm5)
    P32, X32 = RF.params(5), RF.noisy_faces(tucker_art, 5, 32)
    for name, X, P in (("FX4", f4["x"], f4["params"]), ("rank_fixture 32", X32, P32), ("td_fast_cases 37", c["X"], c["P"])):
        want_e, want_x = CO.tucker_objective(Wm5, X, P, cp, want_xhat=True, device_order=True)
        got_e, got_x = CO.tucker_objective_fast(Wm5, X, P, cp, want_xhat=True)
        print(f"{name}: err mismatches {FC.mismatches(got_e, want_e)} of {len(want_e)}, x_hat mismatches {FC.mismatches(got_x, want_x)}")
        assert FC.mismatches(got_e, want_e) == 0 and FC.mismatches(got_x, want_x) == 0
    assert FC.mismatches(c["err"], want_e) == 0 and FC.mismatches(c["x_hat"], want_x) == 0   # the stored answers of the shared case


@pytest.mark.parametrize("R", FC.RANKS)
def test_every_rank_is_within_1e12_of_the_einsum_and_not_its_bits(R, tucker_art, einsum):
    c = FC.objective_case(tucker_art, R)
    want_e, want_x = einsum(R)
    rel = float(np.max(np.abs(c["err"] - want_e) / np.abs(want_e)))
    xrel = float(np.abs(c["x_hat"] - want_x).max() / np.abs(want_x).max())
    frac = FC.mismatches(c["x_hat"], want_x) / want_x.size
    print(f"R={R}: err rel {rel:.2e}, x_hat rel of scale {xrel:.2e}; x_hat differs in bits from the einsum's in {100 * frac:.1f} % of the "
          f"entries, err in {FC.mismatches(c['err'], want_e)} of {len(want_e)}")
    assert rel <= 1e-12 and xrel <= 1e-12
    assert frac >= 0.25


@pytest.mark.parametrize("R", FC.RANKS)
def test_wrong_orders_show_on_the_gpu_tests_inputs(R, tucker_art):
    """Variants 3 and 4 re-order or extend the residual sum alone: x_hat is the model's by construction, and err must change.  Every
    other variant must change at least one err and at least one x_hat value -- at every batch size the GPU test runs, the smallest
    (evaluation 1 of 37; evaluation 0 is the all-zero start, where x_hat = 0 in any order) included."""
    c = FC.objective_case(tucker_art, R)
    for v, what in FC.VARIANTS.items():
        e, xh = CO.tucker_objective_fast(c["Wm"], c["X"], c["P"], c["cp"], want_xhat=True, variant=v, fvec=c["fvec"])
        ne, nx = FC.mismatches(e, c["err"]), FC.mismatches(xh, c["x_hat"])
        big = max(np.max(np.abs(e - c["err"]) / np.abs(c["err"])), np.abs(xh - c["x_hat"]).max() / np.abs(c["x_hat"]).max())
        print(f"R={R} variant {v} ({what}): err changes in {ne} of {FC.N_MAX}, x_hat in {nx} of {xh.size}; largest change {big:.1e} relative "
              f"(the suite's tolerance for this order was 1e-12)")
        assert ne >= 1
        if v in FC.ERR_ONLY:
            assert nx == 0
        else:
            assert nx >= 1
            # ... and already in the batch of one evaluation that carries a face's worth of coefficients (N = 1 is the zero start)
            assert FC.mismatches(xh[1], c["x_hat"][1]) >= 1
    assert not c["P"][0].any() and not c["x_hat"][0].any()


@pytest.mark.parametrize("R", [1, 3, 5, 16])
def test_row_stride_and_shared_rows_give_the_gathered_bits(R, tucker_art):
    s = FC.shared_rows(tucker_art, R)
    buf = FC.padded(s["X7"], 1408, spare_rows=1)
    e, xh = CO.tucker_objective_fast(s["Wm"], buf, s["P"], s["cp"], x_index=s["x_index"], ldx=1408, want_xhat=True)
    assert np.isfinite(e).all() and np.isfinite(xh).all()
    assert FC.mismatches(e, s["err"]) == 0 and FC.mismatches(xh, s["x_hat"]) == 0
    c = FC.objective_case(tucker_art, R)
    assert FC.mismatches(xh, c["x_hat"]) == 0        # x_hat does not depend on the face
    assert FC.mismatches(e[1:], c["err"][1:]) > 0     # ... err does: only evaluation 0 keeps its own face
    one = CO.tucker_objective_fast(s["Wm"], buf, s["P"][5:6], s["cp"], x_index=s["x_index"][5:6], ldx=1408)
    assert FC.mismatches(one, s["err"][5:6]) == 0
    with pytest.raises(IndexError):
        CO.tucker_objective_fast(s["Wm"], buf, s["P"], s["cp"], x_index=s["x_index"] + 2, ldx=1408)


@pytest.mark.parametrize("R", FC.EXACT_RANKS)
def test_exactly_summable_inputs_on_the_host(R):
    """The integer case of the GPU test on the two host objectives: its bounds hold, and the model and numpy's einsum both return the
    int64 answer exactly (a first check of the case itself, and of the model where no order matters)."""
    c = FC.exact_case(R)
    assert c["abs_sum"].max() < 2 ** 23 and np.abs(c["X_int"]).max() < 2 ** 24 and c["ss"].max() < 2 ** 53
    assert np.array_equal(c["X"].astype(np.int64), c["X_int"])
    print(f"R={R}: largest sum of |products| {c['abs_sum'].max()}, |x| {np.abs(c['X_int']).max()}, err {c['err'].max():.4g}")
    for N in FC.EXACT_BATCHES:
        buf, xi = FC.exact_batch(c, N)
        assert sorted(xi.tolist()) == list(range(2, 2 + N)) and np.isnan(buf[:2]).all()
        e, xh = CO.tucker_objective_fast(c["Wm"], buf, c["P"][:N], c["cp"], x_index=xi, want_xhat=True)
        assert FC.mismatches(e, c["err"][:N]) == 0 and FC.mismatches(xh, c["x_hat"][:N]) == 0
    Py, Pp, Pr = c["cp"]
    W = c["Wm"].reshape(R, 3, 3, 3, FC.F)
    for n in (0, 36):
        assert TK.objective(c["P"][n], W, c["X"][n], Py, Pp, Pr) == c["err"][n]
        assert np.array_equal(TK.x_hat(c["P"][n], W, Py, Pp, Pr), c["x_hat"][n])
