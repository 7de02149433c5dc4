"""CPU: the yardstick of tests/test_td_powell_edges_gpu.py pinned on its own -- the host state machine (powell_host.minimize_powell,
the code of nlml_hpe_amd/csrc/powell.h that the device runs) against scipy.optimize.minimize(method='Powell') on the faces and starts
of tests/powell_cases.py, at identity ranks 1, 3 and 5 (n = 4, 6 and 8 parameters):

  face / start                                            R = 5 (n = 8)                        R = 3 (n = 6)      R = 1 (n = 4)
  one NaN feature; all NaN; x0[0] = NaN; x0[0] = Inf      status 4, nfev 25, nit 1, x, fun NaN  4, 19, 1           4, 13, 1
  one +Inf feature; one +Inf and one -Inf                 status 2, nfev 8000, nit 320,         2, 6000, 315       2, 4000, 307
                                                          fun +inf, x = x0 = 0
  all-zero row (the "no face" sentinel)                   status 1, nfev 45, nit 1, fun 0, x 0  1, 31, 1           1, 17, 1
  face x 1e30                                             status 1, nfev 25, nit 1, x 0         1, 19, 1           1, 13, 1
  x0 = (3e4, -2e4, 1e5, 0...)                             status 1, nfev 2742, nit 31           1, 796, 13         1, 564, 12

Status is the project's (1 converged, 2 maxfev, 3 maxiter, 4 nan) = scipy's res.status + 1.  STATUS 3 IS NOT PINNED, here or on the
device: with scipy's defaults maxiter = maxfev = 1000 n and an iteration costs at least n evaluations, so maxfev always comes first.

An infinite feature makes the objective +inf at every point, so the run ends at maxfev exactly.  The device tests replay such a face on
the constant +inf; here that replay is shown equal to the replay on the true objective: numpy's (oracle.tucker.objective) at ranks 1
and 3, the plain-C objective in the reference's order (oracle.c_oracle, which is rank 5 only and bit-equal to numpy's, FX4) at rank 5.
"""
import warnings

import numpy as np
import pytest
from scipy.optimize import minimize

import powell_cases as PC
import rank_fixture as RF
from nlml_hpe_amd.powell_host import minimize_powell

RANKS = (1, 3, 5)
NAN_ROWS = ("one_nan", "all_nan", "nan_start", "inf_start")
#          name: {R: (status, nfev, nit)}
TABLE = {
    **{k: {5: (4, 25, 1), 3: (4, 19, 1), 1: (4, 13, 1)} for k in NAN_ROWS},
    **{k: {5: (2, 8000, 320), 3: (2, 6000, 315), 1: (2, 4000, 307)} for k in PC.INF_FACES},
    "zero": {5: (1, 45, 1), 3: (1, 31, 1), 1: (1, 17, 1)},
    "huge": {5: (1, 25, 1), 3: (1, 19, 1), 1: (1, 13, 1)},
    "far_start": {5: (1, 2742, 31), 3: (1, 796, 13), 1: (1, 564, 12)},
}
HUGE_FUN = {5: 3.706545006050772e+60, 3: 3.700488350943967e+60}


def _memo(fun):
    """The same objective for scipy and for the host machine, evaluated once per distinct point."""
    seen = {}

    def f(p):
        key = np.asarray(p, np.float64).tobytes()
        if key not in seen:
            seen[key] = float(fun(np.array(p, np.float64)))
        return seen[key]
    return f


def _scipy(fun, x0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return minimize(fun, x0, method="Powell")


def _case(art, R, name):
    """-> (objective, x0) of a row of the table."""
    n = 3 + R
    if name in PC.bad_starts(R):
        return PC.numpy_objective(art, R, PC.base_face(art, R)), PC.bad_starts(R)[name]
    if name in PC.INF_FACES:
        return PC.constant_inf, np.zeros(n)        # the true objective: test_an_infinite_feature_is_the_constant_inf_objective
    return PC.numpy_objective(art, R, PC.bad_faces(art, R)[name]), np.zeros(n)


@pytest.mark.parametrize("name", sorted(TABLE))
@pytest.mark.parametrize("R", RANKS)
def test_host_machine_is_scipy_on_the_table(R, name, tucker_art):
    fun, x0 = _case(tucker_art, R, name)
    fun = _memo(fun)
    ref = _scipy(fun, x0)
    got = PC.host_run(fun, x0)
    print(f"R={R} {name}: status {got['status']} nfev {got['nfev']} nit {got['nit']} fun {float(got['fun'])!r}; scipy status {ref.status} "
          f"nfev {ref.nfev} nit {ref.nit} fun {float(ref.fun)!r}")
    want = PC.as_outputs(ref.x, ref.fun, ref.nfev, ref.nit, {0: 1, 1: 2, 2: 3, 3: 4}[ref.status])
    assert PC.same_outputs(got, want), PC.differing(got, want)
    assert (int(got["status"]), int(got["nfev"]), int(got["nit"])) == TABLE[name][R]
    if name in NAN_ROWS:
        assert np.isnan(got["x"]).all() and np.isnan(got["fun"]) and int(got["nfev"]) == PC.NAN_NFEV(3 + R)
    elif name in PC.INF_FACES:
        assert got["fun"] == np.inf and not got["x"].any() and int(got["nfev"]) == 1000 * (3 + R)
    elif name == "zero":
        assert got["fun"] == 0.0 and not got["x"].any()
    elif name == "huge":
        assert not got["x"].any() and (R not in HUGE_FUN or float(got["fun"]) == HUGE_FUN[R])
    # what the device tests use is what was checked here
    if name != "far_start" or R != 5:              # (that replay costs seconds: the device test makes its own once)
        assert PC.same_outputs(PC.host_case(tucker_art, R, name), got)


@pytest.mark.parametrize("R", RANKS)
def test_an_infinite_feature_is_the_constant_inf_objective(R, tucker_art):
    """The replay on the true objective of a face with an infinite feature equals the replay on the constant +inf, every trial point
    included.  Ranks 1 and 3: numpy's objective; rank 5: the plain-C objective in the reference's order."""
    const_pts = []
    const = PC.host_run(PC.constant_inf, np.zeros(3 + R), record=const_pts)
    for name in PC.INF_FACES:
        face = PC.bad_faces(tucker_art, R)[name]
        if R == 5:
            from oracle import c_oracle as CO
            Wm, cp = tucker_art["W"].reshape(135, PC.F), np.stack(RF.cos_rows(tucker_art))
            fun = lambda p: float(CO.tucker_objective(Wm, face[None], p[None, :], cp, reference_order=True)[0])
        else:
            fun = PC.numpy_objective(tucker_art, R, face)
        pts = []
        true = PC.host_run(fun, np.zeros(3 + R), record=pts)
        assert PC.same_outputs(true, const), (name, PC.differing(true, const))
        assert len(pts) == len(const_pts) == 1000 * (3 + R) and all(np.array_equal(a, b) for a, b in zip(pts, const_pts)), name
        if R != 1:
            break                                   # (the second face goes the same way; one is 4-6 s of CPU at these ranks)


def test_constant_inf_ends_at_maxfev_for_every_machine_size():
    """nfev / nit of the rank-aware machine on +inf, and the fixed 8-parameter machine beside it."""
    want = {4: (4000, 307), 6: (6000, 315), 8: (8000, 320), 11: (11000, 323), 19: (19000, 327)}
    for n, (nfev, nit) in want.items():
        h = minimize_powell(PC.constant_inf, np.zeros(n), rank_aware=True)
        assert (h.status, h.nfev, h.nit, h.fun) == (2, nfev, nit, np.inf) and not h.x.any(), n
    h = minimize_powell(PC.constant_inf, np.zeros(8))
    assert (h.status, h.nfev, h.nit, h.fun) == (2, 8000, 320, np.inf) and not h.x.any()


@pytest.mark.parametrize("R", [1, 5])
def test_returned_fun_is_the_objective_at_the_returned_point(R, tucker_art):
    """fun == objective(x) bit for bit, on three clean and two noisy faces per rank: the returned x is p + alpha xi, the very point Brent
    evaluated last (nothing in powell.h is contracted into an fma).  The device's wide-batch test leans on this.  Rank 5 runs on the
    plain-C objective in the reference's order (numpy's bits, at a third of the time)."""
    faces = np.concatenate([RF.grid_faces(tucker_art, R)[:3], RF.noisy_faces(tucker_art, R, 2)])
    for i, face in enumerate(faces):
        if R == 5:
            from oracle import c_oracle as CO
            Wm, cp = tucker_art["W"].reshape(135, PC.F), np.stack(RF.cos_rows(tucker_art))
            fun = lambda p, face=face: float(CO.tucker_objective(Wm, face[None], p[None, :], cp, reference_order=True)[0])
        else:
            fun = PC.numpy_objective(tucker_art, R, face)
        h = minimize_powell(fun, np.zeros(3 + R))
        assert h.status == 1 and h.fun == fun(h.x), (R, i, h.nfev)
