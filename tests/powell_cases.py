"""Test helper: the faces, starts and batches that take the Powell minimiser (nlml_hpe_amd/csrc/powell.h, tucker_powell.hip) off its
happy path, and the host machine's answers for them.  Deterministic data preparation on top of tests/rank_fixture.py; no test here.

  bad_faces     the base face (rank_fixture.grid_faces(art, R)[0]) with non-finite, zero or huge features;
  bad_starts    starting points with a NaN, an Inf, or far outside the f-vectors' usual argument range;
  nan_face      all NaN: its machine stops after 1 + 3 n evaluations (the start, then the three bracket points along each of the
                n directions of the first iteration) with status 4 -- the tool for emptying chosen machine slots of a workgroup
                early;
  mixed_batch   real, distinct faces at chosen slots, nan_face() in every other;
  replicas      k copies of one face.
The host answers come from powell_host.minimize_powell (the state machine the device runs, checked against scipy step for step in
tests/test_powell_sm.py and tests/test_td_powell_edges_host.py) on numpy's objective (oracle.tucker.objective), and for a face with an
infinite feature on the constant +inf that objective is there (tests/test_td_powell_edges_host.py shows the two replays equal).
"""
from __future__ import annotations

import numpy as np

import rank_fixture as RF
from test_centroid_host import same_bits   # noqa: F401  (any NaN equals any NaN; re-exported for the two test modules)

F = 1404
EV = 16                                      # faces per workgroup (machine slots)
FAR_START = (3e4, -2e4, 1e5)                 # radians: |b w + c| up to 2.93e5 < 2^20 along the run (cr_cos.h's own reduction)
OUTPUTS = ("x", "fun", "nfev", "nit", "status")
NAN_NFEV = lambda n: 1 + 3 * n               # evaluations a machine spends on an objective that is NaN everywhere


def base_face(art: dict, R: int) -> np.ndarray:
    return RF.grid_faces(art, R)[0].copy()


def nan_face() -> np.ndarray:
    return np.full(F, np.nan, np.float32)


def bad_faces(art: dict, R: int) -> dict:
    """name -> f32[1404].  The names are the rows of the table in tests/test_td_powell_edges_host.py."""
    f = base_face(art, R)
    out = {}
    out["one_nan"] = f.copy()
    out["one_nan"][700] = np.nan
    out["all_nan"] = nan_face()
    out["one_inf"] = f.copy()
    out["one_inf"][700] = np.inf
    out["inf_both_signs"] = f.copy()
    out["inf_both_signs"][100] = np.inf
    out["inf_both_signs"][900] = -np.inf
    out["zero"] = np.zeros(F, np.float32)    # the "no face" sentinel row
    out["huge"] = (f * np.float32(1e30)).astype(np.float32)
    assert np.isfinite(out["huge"]).all()
    return out


INF_FACES = ("one_inf", "inf_both_signs")


def bad_starts(R: int) -> dict:
    """name -> f64[3+R], to be run on base_face."""
    n = 3 + R
    out = {k: np.zeros(n) for k in ("nan_start", "inf_start", "far_start")}
    out["nan_start"][0] = np.nan
    out["inf_start"][0] = np.inf
    out["far_start"][:3] = FAR_START
    return out


POOL = 16
_POOL = {}


def ordinary_faces(art: dict, R: int, count: int) -> np.ndarray:
    """count distinct real faces f32[count,1404]: the four clean grid faces, then noisy ones (their evaluation counts differ, so the
    live set of a workgroup that holds them shrinks one machine at a time)."""
    if R not in _POOL:                       # one pool per rank: face i is the same face whatever count is asked for
        _POOL[R] = np.ascontiguousarray(np.concatenate([RF.grid_faces(art, R), RF.noisy_faces(art, R, POOL - len(RF.PICKS))]))
    assert count <= POOL
    return _POOL[R][:count].copy()


def mixed_batch(art: dict, R: int, live_slots, N: int):
    """-> (faces f32[N,1404], which): ordinary face which[i] at live_slots[i] (ascending), nan_face() everywhere else."""
    live = sorted(live_slots)
    assert len(set(live)) == len(live) and 0 <= live[0] and live[-1] < N
    X = np.tile(nan_face(), (N, 1))
    X[live] = ordinary_faces(art, R, len(live))
    return X, list(range(len(live)))


def replicas(face: np.ndarray, k: int) -> np.ndarray:
    return np.ascontiguousarray(np.tile(np.asarray(face, np.float32), (k, 1)))


# ---- the host machine's answers ------------------------------------------------------------------------------------------------

def numpy_objective(art: dict, R: int, face: np.ndarray):
    from oracle import tucker as TK
    W = RF.rank_W(art["W"], R)
    Py, Pp, Pr = RF.cos_rows(art)
    x = np.asarray(face, np.float32)

    def fun(p):
        with np.errstate(all="ignore"):
            return TK.objective(p, W, x, Py, Pp, Pr)
    return fun


def constant_inf(_p):
    return np.inf


def host_run(fun, x0, record=None):
    """minimize_powell with the machine the device runs for that many parameters -> dict of OUTPUTS, typed as the device's."""
    from nlml_hpe_amd.powell_host import minimize_powell
    h = minimize_powell(fun, np.asarray(x0, np.float64), record=record)
    return as_outputs(h.x, h.fun, h.nfev, h.nit, h.status)


def as_outputs(x, fun, nfev, nit, status) -> dict:
    return {"x": np.asarray(x, np.float64), "fun": np.float64(fun), "nfev": np.int32(nfev), "nit": np.int32(nit),
            "status": np.int32(status)}


_HOST = {}


def host_case(art: dict, R: int, name: str) -> dict:
    """The host machine's outputs for bad face / bad start `name` at rank R (computed once per process)."""
    if (R, name) not in _HOST:
        n = 3 + R
        if name in INF_FACES:
            out = host_run(constant_inf, np.zeros(n))
        elif name in bad_starts(R):
            out = host_run(numpy_objective(art, R, base_face(art, R)), bad_starts(R)[name])
        else:
            out = host_run(numpy_objective(art, R, bad_faces(art, R)[name]), np.zeros(n))
        _HOST[(R, name)] = out
    return _HOST[(R, name)]


def row(res: dict, i: int) -> dict:
    """Face i of a batch's outputs."""
    return {k: np.asarray(res[k])[i] for k in OUTPUTS}


def same_outputs(a: dict, b: dict) -> bool:
    """All five outputs equal bit for bit (any NaN equals any NaN)."""
    return all(same_bits(np.asarray(a[k]), np.asarray(b[k])) for k in OUTPUTS)


def differing(a: dict, b: dict) -> list:
    return [k for k in OUTPUTS if not same_bits(np.asarray(a[k]), np.asarray(b[k]))]
