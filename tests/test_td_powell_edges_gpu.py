"""GPU: the device Powell kernel (nlml_tucker_powell*, nlml_hpe_amd/csrc/tucker_powell.hip) off its happy path.  Every comparison is
bit for bit (powell_cases.same_bits: any NaN equals any NaN); there is no tolerance in this file.

  1  abnormal exits     faces with NaN / Inf / zero / huge features and NaN / Inf starts next to ordinary faces: status 4 and 2, the
                        write-out of a machine that hit maxfev, the round cap; x, fun, nfev, nit, status = the host machine's
                        (tests/test_td_powell_edges_host.py pins that machine on the same cases against scipy);
  2  live count held    k replicas of one face: the whole run goes through ONE round form -- tucker_few<1> (k = 1), tucker_mfma4 with
                        2, 3, 4 live, tucker_round16 (5, 16); reference order: every pass size and partition;
  3  sparse live masks  real faces at chosen machine slots, NaN faces (gone after 1 + 3 n evaluations) in all others;
  4  the C entry point  ldx != 1404 with NaN in the pad columns, each optional output NULL, nothing written past row N - 1;
  5  far starts         x0 = (3e4, -2e4, 1e5, 0...): cr_cos.h's double-double reduction at k ~ 1.9e5 inside the kernel (host replays:
                        reference order here, fast order in tests/test_td_fast_order_gpu.py, which also replays ordinary fast-order runs
                        on the host's matrix-core objective at ranks 1, 3, 5, 8);
  6  wide batch         645 faces = 40 workgroups + 5: fun == the objective at the returned x, and reversal.

Deliberately NOT pinned: status 3 (maxiter) -- unreachable with the fixed limits maxiter = maxfev = 1000 n, since an iteration costs
at least n evaluations and maxfev comes first; and starts that take |b w + c| beyond 2^20, where cr_cos.h hands over to the library cos
on either side.  Identity rank 16 on an Inf face (19,000 rounds) is out of scope.
"""
import os
import time

import numpy as np
import pytest
import torch

import powell_cases as PC
import rank_fixture as RF
from nlml_hpe_amd import _lib, ops

pytestmark = pytest.mark.gpu
ORDERS = ("reference", "fast")
ORDER_ID = {"reference": _lib.TD_ORDER_REFERENCE, "fast": _lib.TD_ORDER_FAST}


class _Dev:
    """The device operands per rank and the solo runs (one face, one launch) the batches are compared with, each made once."""

    def __init__(self, art, device):
        self.art, self.device = art, device
        self._wm, self._solo = {}, {}
        self.cp = torch.from_numpy(np.stack(RF.cos_rows(art))).to(device)

    def wm(self, R):
        if R not in self._wm:
            self._wm[R] = torch.from_numpy(RF.rank_W(self.art["W"], R).reshape(-1, PC.F)).to(self.device)
        return self._wm[R]

    def run(self, R, order, X, x0=None, timed=None):
        X = torch.from_numpy(np.ascontiguousarray(X, np.float32)).to(self.device)
        x0 = None if x0 is None else torch.from_numpy(np.ascontiguousarray(x0, np.float64)).to(self.device)
        torch.cuda.synchronize(self.device)
        t = time.perf_counter()
        res = ops.tucker_powell(self.wm(R), X, self.cp, x0=x0, order=order)
        torch.cuda.synchronize(self.device)
        if timed is not None:
            print(f"{timed}: {1e3 * (time.perf_counter() - t):.1f} ms wall")
        return {k: v.cpu().numpy() for k, v in res.items()}

    def solo(self, R, order, i):
        """Ordinary face i of powell_cases.ordinary_faces alone in a launch, from zeros."""
        if (R, order, i) not in self._solo:
            self._solo[(R, order, i)] = PC.row(self.run(R, order, PC.ordinary_faces(self.art, R, i + 1)[i:i + 1]), 0)
        return self._solo[(R, order, i)]


@pytest.fixture(scope="module")
def dev(tucker_art, device):
    return _Dev(tucker_art, device)


def _assert_dead(res, i, n):
    """A NaN face: status 4 after 1 + 3 n evaluations and one iteration, NaN everywhere."""
    assert int(res["status"][i]) == 4 and int(res["nfev"][i]) == PC.NAN_NFEV(n) and int(res["nit"][i]) == 1, i
    assert np.isnan(res["x"][i]).all() and np.isnan(res["fun"][i]), i


# ---- 1. abnormal exits -----------------------------------------------------------------------------------------------------------

#           slot: a bad face's name, or the index of an ordinary face.  One full workgroup + 1; the two Inf faces keep the first
#           workgroup at two live machines for most of its 1000 n rounds, the huge face is alone in the second.
LAYOUT = (0, "one_nan", 1, "one_inf", "all_nan", 2, "zero", "inf_both_signs", 3, "huge", 4, "one_nan", 5, "all_nan", 6, "zero", "huge")


@pytest.mark.parametrize("R", [5, 3, 1])
@pytest.mark.parametrize("order", ORDERS)
def test_abnormal_exits_next_to_ordinary_faces(order, R, dev):
    n = 3 + R
    bad, good = PC.bad_faces(dev.art, R), PC.ordinary_faces(dev.art, R, 7)
    X = np.stack([bad[s] if isinstance(s, str) else good[s] for s in LAYOUT])
    assert len(X) == PC.EV + 1
    res = dev.run(R, order, X, timed=f"R={R} {order}: 17 faces, two of them with an Inf feature")
    print(f"status {res['status'].tolist()} nfev {res['nfev'].tolist()} nit {res['nit'].tolist()}")
    assert (res["status"] != 0).all()                       # PW_RUNNING never escapes
    for i, s in enumerate(LAYOUT):
        got = PC.row(res, i)
        if not isinstance(s, str):
            assert PC.same_outputs(got, dev.solo(R, order, s)), (i, s, PC.differing(got, dev.solo(R, order, s)))
        elif order == "fast" and s in ("zero", "huge"):
            # Finite objective values on the matrix cores: first the solo run, which holds whatever the objective's last bits are; then
            # the host replay on numpy's objective.  On the huge face x_hat is below the last place of x, so the objective is one
            # constant and the path is the host's in any order; on the zero face the objective is 0 wherever u_id is 0 and the
            # path hangs on the bits of a handful of values along the u_id directions, which the two orders have been seen to share.
            one = PC.row(dev.run(R, order, X[i:i + 1]), 0)
            want = PC.host_case(dev.art, R, s)
            print(f"slot {i} {s}: differs from the host replay on numpy's objective in {PC.differing(got, want)}")
            assert PC.same_outputs(got, one) and int(got["status"]) == 1, (i, s, PC.differing(got, one))
            assert not got["x"].any() and (s == "huge" or got["fun"] == 0.0)
            assert PC.same_outputs(got, want), (i, s, PC.differing(got, want), got, want)
        else:
            want = PC.host_case(dev.art, R, s)
            assert PC.same_outputs(got, want), (i, s, PC.differing(got, want), got, want)
    inf = [i for i, s in enumerate(LAYOUT) if s in PC.INF_FACES]
    assert all(int(res["status"][i]) == 2 and int(res["nfev"][i]) == 1000 * n and res["fun"][i] == np.inf and not res["x"][i].any()
               for i in inf)


@pytest.mark.parametrize("R", [5, 3])
@pytest.mark.parametrize("order", ORDERS)
def test_nan_and_inf_starts(order, R, dev):
    n = 3 + R
    starts = PC.bad_starts(R)
    near = np.array([0.1, -0.05, 0.02] + [0.01] * R)
    x0 = np.stack([np.zeros(n), starts["nan_start"], near, starts["inf_start"], np.zeros(n)])
    X = PC.replicas(PC.base_face(dev.art, R), len(x0))
    res = dev.run(R, order, X, x0=x0)
    print(f"status {res['status'].tolist()} nfev {res['nfev'].tolist()}")
    assert (res["status"] != 0).all()
    for i, name in ((1, "nan_start"), (3, "inf_start")):
        want = PC.host_case(dev.art, R, name)
        assert PC.same_outputs(PC.row(res, i), want), (name, PC.differing(PC.row(res, i), want))
        assert int(res["status"][i]) == 4 and int(res["nfev"][i]) == PC.NAN_NFEV(n)
    assert PC.same_outputs(PC.row(res, 0), dev.solo(R, order, 0)) and PC.same_outputs(PC.row(res, 4), dev.solo(R, order, 0))
    one = PC.row(dev.run(R, order, X[:1], x0=x0[2:3]), 0)
    assert PC.same_outputs(PC.row(res, 2), one) and int(one["status"]) == 1
    if order == "reference":
        want = PC.host_run(PC.numpy_objective(dev.art, R, X[0]), near)
        assert PC.same_outputs(one, want), PC.differing(one, want)


@pytest.mark.parametrize("R", [5, 3])
@pytest.mark.parametrize("order", ORDERS)
def test_inf_face_alone_in_the_last_slot(order, R, dev):
    """1000 n rounds with one live machine, at slot 15: tucker_few<1> (rank 5, fast order), one-evaluation passes (reference order)."""
    n = 3 + R
    X = PC.replicas(PC.nan_face(), PC.EV)
    X[15] = PC.bad_faces(dev.art, R)["one_inf"]
    res = dev.run(R, order, X, timed=f"R={R} {order}: an Inf face at slot 15, fifteen NaN faces")
    assert (res["status"] != 0).all()
    for i in range(15):
        _assert_dead(res, i, n)
    want = PC.host_case(dev.art, R, "one_inf")
    assert PC.same_outputs(PC.row(res, 15), want), (PC.differing(PC.row(res, 15), want), PC.row(res, 15))
    assert int(res["status"][15]) == 2 and int(res["nfev"][15]) == 1000 * n


# ---- 2. the live count held constant ---------------------------------------------------------------------------------------------

REPLICA_K = [("fast", 5, k) for k in (1, 2, 3, 4, 5, 16)] + [("reference", 5, k) for k in range(1, 17)] + \
            [("reference", 3, k) for k in (1, 5, 6, 7, 8, 12, 13, 16)] + [("fast", 3, k) for k in (1, 4, 16)]


@pytest.mark.parametrize("order,R,k", REPLICA_K)
def test_k_replicas_are_k_times_the_solo_run(order, R, k, dev, golden_dir):
    """Fast order, rank 5: k = 1 few<1>; 2, 3, 4 mfma4 with that many live; 5 round16 with dead slots; 16 round16 full.  Reference
    order: rank 5 passes of k (k <= 8) or two of about k / 2; rank 3 (seven per pass) 1, 5, 6, 7, 4 + 4, 6 + 6, 5 + 4 + 4, 6 + 5 + 5."""
    res = dev.run(R, order, PC.replicas(PC.base_face(dev.art, R), k))
    want = dev.solo(R, order, 0)                            # ordinary face 0 is the base face
    assert np.array_equal(PC.ordinary_faces(dev.art, R, 1)[0], PC.base_face(dev.art, R))
    for i in range(k):
        assert PC.same_outputs(PC.row(res, i), want), (i, PC.differing(PC.row(res, i), want))
    assert int(want["status"]) == 1
    if order == "reference" and R == 5:
        g = np.load(os.path.join(golden_dir, "fx5_td_end_to_end.npz"))
        assert (res["nfev"] == g["nfev"][0]).all() and all(PC.same_bits(np.degrees(x)[:3], g["deg"][0]) for x in res["x"])
    if order == "reference" and R == 3:
        g = np.load(os.path.join(golden_dir, "fx10_td_identity_rank.npz"))
        assert (res["nfev"] == g["r3_nfev"][0]).all()
        assert all(PC.same_bits(x, g["r3_res_x"][0]) for x in res["x"]) and all(PC.same_bits(f, g["r3_res_fun"][0]) for f in res["fun"])


# ---- 3. sparse live masks --------------------------------------------------------------------------------------------------------

MASKS = {
    "0": ((0,), 16), "7": ((7,), 16), "15": ((15,), 16), "3+9": ((3, 9), 16), "0+15": ((0, 15), 16), "1+8+14": ((1, 8, 14), 16),
    "2+5+11+13": ((2, 5, 11, 13), 16), "0+4+8+12+15": ((0, 4, 8, 12, 15), 16), "nine": ((0, 2, 3, 5, 7, 8, 11, 13, 15), 16),
    "N33": ((0, 15, 16, 21, 32), 33),                       # three workgroups, the last one holds a single (live) face
}


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("R", [5, 3])
@pytest.mark.parametrize("order", ORDERS)
def test_sparse_live_masks(order, R, mask, dev):
    live, N = MASKS[mask]
    X, which = PC.mixed_batch(dev.art, R, live, N)
    res = dev.run(R, order, X)
    print(f"live {live}: nfev {res['nfev'][list(live)].tolist()}")
    assert (res["status"] != 0).all()
    for i in range(N):
        if i not in live:
            _assert_dead(res, i, 3 + R)
    for slot, w in zip(sorted(live), which):
        want = dev.solo(R, order, w)
        assert PC.same_outputs(PC.row(res, slot), want), (slot, w, PC.differing(PC.row(res, slot), want))
        assert int(want["status"]) == 1
    # the premise of the test: the live faces finish at different rounds, so the live set passes through further patterns
    assert len(which) == 1 or len({int(dev.solo(R, order, w)["nfev"]) for w in which}) > 1


# ---- 4. the C entry point itself ---------------------------------------------------------------------------------------------------

MARK_F, MARK_I = -7.25, -77


def _call(dev, R, order, X, ldx, skip=(), use_r=True):
    """nlml_tucker_powell_r (or _ex at rank 5) on the default stream: x with row stride ldx and NaN in the pad columns, one spare row
    in every buffer, outputs pre-filled with a marker; the outputs named in `skip` are passed as NULL -> dict of the [N+1]-row buffers."""
    N, n, d = len(X), 3 + R, dev.device
    xb = torch.full((N + 1, ldx), float("nan"), dtype=torch.float32, device=d)
    xb[:N, :PC.F] = torch.from_numpy(X).to(d)
    out = {"x": torch.full((N + 1, n), MARK_F, dtype=torch.float64, device=d), "fun": torch.full((N + 1,), MARK_F, dtype=torch.float64, device=d)}
    out.update({k: torch.full((N + 1,), MARK_I, dtype=torch.int32, device=d) for k in ("nfev", "nit", "status")})
    ptr = lambda k: None if k in skip else out[k].data_ptr()
    a = (dev.wm(R).data_ptr(), xb.data_ptr(), ldx, dev.cp.data_ptr(), N, None, out["x"].data_ptr(), ptr("fun"), ptr("nfev"), ptr("nit"),
         ptr("status"))
    torch.cuda.synchronize(d)
    L = _lib.lib()
    rc = L.nlml_tucker_powell_r(*a, R, ORDER_ID[order], None) if use_r else L.nlml_tucker_powell_ex(*a, ORDER_ID[order], None)
    assert rc == 0, L.nlml_last_error()
    torch.cuda.synchronize(d)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("R", [5, 3])
@pytest.mark.parametrize("order", ORDERS)
def test_c_entry_point_row_stride_and_null_outputs(order, R, dev):
    N = 17
    X = np.concatenate([PC.ordinary_faces(dev.art, R, 15), PC.bad_faces(dev.art, R)["zero"][None], PC.ordinary_faces(dev.art, R, 16)[15:]])
    base = _call(dev, R, order, X, PC.F)
    assert (base["status"][:N] != 0).all() and (base["status"][:N] == 1).all()
    optional = ("fun", "nfev", "nit", "status")
    mark = lambda a: MARK_F if a.dtype == np.float64 else MARK_I
    runs = [(1408, (), True), (1408, optional, True)] + [(1408, (k,), True) for k in optional]
    if order == "reference":
        runs += [(1405, (), True), (1405, optional, True)]
    if R == 5:
        runs += [(1408, (), False), (1408, optional, False)]            # nlml_tucker_powell_ex
    for ldx, skip, use_r in runs:
        got = _call(dev, R, order, X, ldx, skip, use_r)
        for k in PC.OUTPUTS:
            if k not in skip:
                assert PC.same_bits(got[k][:N], base[k][:N]), (ldx, skip, use_r, k)
            assert (got[k][N if k not in skip else 0:] == mark(got[k])).all(), (ldx, skip, use_r, k)   # the spare row; a NULL output's buffer
    for k in PC.OUTPUTS:
        assert (base[k][N:] == mark(base[k])).all(), k


# ---- 5. far starts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [3, 5])
def test_far_start_replays_on_the_host(R, dev):
    """Reference order from x0 = (3e4, -2e4, 1e5, 0...): the f-vectors' arguments reach 2.9e5 (k ~ 1.9e5 in cr_cos.h's reduction), where
    the device must still hand the machine numpy's objective bits.  (Beyond 2^20 both sides take their library cos: not pinned.)"""
    x0 = PC.bad_starts(R)["far_start"][None]
    got = PC.row(dev.run(R, "reference", PC.base_face(dev.art, R)[None], x0=x0), 0)
    want = PC.host_case(dev.art, R, "far_start")
    print(f"R={R}: device nfev {got['nfev']} nit {got['nit']} status {got['status']}; host nfev {want['nfev']} nit {want['nit']}")
    assert PC.same_outputs(got, want), (PC.differing(got, want), got, want)
    assert int(got["status"]) == 1 and np.abs(got["x"][:3]).min() > 1.9e4


@pytest.mark.parametrize("R", [3, 5])
def test_far_start_in_fast_order(R, dev):
    """The same start on the matrix cores: fun is the fast-order objective at the returned x; at rank 5 nlml_tucker_powell_ex and
    nlml_tucker_powell_r agree.  (The host replay of the rank-5 run on the matrix-core objective, oracle_tucker_objective_fast, is
    tests/test_td_fast_order_gpu.py::test_fast_powell_at_rank_five_replays_from_a_far_start.)"""
    x0 = PC.bad_starts(R)["far_start"][None]
    X = PC.base_face(dev.art, R)[None]
    got = dev.run(R, "fast", X, x0=x0)
    assert int(got["status"][0]) == 1 and np.abs(got["x"][0, :3]).min() > 1.9e4
    f = ops.tucker_objective(dev.wm(R), torch.from_numpy(X).to(dev.device), torch.from_numpy(got["x"]).to(dev.device), dev.cp, order="fast")
    assert PC.same_bits(f.cpu().numpy(), got["fun"])
    if R == 5:
        d = dev.device
        Xd, X0 = torch.from_numpy(X).to(d), torch.from_numpy(x0).to(d)
        outs = []
        for use_r in (False, True):
            o = [torch.empty(1, 8, dtype=torch.float64, device=d), torch.empty(1, dtype=torch.float64, device=d)] + \
                [torch.empty(1, dtype=torch.int32, device=d) for _ in range(3)]
            a = (dev.wm(5).data_ptr(), Xd.data_ptr(), PC.F, dev.cp.data_ptr(), 1, X0.data_ptr()) + tuple(t.data_ptr() for t in o)
            stream = torch.cuda.current_stream(d).cuda_stream
            L = _lib.lib()
            rc = L.nlml_tucker_powell_r(*a, 5, _lib.TD_ORDER_FAST, stream) if use_r else L.nlml_tucker_powell_ex(*a, _lib.TD_ORDER_FAST, stream)
            assert rc == 0
            torch.cuda.synchronize(d)
            outs.append(dict(zip(PC.OUTPUTS, (t.cpu().numpy() for t in o))))
        assert PC.same_outputs(outs[0], outs[1]) and PC.same_outputs(outs[0], got)


# ---- 6. wide batch ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide_faces(tucker_art):
    return RF.noisy_faces(tucker_art, 5, 645)               # 40 workgroups + 5


@pytest.mark.parametrize("order", ORDERS)
def test_wide_batch_fun_is_the_objective_at_x(order, dev, wide_faces):
    """Every one of 645 faces converges, and its fun is the objective (same order, its own kernel) at its x bit for bit: x is the very
    point the last line search evaluated (tests/test_td_powell_edges_host.py shows it on the host).  The batch reversed: the same
    outputs reversed."""
    res = dev.run(5, order, wide_faces, timed=f"{order}: 645 faces")
    assert (res["status"] == 1).all(), np.flatnonzero(res["status"] != 1)
    f = ops.tucker_objective(dev.wm(5), torch.from_numpy(wide_faces).to(dev.device), torch.from_numpy(res["x"]).to(dev.device), dev.cp,
                             order=order).cpu().numpy()
    bad = np.flatnonzero(f.view(np.uint64) != res["fun"].view(np.uint64))
    print(f"{order}: nfev {res['nfev'].min()}..{res['nfev'].max()}, fun != objective(x) at {bad.tolist()}")
    assert bad.size == 0
    rev = dev.run(5, order, wide_faces[::-1])
    for k in PC.OUTPUTS:
        assert PC.same_bits(rev[k][::-1], res[k]), k
