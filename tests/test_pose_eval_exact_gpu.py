"""GPU: K5 (nlml_pose_eval / nlml_pose_eval_merge) against the exact reference of tests/pose_eval_cases.py, record by record: the
2048-face records read back out of a workspace of the test's own, the merged record and the result, at the face counts where a record
fills, the merge launch on its own across its LDS tile (1024 / 877 / 256 / 87 records for K = 0 / 1 / 18 / 64), every rounding and
range / interval edge through both input forms, and the vector errors inside a derived per-face bound.

Bit for bit: the counts, pred_out, keep_out, and on dyadic inputs every sum, interval field and per-record mean.  Per-record M2, merged
mean, std, interval mae of other inputs: the project's 1e-12 relative (a two-pass M2 over at most 2048 values is inside (n + 4) 2^-53),
plus n (ulp(mean) / 2)^2 for the rounded mean a two-pass M2 is taken about.  The merged M2 of near-constant records: 4x the distance of
the flat f64 Chan fold from the exact value, measured in tests/test_pose_eval_exact_host.py."""
import math

import numpy as np
import pytest
import torch

import pose_eval_cases as PC
from nlml_hpe_amd import ops
from test_gpu_parity import _report

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


def _dv(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want):
    """Bit for bit, a NaN for a NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and np.array_equal(_bits(got[~nan]), _bits(want[~nan])))


def _close(got, want, tol):
    """|got - want| <= tol where want is finite; the same infinity, or a NaN, where it is not."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), want.shape)
    fin = np.isfinite(want)
    ok = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)) <= tol, False)
    ok = np.where(np.isnan(want), np.isnan(got), ok)
    ok = np.where(np.isinf(want), got == want, ok)
    return bool(ok.all())


def _run(case, device, pose=None):
    """One ops.pose_eval call with a workspace of the test's own -> records f64[nrec, L], record, result, pred, keep (numpy)."""
    K = len(case.intervals)
    L = 12 + 2 * K
    nrec = -(-len(case.gt) // PC.FACES)
    ws = torch.full((nrec * L + 16,), SENTINEL, dtype=torch.float64, device=device)
    rec, res, pred, keep = ops.pose_eval(_dv(case.pose if pose is None else pose, device), _dv(case.gt, device), _dv(case.valid, device),
                                         case.lo, case.hi, case.intervals, case.decimals, return_per_face=True, workspace=ws)
    w = ws.cpu().numpy()
    assert (w[nrec * L:] == SENTINEL).all(), "the record launch wrote past its records"
    return dict(ws=ws, records=w[:nrec * L].reshape(nrec, L), record=rec.cpu().numpy(), result=res.cpu().numpy(), pred=pred.cpu().numpy(),
                keep=keep.cpu().numpy(), rec_t=rec, res_t=res)


def _check_record(got, want, K, dyadic, m2_tol, m2_floor, v_tol, what, mean_exact):
    iv_cnt, iv_sum = slice(12, 12 + 2 * K, 2), slice(13, 12 + 2 * K, 2)
    assert _same(got[:3], want[:3]), (what, "counts", got[:3], want[:3])
    assert _same(got[iv_cnt], want[iv_cnt]), (what, "interval counts")
    if dyadic:
        assert _same(got[iv_sum], want[iv_sum]), (what, "interval sums")
    else:
        assert _close(got[iv_sum], want[iv_sum], PC.REL * np.abs(want[iv_sum])), (what, "interval sums", got[iv_sum], want[iv_sum])
    if mean_exact:
        assert _same(got[3:6], want[3:6]), (what, "mean", got[3:6], want[3:6])
    else:
        assert _close(got[3:6], want[3:6], PC.REL * np.abs(want[3:6])), (what, "mean", got[3:6], want[3:6])
    assert _close(got[6:9], want[6:9], m2_tol * np.abs(want[6:9]) + m2_floor), (what, "M2", got[6:9], want[6:9])
    assert _close(got[9:12], want[9:12], v_tol), (what, "sum v", got[9:12], want[9:12], v_tol)


def _check(case, ex, out):
    K = len(case.intervals)
    m2_tol = PC.MERGE_TOL_M2[case.m2_family] if case.m2_family else PC.REL
    # per face
    assert _same(out["pred"], ex.pred), (case.name, "pred_out")
    assert np.array_equal(out["keep"], ex.keep), (case.name, "keep_out")
    # every record, then the merged one
    assert out["records"].shape == ex.records.shape
    for r in range(len(ex.records)):
        _check_record(out["records"][r], ex.records[r], K, case.dyadic, PC.REL, ex.m2_floor_records[r], ex.v_tol_records[r],
                      (case.name, "record", r), mean_exact=case.dyadic)
    _check_record(out["record"], ex.record, K, case.dyadic, m2_tol, ex.m2_floor_record, ex.v_tol_record, (case.name, "merged"),
                  mean_exact=case.dyadic and len(ex.records) == 1)
    # the result
    got, want = out["result"], ex.result
    n = want[11]
    assert _same(got[11:14], want[11:14]) and _same(got[14::2], want[14::2]), (case.name, "result counts")
    assert _close(got[:4], want[:4], PC.REL * np.abs(want[:4])), (case.name, "mae", got[:4], want[:4])
    assert _close(got[4:8], want[4:8], ex.v_tol_result), (case.name, "vector errors", got[4:8], want[4:8], ex.v_tol_result)
    if n > 1:
        M2 = ex.record[6:9]
        with np.errstate(invalid="ignore"):
            dstd = np.sqrt((M2 + m2_tol * M2 + ex.m2_floor_record) / (n - 1)) - want[8:11] + 8 * PC.U * want[8:11]
        assert _close(got[8:11], want[8:11], np.nan_to_num(dstd)), (case.name, "std", got[8:11], want[8:11])
    else:
        assert np.isnan(got[8:11]).all(), (case.name, "std of fewer than two faces")
    if case.dyadic:
        assert _same(got[15::2], want[15::2]), (case.name, "interval mae")
    else:
        assert _close(got[15::2], want[15::2], PC.REL * np.abs(want[15::2])), (case.name, "interval mae")


def _self_consistent(case, out):
    """pose_eval_merge of the call's own workspace records returns the call's merged record and result, bit for bit."""
    K = len(case.intervals)
    nrec = len(out["records"])
    recs = out["ws"][:nrec * (12 + 2 * K)].view(nrec, 12 + 2 * K)
    rec2, res2 = ops.pose_eval_merge(recs, K)
    assert torch.equal(rec2.view(torch.int64), out["rec_t"].view(torch.int64)), (case.name, "merge of the workspace: record")
    assert torch.equal(res2.view(torch.int64), out["res_t"].view(torch.int64)), (case.name, "merge of the workspace: result")


@pytest.mark.parametrize("B", PC.SIZES)
def test_dyadic_records_bit_for_bit(B, device):
    case = PC.dyadic(B)
    out = _run(case, device)
    _check(case, PC.exact_of(case), out)
    _self_consistent(case, out)


@pytest.mark.parametrize("B", PC.SIZES)
def test_masks_records_bit_for_bit(B, device):
    for case in PC.masks(B):
        out = _run(case, device)
        _check(case, PC.exact_of(case), out)
        _self_consistent(case, out)
    # a bool mask is its bytes: the same mask as 0 / 255 gives the same bits
    case = PC.masks(B)[1]
    as_u8 = PC.Case(case.name + "-as-u8", case.gt, case.pose, case.valid.astype(np.uint8) * 255, None, None, case.intervals, -1, dyadic=True)
    a, b = _run(case, device), _run(as_u8, device)
    assert np.array_equal(_bits(a["records"]), _bits(b["records"])) and np.array_equal(_bits(a["result"]), _bits(b["result"]))


def test_near_constant_errors_need_a_two_pass_variance(device):
    """e = 40 + k 2^-30: per-record M2 inside 1e-12 relative; the merged M2 inside 4x the flat f64 Chan fold's distance from the exact
    value, measured on the CPU as 4.52e-8 relative (quoted 4.6e-8, so 1.84e-7 is allowed; test_pose_eval_exact_host.py).  The device's own
    distance on an MI355X: 4.52e-8 merged (three records fold the same way flat or in blocks), 1.0e-14 per record."""
    case = PC.near_constant()
    ex = PC.exact_of(case)
    out = _run(case, device)
    d = np.abs(out["record"][6:9] - ex.record[6:9]) / ex.record[6:9]
    dr = np.abs(out["records"][:2, 6:9] - ex.records[:2, 6:9]) / ex.records[:2, 6:9]
    print(f"near-constant: merged M2 off by {d.max():.3e} relative (allowed {PC.MERGE_TOL_M2['near-eval']:.3e}), per record {dr.max():.3e}")
    _report("pose_eval_near_constant", merged_m2_distance=d.max(), allowed=PC.MERGE_TOL_M2["near-eval"], record_m2_distance=dr.max(),
            measured_flat_fold=PC.MEASURED_M2["near-eval"])
    _check(case, ex, out)
    _self_consistent(case, out)


@pytest.mark.parametrize("K", [0, 1, 18, 64])
def test_merge_launch_on_its_own(K, device):
    """Synthetic records across the merge's LDS tile, empty records interleaved.  Counts, plain sums and interval fields bit for bit (the
    records are dyadic); the pooled mean inside 1e-12; the pooled M2 inside 1e-12 for dyadic records, and for near-constant ones inside
    4x the flat f64 Chan fold's distance from the exact value, measured on the CPU as 7.92e-8 relative at K = 64, n = 177 (quoted
    8.0e-8, so 3.2e-7 is allowed; test_pose_eval_exact_host.py).  The device's own worst distances on an MI355X: 5.2e-8 near-constant,
    4.4e-16 dyadic."""
    worst = {"dyadic": 0.0, "near": 0.0}
    for n in PC.merge_sizes(K):
        for fam in ("dyadic", "near"):
            rec = PC.merge_records(K, n, fam)
            got_rec, got_res = (t.cpu().numpy() for t in ops.pose_eval_merge(_dv(rec, device).reshape(n, 12 + 2 * K), K))
            what = (K, n, fam)
            cnt, mean, M2 = PC.pooled_exact(rec)
            plain = [0, 1, 2, 9, 10, 11] + list(range(12, 12 + 2 * K))
            want_plain = rec[:, plain].sum(0) if n else np.zeros(len(plain))
            assert _same(got_rec[plain], want_plain), (what, "plain sums")
            assert cnt == got_rec[0]
            tol = PC.merge_tol_m2(fam, n)
            for a in range(3):
                m, M = PC.rne(mean[a]), PC.rne(M2[a])
                assert abs(got_rec[3 + a] - m) <= PC.REL * m, (what, "mean", a, got_rec[3 + a], m)
                assert abs(got_rec[6 + a] - M) <= tol * M, (what, "M2", a, got_rec[6 + a], M, tol)
                if M:
                    worst[fam] = max(worst[fam], abs(got_rec[6 + a] - M) / M)
            # the result: one division of exact sums where the sums are plain; mean and std from the merged record
            with np.errstate(invalid="ignore", divide="ignore"):
                sv = want_plain[3:6]
                want_v = np.array([(sv[0] + sv[1] + sv[2]) / (3.0 * cnt), *(sv / float(cnt))]) if cnt else np.full(4, np.nan)
                ic, isum = want_plain[6::2], want_plain[7::2]
                want_iv = np.where(ic > 0, isum / np.where(ic > 0, ic, 1.0), np.nan)
            assert _same(got_res[4:8], want_v), (what, "vector means")
            assert _same(got_res[11:14], want_plain[:3]) and _same(got_res[14::2], ic) and _same(got_res[15::2], want_iv), (what, "result")
            if cnt:
                assert _same(got_res[:3], got_rec[3:6]), (what, "mae is the merged mean")
                mt = PC.rne(sum(mean) / 3)
                assert abs(got_res[3] - mt) <= PC.REL * mt
            else:
                assert np.isnan(got_res[:11]).all() and (got_rec[3:9] == 0).all(), (what, "no kept face")
            for a in range(3):
                if cnt > 1:
                    want = math.sqrt(PC.rne(M2[a] / (cnt - 1)))
                    assert abs(got_res[8 + a] - want) <= (tol / 2 + 8 * PC.U) * want, (what, "std", a, got_res[8 + a], want)
                else:
                    assert np.isnan(got_res[8 + a]), (what, "std of fewer than two faces")
    # one kept face in all: the std is NaN (ddof 1) whatever the record's M2 field holds, the means are the record's
    one = np.zeros((3, 12 + 2 * K))
    one[1, 0], one[1, 3:6], one[1, 6:9] = 1.0, (1.5, 2.25, 40.0), (0.5, 2.0, 1e-20)
    got_rec, got_res = (t.cpu().numpy() for t in ops.pose_eval_merge(_dv(one, device), K))
    assert _same(got_rec, one[1]) and _same(got_res[:3], one[1, 3:6]) and got_res[11] == 1
    assert np.isnan(got_res[8:11]).all(), ("std of one face", got_res[8:11])
    print(f"merge launch K={K}: worst M2 distance dyadic {worst['dyadic']:.3e} (allowed {PC.REL:.1e}), near-constant {worst['near']:.3e} "
          f"(allowed {PC.MERGE_TOL_M2['near-merge']:.3e})")
    _report(f"pose_eval_merge_K{K}", dyadic_m2_distance=worst["dyadic"], near_m2_distance=worst["near"],
            near_allowed=PC.MERGE_TOL_M2["near-merge"], measured_flat_fold=PC.MEASURED_M2["near-merge"])


@pytest.mark.parametrize("case", PC.rounding() + PC.edges(), ids=lambda c: c.name)
def test_rounding_and_edges(case, device):
    ex = PC.exact_of(case)
    out = _run(case, device)
    _check(case, ex, out)
    _self_consistent(case, out)
    if case.pose.dtype == np.float32:
        # the other input form: the same degrees as f64 (np.degrees of the f32 radians, which the host test pins to the reference's bits)
        with np.errstate(invalid="ignore"):
            deg = np.degrees(case.pose.astype(np.float64))
        other = _run(case, device, pose=deg)
        _check(case, ex, other)
        for k in ("records", "record", "result", "pred"):
            assert _same(other[k], out[k]), (case.name, "f64 degrees against f32 radians", k)
        assert np.array_equal(other["keep"], out["keep"])


def test_empty_records_leave_an_infinite_mean_as_it_is(device):
    """An infinite GT angle inside the unbounded range gives an infinite e, mean and mae, as numpy's mean does.  Merged with the records
    of shards without a kept face, before and after, it stays so: an empty side must not enter the arithmetic (inf * 0 is a NaN)."""
    case = {c.name: c for c in PC.edges()}["edges-inf-gt"]
    ex = PC.exact_of(case)
    out = _run(case, device)
    assert out["record"][3] == np.inf and out["record"][4] == np.inf and np.isfinite(out["record"][5])
    empty = PC.Case("edges-inf-gt-no-face", case.gt, case.pose, np.zeros(len(case.gt), np.uint8), None, None, case.intervals, -1)
    rec0 = _run(empty, device)["rec_t"]
    assert rec0[0] == 0 and rec0[1] == len(case.gt)
    rec, res = (t.cpu().numpy() for t in ops.pose_eval_merge(torch.stack([rec0, out["rec_t"], rec0, rec0]), len(case.intervals)))
    want_rec, want_res = out["record"].copy(), out["result"].copy()
    want_rec[1] = want_res[12] = 3 * len(case.gt)
    assert _same(rec, want_rec), (rec, want_rec)
    assert _same(res, want_res), (res, want_res)
    assert _same(want_res[:3], ex.result[:3])


@pytest.mark.parametrize("name", ["edges-bounds", "edges-bounds-f32", "edges-K64", "edges-K0", "round-f64-half-d0", "round-f32-d15"])
def test_torch_op_returns_the_same_bits(name, device):
    case = {c.name: c for c in PC.rounding() + PC.edges()}[name]
    out = _run(case, device)
    inf = float("inf")
    rec, res = torch.ops.nlml_hpe.pose_eval(_dv(case.pose, device), _dv(case.valid, device), _dv(case.gt, device),
                                            [-inf] * 3 if case.lo is None else list(case.lo), [inf] * 3 if case.hi is None else list(case.hi),
                                            case.decimals, [float(v) for _, lo, hi in case.intervals for v in (lo, hi)],
                                            [a for a, _, _ in case.intervals])
    assert torch.equal(rec.view(torch.int64), out["rec_t"].view(torch.int64))
    assert torch.equal(res.view(torch.int64), out["res_t"].view(torch.int64))
    K = len(case.intervals)
    m1 = ops.pose_eval_merge(torch.stack([rec, rec]), K)
    m2 = torch.ops.nlml_hpe.pose_eval_merge(torch.stack([rec, rec]), K)
    assert torch.equal(m1[0].view(torch.int64), m2[0].view(torch.int64)) and torch.equal(m1[1].view(torch.int64), m2[1].view(torch.int64))


@pytest.mark.parametrize("case", PC.rotations(), ids=lambda c: c.name)
def test_vector_errors_inside_the_derived_bound(case, device):
    """The sums of the three vector errors against mpmath's, inside the per-face bound of pose_eval_cases.vbound summed over the kept
    faces plus the summation error: ~1e-11 degrees per face on generic poses, ~1e-5 at pred == gt, where acos is steep."""
    ex = PC.exact_of(case)
    out = _run(case, device)
    d = np.abs(out["record"][9:12] - ex.record[9:12])
    print(f"{case.name}: sum v off by {d.max():.3e} degrees over {int(ex.record[0])} faces, bound {ex.v_tol_record.max():.3e}")
    _report(f"pose_eval_vectors_{case.name}", distance=d.max(), bound=ex.v_tol_record.max())
    _check(case, ex, out)
    # a face at a time: the sum of a one-face call is that face's error
    for f in (0, len(case.gt) - 1):
        one = PC.Case(f"{case.name}-face{f}", case.gt[f:f + 1], case.pose[f:f + 1])
        _check(one, PC.exact_of(one), _run(one, device))
