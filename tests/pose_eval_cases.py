"""Test helper of tests/test_pose_eval_exact_host.py and tests/test_pose_eval_exact_gpu.py: an EXACT reference of K5 (nlml_pose_eval /
nlml_pose_eval_merge) and the small input families at which the kernel changes form or can go wrong.  No GPU, no torch.cuda.

exact(gt, pred_or_pose, valid, lo, hi, intervals, decimals) -> Exact: every 2048-face record, the merged record and the result vector
in the layouts of include/nlml_hpe.h, built without the kernel, nlml_hpe_amd/metrics.py or oracle/metrics.py:

  pred        rational arithmetic on the exact value of float64(pose_f32) * 57.29577951308232, rounded ONCE to f64 (ties to even), then
              rint(x 10^d) / 10^d with the product, the rint and the quotient each rounded once: np.round's bits, the sign of zero
              included.  An f64 pose is degrees already and is only rounded (d >= 0).
  e, counts, sums, means, M2 about the EXACT mean     fractions.Fraction, rounded to f64 at the very end
  vector errors                                       mpmath at 60 digits on the f64 pred and gt, with a per-face error bound (vbound)
  result                                              mae, std (ddof 1), interval mae from the exact pooled totals, not from a merge

A NaN among a sum's terms gives NaN; a +inf (and no NaN) gives sum = mean = +inf and M2 = NaN (inf - inf), which is what any order of
IEEE additions gives inside one record; across records a Chan merge of an infinite mean depends on the order, so exact() refuses an
infinite e in a call of more than one record.

Input families (each returns Case objects; B is at most 3 * 2048 + 1):
  dyadic(B)            gt, pred multiples of 2^-10 inside +-64 as f64 degrees, decimals -1: every e and every sum of e is an exact f64 in
                       any order, so counts, sums, interval fields and the per-record mean (one division) are compared on the bits
  near_constant(B)     e = 40 + k 2^-30, |k| <= 64 plus a per-record offset: a one-pass variance or a merge that loses d fails
  rounding()           f32 radians through every decimals, f64 degrees on exact ties of both parities and signs, -0.0, +-inf, NaN
  edges()              gt on and next to lo / hi / interval bounds, -0.0, NaN and +-inf gt, overlapping / empty / repeated intervals,
                       K in {0, 1, 18, 64} with the axes in mixed order
  masks(B)             valid as bool and as u8 with 0 / 1 / 2 / 255, a single kept face at the record seams, empty records, no kept face
  rotations()          generic poses, pred == gt, yaw off by 180, pitch +-90, angles beyond +-360
  merge_records(K, n, family)   synthetic records for the merge launch on its own, with their exact pooled record

The vector-error bound.  vbound(c, theta) bounds |v_device - v_exact| in degrees for one vector of one face, c the exact dot product:
  max |acos(clip(c +- delta)) - acos(c)| * 180/pi + 8 ulp(v),
delta a bound on the error of the device's f64 dot product, u = 2^-53:
  - an angle in radians is fl(x * kRad): one rounding and kRad's own representation error, together <= 2 u |theta|;
  - OCML documents sincos and acos in f64 within 2 ulp; a sine or cosine is at most 1, its ulp at most 2 u, so with the argument's error
    (|d sin| <= |d theta|) each of the six values of a pose is within  et = (4 + 2 |theta|) u  of the exact one;
  - columns(): an entry is a product of at most three such values (2 roundings) plus a product of two (1 rounding) and one addition:
    3 et + 2 u + 2 et + u + u = 5 et + 4 u =: ec  (all factors and partial results are at most 1 in magnitude);
  - the dot product: three products of two entries (2 ec + u each) and two additions (u each): 6 ec + 5 u.
  delta = 6 (5 et + 4 u) + 5 u = (149 + 60 |theta|) u, taken with theta the largest of the face's six angles, times 1.01 for the
  second-order terms.  A contraction into fma only removes roundings.  The 8 ulp(v) cover acos (2 ulp), the product with the rounded
  180/pi (2 ulp) and slack.  tests/test_pose_eval_exact_host.py checks that numpy's own f64 evaluation lies inside this bound.
At a few degrees of error the bound is ~1e-11 degrees; at pred == gt (c = 1) it is acos(1 - delta) ~ 1e-5 degrees: the bound says so.

Nothing here looks at the code under test."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction

import mpmath
import numpy as np

FACES = 2048                                   # NLML_POSE_EVAL_FACES_PER_RECORD
K_DEG = 57.29577951308232                      # np.degrees' factor
MP_DPS = 60
U = 2.0 ** -53
REL = 1e-12                                    # the project's relative bound for M2, merged mean, std, interval mae (test_pose_eval_gpu.py)
KEYS = ("mae_yaw", "mae_pitch", "mae_roll", "mae_total", "maev", "v_left", "v_down", "v_front", "std_yaw", "std_pitch", "std_roll")

# Where a merged M2 needs more than 1e-12 relative: near-constant records, whose merged mean carries a rounding of 2^-48 into a d of
# 2^-30 |k|.  The figure is the relative distance of the flat f64 Chan fold (chan_fold below) from the exact pooled M2, the largest over
# the cases named, as tests/test_pose_eval_exact_host.py measures it (it fails if a figure here is no longer the measured one); the GPU
# tests allow 4x, since the kernel folds in blocks, not flat.  Dyadic records stay at 1e-12 beyond 512 records too: the same test
# measures 1.6e-15 for them.
MEASURED_M2 = {"near-merge": 8.0e-8,           # merge_cases() of family "near": 7.92e-8, at K = 64, n = 177
               "near-eval": 4.6e-8}            # near_constant()'s own three records: 4.52e-8
MERGE_TOL_M2 = {f: 4.0 * v for f, v in MEASURED_M2.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# exact scalar pieces
def rne(q: Fraction) -> float:
    """The f64 nearest a rational, ties to even: Python's int / int is correctly rounded."""
    return q.numerator / q.denominator


def _signed_zero(neg: bool) -> float:
    return -0.0 if neg else 0.0


def mul_once(x: float, c: float) -> float:
    """fl(x * c) with one rounding, the sign of zero and the non-finite cases as IEEE has them (c finite and positive)."""
    if not math.isfinite(x):
        return x
    if x == 0.0:
        return x
    return rne(Fraction(x) * Fraction(c))


def round_decimals(x: float, d: int) -> float:
    """np.round(x, d) for d >= 0: fl(rint(fl(x * 10^d)) / 10^d); d < 0: x."""
    if d < 0 or not math.isfinite(x):
        return x
    s = Fraction(10) ** d
    y = mul_once(x, float(s))
    if not math.isfinite(y):
        return y
    neg = math.copysign(1.0, y) < 0
    r = round(Fraction(y))                     # an int, ties to even
    if r == 0:
        return _signed_zero(neg)
    return rne(Fraction(r) / s)


def exact_pred(pose: np.ndarray, decimals: int) -> np.ndarray:
    """f32 radians -> np.round(np.degrees(pose.astype(f64)), decimals); f64 degrees -> np.round(pose, decimals); no rounding for d < 0."""
    out = np.empty(pose.shape, np.float64)
    flat, o = pose.ravel(), out.reshape(-1)
    f32 = pose.dtype == np.float32
    for i, v in enumerate(flat):
        x = float(v)
        if f32:
            x = mul_once(x, K_DEG)
        o[i] = round_decimals(x, decimals)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# vector errors in mpmath
_vcache: dict = {}


def _columns(yaw, pitch, roll):
    """The l / b / f columns of Rx(pitch) Ry(-yaw) Rz(roll), degrees in; an entry is None where a non-finite angle reaches it."""
    def sc(x):
        if not math.isfinite(x):
            return None, None
        t = mpmath.mpf(x) * mpmath.pi / 180
        return mpmath.sin(t), mpmath.cos(t)

    def mul(*f):
        if any(v is None for v in f):
            return None
        out = mpmath.mpf(1)
        for v in f:
            out *= v
        return out

    def add(a, b):
        return None if a is None or b is None else a + b

    def neg(a):
        return None if a is None else -a
    sx, cx = sc(pitch)
    sy, cy = sc(-yaw)
    sz, cz = sc(roll)
    return [[mul(cy, cz), add(mul(sx, sy, cz), mul(cx, sz)), add(neg(mul(cx, sy, cz)), mul(sx, sz))],
            [neg(mul(cy, sz)), add(neg(mul(sx, sy, sz)), mul(cx, cz)), add(mul(cx, sy, sz), mul(sx, cz))],
            [sy, neg(mul(sx, cy)), mul(cx, cy)]]


def vbound(c, theta: float):
    """The per-vector bound of the module docstring, in degrees (an mpf); c the exact dot product, theta the largest angle in radians."""
    delta = mpmath.mpf(1.01 * (149.0 + 60.0 * theta) * U)
    deg = 180 / mpmath.pi
    clip = lambda v: max(mpmath.mpf(-1), min(mpmath.mpf(1), v))  # noqa: E731
    a0 = mpmath.acos(clip(c))
    spread = max(abs(mpmath.acos(clip(c + delta)) - a0), abs(mpmath.acos(clip(c - delta)) - a0))
    v = a0 * deg
    return spread * deg + 8 * 2 * U * v + mpmath.mpf(2) ** -1070


def face_vectors(g, p):
    """((v_left, v_down, v_front), (bound x 3)) of one face as mpf, None for a vector that a non-finite angle reaches.  Cached per face:
    the size cases are prefixes of one data set."""
    key = (g.tobytes(), p.tobytes())
    hit = _vcache.get(key)
    if hit is not None:
        return hit
    with mpmath.workdps(MP_DPS):
        cg, cp = _columns(*(float(v) for v in g)), _columns(*(float(v) for v in p))
        ang = [abs(float(v)) for v in (*g, *p) if math.isfinite(v)]
        theta = max(ang, default=0.0) * math.pi / 180.0
        vs, bs = [], []
        for a, b in zip(cg, cp):
            if any(v is None for v in (*a, *b)):
                vs.append(None)
                bs.append(None)
                continue
            c = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
            c = max(mpmath.mpf(-1), min(mpmath.mpf(1), c))
            vs.append(mpmath.acos(c) * 180 / mpmath.pi)
            bs.append(vbound(c, theta))
    _vcache[key] = (tuple(vs), tuple(bs))
    return _vcache[key]


def _mpf_to_float(v) -> float:
    sign, man, exp, _ = v._mpf_
    if man == 0:
        return 0.0
    man = int(man)
    r = float(man << exp) if exp >= 0 else man / (1 << -exp)
    return -r if sign else r


# ---------------------------------------------------------------------------------------------------------------------------------
class _Stat:
    """An exact (count, sum, sum of squares) of f64 terms with IEEE's non-finite outcomes."""

    def __init__(self):
        self.n, self.s, self.q, self.nan, self.inf = 0, Fraction(0), Fraction(0), False, False

    def add(self, e: float):
        self.n += 1
        if math.isnan(e):
            self.nan = True
        elif math.isinf(e):
            self.inf = True
        else:
            f = Fraction(e)
            self.s += f
            self.q += f * f

    def merge(self, o: "_Stat"):
        self.n += o.n
        self.s += o.s
        self.q += o.q
        self.nan |= o.nan
        self.inf |= o.inf

    def sum(self) -> float:
        return math.nan if self.nan else (math.inf if self.inf else rne(self.s))

    def mean_q(self) -> Fraction:
        return self.s / self.n

    def mean(self, empty=0.0) -> float:
        if self.n == 0:
            return empty
        return math.nan if self.nan else (math.inf if self.inf else rne(self.mean_q()))

    def m2_q(self) -> Fraction:
        return self.q - self.s * self.s / self.n

    def m2(self) -> float:
        if self.n == 0:
            return 0.0
        return math.nan if (self.nan or self.inf) else rne(self.m2_q())


class _VSum:
    def __init__(self):
        self.s, self.b, self.abs, self.nan, self.n = mpmath.mpf(0), mpmath.mpf(0), mpmath.mpf(0), False, 0

    def add(self, v, b):
        self.n += 1
        if v is None:
            self.nan = True
        else:
            self.s += v
            self.b += b
            self.abs += abs(v)

    def merge(self, o):
        self.s += o.s
        self.b += o.b
        self.abs += o.abs
        self.nan |= o.nan
        self.n += o.n

    def value(self) -> float:
        return math.nan if self.nan else _mpf_to_float(self.s)

    def bound(self, extra_terms=0) -> float:
        """The per-face bounds summed, plus the summation error of n + extra_terms f64 additions of non-negative terms."""
        return float(self.b + (self.n + extra_terms + 2) * U * self.abs)


@dataclass
class Exact:
    pred: np.ndarray            # f64[B,3]
    keep: np.ndarray            # bool[B]
    records: np.ndarray         # f64[nrec, 12+2K]
    record: np.ndarray          # f64[12+2K] the pooled record
    result: np.ndarray          # f64[14+2K]
    v_tol_records: np.ndarray   # f64[nrec,3] bound on |sum v| per record
    v_tol_record: np.ndarray    # f64[3] the same for the pooled sums
    v_tol_result: np.ndarray    # f64[4] for result[4..7]
    m2_floor_records: np.ndarray  # f64[nrec,3] n (ulp(mean)/2)^2: what the rounded mean adds to a two-pass M2
    m2_floor_record: np.ndarray   # f64[3]
    nonfinite: bool = False


def _record_row(kept, noface, oor, st, vs, ivs):
    row = [float(kept), float(noface), float(oor)]
    row += [s.mean() for s in st]
    row += [s.m2() for s in st]
    row += [v.value() for v in vs]
    for s in ivs:
        row += [float(s.n), s.sum() if s.n else 0.0]
    return row


def _floor(st):
    out = []
    for s in st:
        m = s.mean()
        out.append(2.0 * s.n * (np.spacing(abs(m)) / 2) ** 2 if s.n and math.isfinite(m) else 0.0)
    return out


def exact(gt, pred_or_pose, valid, lo, hi, intervals, decimals) -> Exact:
    gt = np.ascontiguousarray(gt, np.float64)
    pose = np.ascontiguousarray(pred_or_pose)
    assert pose.dtype in (np.float32, np.float64) and pose.shape == gt.shape
    B = len(gt)
    lo = [-math.inf] * 3 if lo is None else [float(v) for v in lo]
    hi = [math.inf] * 3 if hi is None else [float(v) for v in hi]
    intervals = [(int(a), float(l), float(h)) for a, l, h in intervals]
    K = len(intervals)
    pred = exact_pred(pose, int(decimals))
    face = np.ones(B, bool) if valid is None else (np.asarray(valid).astype(np.int64) != 0)
    keep = np.zeros(B, bool)
    nrec = -(-B // FACES)
    rows, vtol, floors = [], [], []
    P_st, P_vs, P_iv = [_Stat() for _ in range(3)], [_VSum() for _ in range(3)], [_Stat() for _ in range(K)]
    P_cnt = [0, 0, 0]
    any_inf = False
    with mpmath.workdps(MP_DPS):
        for r in range(nrec):
            st, vs, ivs = [_Stat() for _ in range(3)], [_VSum() for _ in range(3)], [_Stat() for _ in range(K)]
            kept = noface = oor = 0
            for f in range(r * FACES, min(B, (r + 1) * FACES)):
                g = gt[f]
                in_range = all(lo[a] <= g[a] <= hi[a] for a in range(3))          # a NaN compares false
                noface += not face[f]
                oor += not in_range
                if not (face[f] and in_range):
                    continue
                keep[f] = True
                kept += 1
                p = pred[f]
                e = []
                for a in range(3):
                    ga, pa = float(g[a]), float(p[a])
                    if math.isnan(ga) or math.isnan(pa) or (math.isinf(ga) and math.isinf(pa) and ga == pa):
                        ev = math.nan
                    elif math.isinf(ga) or math.isinf(pa):
                        ev = math.inf
                    else:
                        ev = rne(abs(Fraction(ga) - Fraction(pa)))
                    any_inf |= math.isinf(ev)
                    e.append(ev)
                    st[a].add(ev)
                v, b = face_vectors(g, p)
                for c in range(3):
                    vs[c].add(v[c], b[c])
                for k, (a, l, h) in enumerate(intervals):
                    if l <= g[a] < h:
                        ivs[k].add(e[a])
            rows.append(_record_row(kept, noface, oor, st, vs, ivs))
            vtol.append([v.bound() for v in vs])
            floors.append(_floor(st))
            for a in range(3):
                P_st[a].merge(st[a])
                P_vs[a].merge(vs[a])
            for k in range(K):
                P_iv[k].merge(ivs[k])
            P_cnt = [P_cnt[0] + kept, P_cnt[1] + noface, P_cnt[2] + oor]
    if any_inf and nrec > 1:
        raise NotImplementedError("an infinite e in a call of more than one record: the merged mean depends on the merge order")
    L = 12 + 2 * K
    records = np.array(rows, np.float64).reshape(nrec, L)
    record = np.array(_record_row(*P_cnt, P_st, P_vs, P_iv), np.float64)
    n = P_cnt[0]
    res = np.full(14 + 2 * K, math.nan)
    nf = any(s.nan or s.inf for s in P_st)
    if n > 0:
        for a in range(3):
            res[a] = P_st[a].mean()
        res[3] = math.nan if any(s.nan for s in P_st) else (math.inf if nf else rne(sum(s.mean_q() for s in P_st) / 3))
        if any(v.nan for v in P_vs):
            res[4] = math.nan
        else:
            res[4] = _mpf_to_float(sum(v.s for v in P_vs) / (3 * n))
        for c in range(3):
            res[5 + c] = math.nan if P_vs[c].nan else _mpf_to_float(P_vs[c].s / n)
        if n > 1:
            for a in range(3):
                res[8 + a] = math.nan if (P_st[a].nan or P_st[a].inf) else math.sqrt(rne(P_st[a].m2_q() / (n - 1)))
    res[11:14] = P_cnt
    for k in range(K):
        res[14 + 2 * k] = P_iv[k].n
        res[15 + 2 * k] = P_iv[k].mean(empty=math.nan)
    vt_rec = np.array([v.bound(extra_terms=nrec) for v in P_vs])
    vt_res = np.array([vt_rec.sum() / (3 * n) + 4 * U * abs(res[4]), *(vt_rec[c] / n + 4 * U * abs(res[5 + c]) for c in range(3))]) \
        if n > 0 and not any(v.nan for v in P_vs) else np.zeros(4)
    return Exact(pred, keep, records, record, res, np.array(vtol).reshape(nrec, 3), vt_rec, vt_res,
                 np.array(floors).reshape(nrec, 3), np.array(_floor(P_st)), nonfinite=nf)


# ---------------------------------------------------------------------------------------------------------------------------------
# the merge rule as a flat f64 left fold (what tests/test_pose_eval_host.py restates), and records for the merge launch on its own
def chan(a, b):
    """(n, mean, M2) merge, as the kernel's merge launch does it: an empty side leaves the other as it is."""
    na, ma, Ma = a
    nb, mb, Mb = b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    d = mb - ma
    return n, ma + d * (nb / n), Ma + Mb + d * d * (na * (nb / n))


def part(x):
    return (len(x), float(x.mean()) if len(x) else 0.0, float(((x - x.mean()) ** 2).sum()) if len(x) else 0.0)


def chan_fold(records: np.ndarray):
    """The flat left fold of records f64[n, L] -> (n, mean[3], M2[3]) in f64."""
    out = []
    for a in range(3):
        acc = (0.0, 0.0, 0.0)
        for r in records:
            acc = chan(acc, (float(r[0]), float(r[3 + a]), float(r[6 + a])))
        out.append(acc)
    return out[0][0], [o[1] for o in out], [o[2] for o in out]


def pooled_exact(records: np.ndarray):
    """The exact pooled (n, mean[3], M2[3]) of records taken at their f64 face value, as Fractions (mean 0 when empty)."""
    n = sum(int(r[0]) for r in records)
    means, m2s = [], []
    for a in range(3):
        if n == 0:
            means.append(Fraction(0))
            m2s.append(Fraction(0))
            continue
        m = sum(int(r[0]) * Fraction(float(r[3 + a])) for r in records) / n
        M = sum((Fraction(float(r[6 + a])) + int(r[0]) * (Fraction(float(r[3 + a])) - m) ** 2) for r in records if r[0] > 0)
        means.append(m)
        m2s.append(M)
    return n, means, m2s


def per_tile(K: int) -> int:
    return 12288 // (12 + 2 * K)


def merge_sizes(K: int):
    t = per_tile(K)
    return [0, 1, 2, 15, 16, 17, t - 1, t, t + 1, 2 * t + 3]


def merge_records(K: int, n: int, family: str, seed: int = 0) -> np.ndarray:
    """n synthetic records f64[n, 12+2K].  Counts are integers up to 2048; every plain-sum field is a multiple of 2^-10 below 2^17, so
    a sum over a few thousand records is exact in any order.  family "dyadic": means and M2 multiples of 2^-10; "near": means
    40 + k 2^-30 with M2 of the size 2048 values spread by 2^-30 |k| have.  About one record in four is empty (count 0, zeros), the
    first of three or more and the one at n // 2 always."""
    rng = np.random.default_rng(1000 * K + 7 * n + seed + (0 if family == "dyadic" else 500_000))
    L = 12 + 2 * K
    rec = np.zeros((n, L))
    cnt = rng.integers(1, FACES + 1, n).astype(np.float64)
    empty = rng.random(n) < 0.25
    if n >= 3:
        empty[0] = empty[n // 2] = True
    cnt[empty] = 0.0
    rec[:, 0] = cnt
    rec[:, 1:3] = rng.integers(0, FACES + 1, (n, 2))
    if family == "dyadic":
        rec[:, 3:6] = rng.integers(0, 128 * 1024, (n, 3)) / 1024.0
        rec[:, 6:9] = rng.integers(0, 1 << 27, (n, 3)) / 1024.0
    else:
        rec[:, 3:6] = 40.0 + rng.integers(-64, 65, (n, 3)) * 2.0 ** -30
        rec[:, 6:9] = cnt[:, None] * rng.integers(1, 4096, (n, 3)) * 2.0 ** -60
    rec[:, 9:12] = rng.integers(0, 1 << 27, (n, 3)) / 1024.0
    for k in range(K):
        rec[:, 12 + 2 * k] = rng.integers(0, FACES + 1, n)
        rec[:, 13 + 2 * k] = rng.integers(0, 1 << 27, n) / 1024.0
    rec[empty, 3:] = 0.0                       # an empty record is all zeros but its no-face / out-of-range counts
    return rec


def merge_cases():
    """[(K, n, family)]: both families at every size; the tolerance of a case is merge_tol_m2(family, n)."""
    return [(K, n, fam) for K in (0, 1, 18, 64) for n in merge_sizes(K) for fam in ("dyadic", "near")]


def merge_tol_m2(family: str, n: int) -> float:
    """The project's 1e-12 for dyadic records; 4x the measured flat-fold distance for near-constant ones."""
    return REL if family == "dyadic" else MERGE_TOL_M2["near-merge"]


# ---------------------------------------------------------------------------------------------------------------------------------
# input families
@dataclass
class Case:
    name: str
    gt: np.ndarray
    pose: np.ndarray                            # f32 radians or f64 degrees
    valid: np.ndarray | None = None
    lo: tuple | None = None
    hi: tuple | None = None
    intervals: list = field(default_factory=list)
    decimals: int = -1
    dyadic: bool = False                        # sums of e are exact in any order: bit-for-bit fields
    m2_family: str | None = None                # a key of MERGE_TOL_M2 for the merged M2

    def args(self):
        return self.gt, self.pose, self.valid, self.lo, self.hi, self.intervals, self.decimals


_exact_cache: dict = {}


def exact_of(case: Case) -> Exact:
    """exact(*case.args()), computed once per case name."""
    if case.name not in _exact_cache:
        _exact_cache[case.name] = exact(*case.args())
    return _exact_cache[case.name]


LO = (-50.0, -40.5, -30.25)
HI = (51.0, 41.0, 31.5)
B_MAX = 3 * FACES + 1
SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, B_MAX)


def intervals_k(K: int):
    """K dyadic intervals, the axes in mixed order (2, 0, 1, 1, 0, 2, ...), 16 wide, stepping by 7 so that neighbours overlap."""
    order = (2, 0, 1, 1, 0, 2)
    return [(order[k % 6], -60.0 + 7.0 * (k // 3) + 0.25 * (k % 3), -44.0 + 7.0 * (k // 3) + 0.25 * (k % 3)) for k in range(K)]


_dy: dict = {}


def _dyadic_data():
    if not _dy:
        rng = np.random.default_rng(2024)
        # yaw within +-64, pitch +-48, roll +-36: LO / HI then keep about half of the faces, not a quarter
        _dy["gt"] = np.stack([rng.integers(-w * 1024, w * 1024 + 1, B_MAX) for w in (64, 48, 36)], axis=1) / 1024.0
        _dy["pred"] = rng.integers(-64 * 1024, 64 * 1024 + 1, (B_MAX, 3)) / 1024.0
    return _dy["gt"], _dy["pred"]


def dyadic(B: int) -> Case:
    gt, pred = _dyadic_data()
    return Case(f"dyadic-{B}", gt[:B].copy(), pred[:B].copy(), None, LO, HI, intervals_k(18), -1, dyadic=True)


def masks(B: int):
    """The mask variants that exist at this B, on the dyadic data (unbounded range: the mask alone decides, but for `u8`)."""
    gt, pred = _dyadic_data()
    gt, pred = gt[:B].copy(), pred[:B].copy()
    rng = np.random.default_rng(77 + B)
    iv = intervals_k(18)
    out = []

    def case(tag, valid, lo=None, hi=None):
        out.append(Case(f"mask-{tag}-{B}", gt, pred, valid, lo, hi, iv, -1, dyadic=True))
    case("u8", rng.choice(np.array([0, 1, 2, 255], np.uint8), B), LO, HI)
    case("bool", rng.random(B) < 0.5)
    case("none-kept", np.zeros(B, bool))
    for idx in sorted({0, 2047, 2048, B - 1}):
        if idx < B:
            v = np.zeros(B, np.uint8)
            v[idx] = 2 if idx % 2 else 1          # the single kept face is also once a byte that is neither 0 nor 1
            case(f"only-{idx}", v)
    if B > 2 * FACES:
        v = rng.random(B) < 0.6
        v[:FACES] = False                          # an empty record at the start ...
        if B > 3 * FACES:
            v[2 * FACES:3 * FACES] = False         # ... and another in the middle
        else:
            v[FACES:2 * FACES] = False
            v[:FACES] = rng.random(FACES) < 0.6
        v[B - 1] = True
        case("empty-records", v)
    return out


def near_constant(B: int = 2 * FACES + 1) -> Case:
    """e = 40 + k 2^-30 exactly: gt a dyadic value, pred = gt -+ e (|pred| < 128, so 2^-30 k is far above its ulp); |k| <= 64 around a
    per-record offset of up to +-64, so both the within-record M2 and the merge's d d term carry weight."""
    rng = np.random.default_rng(31)
    gt = rng.integers(-20 * 1024, 20 * 1024 + 1, (B, 3)) / 1024.0
    off = rng.integers(-64, 65, (-(-B // FACES), 3))
    k = rng.integers(-64, 65, (B, 3)) + np.repeat(off, FACES, axis=0)[:B]
    e = 40.0 + k * 2.0 ** -30
    sign = rng.choice([-1.0, 1.0], (B, 3))
    pred = gt - sign * e
    assert np.array_equal(np.abs(gt - pred), e)
    return Case(f"near-{B}", gt, pred, rng.random(B) < 0.9, None, None, intervals_k(1), -1, m2_family="near-eval")


DECIMALS = (-1, 0, 1, 3, 6, 15)


def rounding():
    """f32 radians through every decimals; f64 degrees at decimals 0 on exact half-integers of both parities and signs and at 1 and 3 on
    decimal ties; values that round to -0.0; +-inf and NaN (on rows without a face, and one NaN on a kept row)."""
    rng = np.random.default_rng(5)
    n = 300
    pose = rng.uniform(-1.6, 1.6, (n, 3)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-10, -1e-10, 8.7e-3, -8.7e-3, 8.726646e-3, -8.726646e-3, 2.6179939e-2, -2.6179939e-2,
                        1e-30, -1e-30, 1.5707964, -1.5707964, 7.0, -7.0], np.float32)
    pose[:len(special), 0] = special
    pose[:len(special), 2] = special[::-1]
    gt = np.degrees(pose.astype(np.float64)) + rng.normal(0.0, 2.0, (n, 3))
    gt[:len(special)] = rng.normal(0.0, 2.0, (len(special), 3))
    valid = np.ones(n, np.uint8)
    pose[100, 0], pose[101, 1], pose[102, 2] = np.inf, -np.inf, np.nan
    valid[100:103] = 0
    pose[103, 1] = np.nan                          # a NaN on a kept face: the pitch statistics and the vectors become NaN
    out = [Case(f"round-f32-d{d}", gt, pose, valid, None, None, intervals_k(3), d) for d in DECIMALS]
    half = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5, 0.49999999999999994, -0.49999999999999994, 0.0, -0.0, -0.2, 0.2,
                     1e-300, -1e-300, 4503599627370495.5, -4503599627370495.5, 4503599627370496.5, 1e17, -1e17, 22.5, -23.5, 24.5])
    m = len(half)
    deg = np.stack([half, half[::-1], np.roll(half, 5)], axis=1)
    gd = np.zeros((m + 3, 3))
    deg = np.concatenate([deg, [[np.inf, 0.0, 0.0], [0.0, -np.inf, 0.0], [0.0, 0.0, np.nan]]])
    vd = np.ones(m + 3, np.uint8)
    vd[m:] = 0
    for d in (0, -1):
        out.append(Case(f"round-f64-half-d{d}", gd, deg, vd, None, None, intervals_k(1), d))
    ties = np.array([0.05, -0.05, 0.15, 0.25, -0.25, 0.35, 2.675, -2.675, 1.0005, -1.0005, 0.0005, -0.0005, 0.0004, -0.0004, 1.0015,
                     0.125, -0.125, 0.375, 12.3456789, -12.3456789, 0.3, -0.7, 33.3335, -33.3345])
    td = np.stack([ties, -ties, ties[::-1]], axis=1)
    for d in (1, 3, 6, 15):
        out.append(Case(f"round-f64-ties-d{d}", np.zeros_like(td), td, None, None, None, [], d))
    return out


def edges():
    """gt on and next to the range bounds and the interval bounds; -0.0 against an interval low of 0.0; NaN gt (out of range); +-inf gt
    under the unbounded range (kept: e = inf); overlapping, empty and repeated intervals; K in {0, 1, 18, 64}."""
    rng = np.random.default_rng(9)
    up = lambda v: np.nextafter(v, np.inf)         # noqa: E731
    dn = lambda v: np.nextafter(v, -np.inf)        # noqa: E731
    lo, hi = (-50.0, -40.0, -30.3), (51.0, 41.7, 31.0)
    iv = [(0, -33.33, 0.0), (0, 0.0, 33.33), (1, -10.1, 10.1), (2, 0.0, 15.5),        # shipped-like, with a low of 0.0
          (0, -10.0, 20.0), (0, 5.0, 40.0),                                             # overlapping
          (1, 3.0, 3.0), (1, 7.0, -7.0),                                                # empty: low >= high
          (0, -5.5, 5.5), (1, -5.5, 5.5), (2, -5.5, 5.5)]                               # the same interval on all three axes
    vals = []
    for a in range(3):
        for v in (lo[a], hi[a]):
            vals += [(a, v), (a, up(v)), (a, dn(v))]
    for a, l, h in iv:
        vals += [(a, l), (a, h), (a, dn(h)), (a, dn(l)), (a, up(l))]
    vals += [(0, -0.0), (2, -0.0), (0, np.nan), (1, np.nan), (2, np.nan)]
    n = len(vals)
    gt = rng.integers(-4 * 1024, 4 * 1024 + 1, (n, 3)) / 1024.0      # inside every range, so the placed value alone decides
    for i, (a, v) in enumerate(vals):
        gt[i, a] = v
    pred = gt + rng.integers(-8 * 1024, 8 * 1024 + 1, (n, 3)) / 1024.0
    pred[np.isnan(pred)] = 1.0
    out = [Case("edges-bounds", gt, pred, None, lo, hi, iv, -1)]
    pose32 = np.radians(pred).astype(np.float32)
    out.append(Case("edges-bounds-f32", gt, pose32, None, lo, hi, iv, 3))
    # K in {0, 1, 18, 64} on gt that sits on the dyadic interval bounds of intervals_k
    for K in (0, 1, 18, 64):
        ivk = intervals_k(K)
        g = rng.integers(-64 * 1024, 64 * 1024 + 1, (400, 3)) / 1024.0
        for i, (a, l, h) in enumerate(ivk):
            g[3 * i % 400, a], g[(3 * i + 1) % 400, a], g[(3 * i + 2) % 400, a] = l, h, dn(h)
        p = g + rng.integers(-8 * 1024, 8 * 1024 + 1, (400, 3)) / 1024.0
        out.append(Case(f"edges-K{K}", g, p, None, LO, HI, ivk, -1, dyadic=False))
    # +-inf gt under the default unbounded range: in range, kept, e = inf on that axis (one record: see exact())
    g = rng.integers(-4 * 1024, 4 * 1024 + 1, (40, 3)) / 1024.0
    g[3, 0], g[17, 1] = np.inf, -np.inf
    p = g.copy()
    p[~np.isfinite(p)] = 2.0
    p[:, 2] += 1.5
    out.append(Case("edges-inf-gt", g, p, None, None, None, [(0, 0.0, np.inf), (1, -np.inf, 0.0), (2, -1.0, 1.0)], -1))
    return out


def rotations():
    """For the vector errors: generic poses, pred == gt bit for bit, yaw off by 180, pitch +-90, angles beyond +-360."""
    rng = np.random.default_rng(13)
    n = 48
    g = rng.uniform(-80.0, 80.0, (n, 3))
    out = [Case("rot-generic", g, g + rng.normal(0.0, 4.0, (n, 3))), Case("rot-identical", g, g.copy())]
    p = g.copy()
    p[:, 0] += 180.0
    out.append(Case("rot-yaw180", g, p))
    g90 = g.copy()
    g90[:, 1] = np.where(np.arange(n) % 2, 90.0, -90.0)
    out.append(Case("rot-pitch90", g90, g90 + rng.normal(0.0, 3.0, (n, 3))))
    out.append(Case("rot-pitch90-identical", g90, g90.copy()))
    big = g + 360.0 * rng.integers(-3, 4, (n, 3))
    out.append(Case("rot-beyond360", big, g + rng.normal(0.0, 2.0, (n, 3)) - 360.0 * rng.integers(-3, 4, (n, 3))))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
def numpy_vectors(gt, pred):
    """numpy's own f64 evaluation of the kernel's formula, per face: f64[n,3] degrees (left, down, front)."""
    def cols(yaw, pitch, roll):
        rx, ry, rz = pitch * 0.017453292519943295, -(yaw * 0.017453292519943295), roll * 0.017453292519943295
        sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
        return [(cy * cz, sx * sy * cz + cx * sz, -cx * sy * cz + sx * sz), (-cy * sz, -sx * sy * sz + cx * cz, cx * sy * sz + sx * cz),
                (sy, -sx * cy, cx * cy)]
    cg, cp = cols(*gt.T), cols(*pred.T)
    out = []
    for a, b in zip(cg, cp):
        out.append(np.arccos(np.clip(a[0] * b[0] + a[1] * b[1] + a[2] * b[2], -1.0, 1.0)) * (180.0 / np.pi))
    return np.stack(out, axis=1)
