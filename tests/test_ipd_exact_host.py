"""The IPD normalisation's three host statements against each other on inputs built to be hard (tests/ipd_cases.py) -- no GPU.

AGREEMENT: the rational reference, the C oracle and oracle.feature_norm (numpy) give the same bits -- the ipd of every face, every
engineered element, the sampled ordinary elements, the faces the rational reference answers whole, and FX1.
CERTIFICATION: what the families claim about themselves (coverage of the 1,395 columns, distance from an f32 midpoint, the visible fma
chain, double-rounding cases).
POWER: the wrong variants a kernel could compute instead, emulated on the engineered elements; the share of them each variant changes
(the bits differ from the rational reference's).  Measured, in % of the 1,395 engineered elements of a family (D: of its 1,395):

    variant                          A      B      C      D      P     PF
    n * (1/ipd), no corrections    4.1    7.3   11.5    8.2    8.5    8.2
    ipd one f64 ulp up            37.3   32.3   40.7   33.0   31.3   33.0
    ipd one f64 ulp down          42.3   31.0   38.9   32.8   31.5   33.6
    separately rounded squares     0.0   20.6    0.0    0.0    0.1    0.0
    an f32 division               49.0   49.6   52.0   59.8   48.7   49.7
    one direct rounding to f32     0.0   18.6   16.7   16.1   18.3   16.6

Each share is asserted to be at least half of that.  The separately rounded squares show only where a coordinate difference of the
eyes has more than 26 bits (its square is then inexact): family B is built that way, ordinary U(0,1) eyes never are.  Family A's ipd and
its ties are exact, so it has no double-rounding case; B and C must have some.  An engineered element is engineered against the RIGHT
arithmetic, so a variant that errs by less than the element's distance from its midpoint passes it: the shares are what one element
sees, and a copy of the prologue meets 3 (a column of one family) to 8,370 (all of them) such elements.
READ-OUT CERTIFICATE: ipd_cases.readout_net through the C oracle's f32 chain (order 2, the f32 kernel's) returns the engineered x itself
(shift 60) and moves with a one-ulp nudge of x on at least half of the probe family's engineered elements (shift 60: all; shift 0, the
live Tanh: measured below).
THE SHIPPED STATEMENT: nlml_hpe_amd/csrc/ipd_norm.h -- the header every kernel compiles: reciprocal, two fma corrections, negated
residual -- built for the host (tests/native/ipd_norm_host.cpp) gives the reference's bits and ipds on every family, the comparison the
GPU test makes of K1; with the residual the way it stood before the sign fix it does not, on family E."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ipd_cases as IC
from oracle import c_oracle as CO
from oracle import encoder_heads as EH
from oracle import feature_norm as FN

FAMILIES = IC.DENSE + IC.PROBES
ENGINEERED = tuple(n for n in FAMILIES if n != "E")
VARIANTS = ("nofma", "ipd_up", "ipd_dn", "sepsq", "f32div", "direct")
# measured shares (module docstring), as fractions
MEASURED = {
    "nofma": dict(A=.041, B=.073, C=.115, D=.082, P=.085, PF=.082),
    "ipd_up": dict(A=.373, B=.323, C=.407, D=.330, P=.313, PF=.330),
    "ipd_dn": dict(A=.423, B=.310, C=.389, D=.328, P=.315, PF=.336),
    "sepsq": dict(A=0, B=.206, C=0, D=0, P=.001, PF=0),
    "f32div": dict(A=.490, B=.496, C=.520, D=.598, P=.487, PF=.497),
    "direct": dict(A=0, B=.186, C=.167, D=.161, P=.183, PF=.166),
}


def _bits(a):
    return IC.f32_bits(a)


@pytest.mark.parametrize("name", FAMILIES)
def test_three_host_statements_agree(name):
    fam = IC.family(name)
    raw = fam["raw"]
    assert np.array_equal(CO.ipd(raw), fam["ipd"]) and np.array_equal(FN.ipd_f64(raw), fam["ipd"])
    with np.errstate(over="ignore", invalid="ignore"):
        c, n = CO.normalize_ipd(raw, True), FN.normalize_ipd(raw, True)
    assert np.array_equal(_bits(c), _bits(n))
    assert np.array_equal(_bits(c[fam["eng_face"], fam["eng_col"]]), _bits(fam["eng_want"]))
    f, col, want = IC.sample(fam, IC.sample_share(name))
    assert np.array_equal(_bits(c[f, col]), _bits(want))
    if len(fam["whole"]):
        assert np.array_equal(_bits(c[fam["whole"]]), _bits(IC.rational_rows(fam, fam["whole"])))
    ref, valid = IC.reference(name)
    assert np.array_equal(_bits(ref), _bits(c)) and np.array_equal(valid, ~FN.no_face_mask(n))
    print(f"family {name}: {len(raw)} faces, {len(fam['eng_face'])} engineered elements (k = -1 / 0 / +1: "
          f"{[int((fam['eng_k'] == k).sum()) for k in (-1, 0, 1)]}), {len(f)} sampled, {len(fam['whole'])} whole faces, "
          f"{int(np.isinf(ref).sum())} infinite and {int(((_bits(ref) & 0x7F800000) == 0).sum() - (ref == 0).sum())} subnormal results")


def _ipd_norm_host(repo_root, tmp_path, raw, *defines):
    """(normalised f32[B,1404], ipd f64[B]) from a host build of the shipped header."""
    exe = tmp_path / "ipd_norm_host"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", *defines, "-o", str(exe),
                    os.path.join(repo_root, "tests", "native", "ipd_norm_host.cpp")], check=True, capture_output=True, text=True)
    raw = np.ascontiguousarray(raw, np.float32).reshape(len(raw), -1)
    raw.tofile(tmp_path / "raw.f32")
    subprocess.run([str(exe), str(tmp_path / "raw.f32"), str(tmp_path / "out.f32"), str(tmp_path / "ipd.f64")], check=True)
    return np.fromfile(tmp_path / "out.f32", np.float32).reshape(raw.shape), np.fromfile(tmp_path / "ipd.f64", np.float64)


@pytest.mark.parametrize("name", FAMILIES)
def test_shipped_header_on_the_host(name, repo_root, tmp_path):
    fam = IC.family(name)
    out, ipd = _ipd_norm_host(repo_root, tmp_path, fam["raw"])
    ref, _ = IC.reference(name)
    assert out.shape == ref.shape and np.array_equal(_bits(out), _bits(ref))
    assert np.array_equal(ipd, fam["ipd"])


def test_old_residual_fails_on_the_signs_family(repo_root, tmp_path):
    """fma(-q, d, n) / fma(r, y, q) turns -0.0 / ipd into +0.0: family E shows it."""
    fam = IC.family("E")
    out, ipd = _ipd_norm_host(repo_root, tmp_path, fam["raw"], "-DIPD_NORM_OLD_RESIDUAL")
    ref, _ = IC.reference("E")
    assert np.array_equal(ipd, fam["ipd"])
    differ = _bits(out) != _bits(ref)
    assert differ.any() and (_bits(ref)[differ] == 0x80000000).all() and not (_bits(out)[differ] != 0).any()
    print(f"old residual: {int(differ.sum())} elements of family E come out +0.0 where the reference has -0.0")


def test_fx1_agrees_with_the_rational_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "fx1_normalise.npz"))
    raw = g["landmarks"]
    fam = {"raw": raw, "ipd_q": [IC.ref_ipd(f[IC.EYE_L], f[IC.EYE_R]) for f in raw]}
    assert np.array_equal(CO.ipd(raw), np.array([float(q) for q in fam["ipd_q"]]))
    want = IC.rational_rows(fam, range(len(raw)))
    assert np.array_equal(_bits(want), _bits(g["features_norm"])) and np.array_equal(_bits(want), _bits(CO.normalize_ipd(raw, True)))
    assert np.array_equal(_bits(want), _bits(FN.normalize_ipd(raw, True)))


def test_zeros_and_signs_family():
    ref, valid = IC.reference("E")
    raw = IC.family("E")["raw"].reshape(9, -1)
    assert not valid[:7].any() and valid[7] and valid[8]
    assert not (_bits(ref[:4]) != 0).any()                                            # +0.0 everywhere
    neg = (_bits(raw) == 0x80000000)
    neg[:, 3:6] = False
    assert np.array_equal(_bits(ref[4:6]) == 0x80000000, neg[4:6]) and neg[4].sum() == 1401 and 300 < neg[5].sum() < 1100
    assert not (_bits(ref[6]) != 0).any()                                             # -0.0 - (-0.0) = +0.0
    assert (ref[7] != 0).sum() == 1 and 0 < ref[7, 601] < 2.0 ** -126                 # one subnormal
    assert _bits(ref[8])[302] == 0x80000000 and ref[8, 1403] == np.float32(2.0 ** -149) and ref[8, 99] == 1.0


@pytest.mark.parametrize("name", ENGINEERED)
def test_families_are_what_they_claim(name):
    fam = IC.family(name)
    raw = fam["raw"].reshape(len(fam["raw"]), -1)
    assert set(fam["eng_col"].tolist()) == set(IC.ENG_COLS.tolist()) and len(fam["eng_col"]) == 1395
    worst = Fraction(0)
    for f, c, m in zip(fam["eng_face"], fam["eng_col"], fam["eng_m"]):
        n = Fraction(float(raw[f, c])) - Fraction(float(raw[f, 3 + c % 3]))
        assert IC.rn64(n) == n                                                         # v - r is exact in f64
        worst = max(worst, abs(n / fam["ipd_q"][f] - Fraction(m)) / IC._ulp53(m))
        mant = np.frexp(m)[0] * 2.0 ** 25
        assert (mant == int(mant) and int(mant) & 1) or abs(m) < 2.0 ** -126           # an f32 midpoint (subnormal: odd multiple of 2^-150)
    assert worst <= 2, worst
    if name == "A":
        assert all(q == Fraction(np.float32(float(q)).item()) for q in fam["ipd_q"])  # a 24-bit ipd
    if name == "C":
        assert all(q == IC.ONE_MICRO for q in fam["ipd_q"]) and fam["raw"].any(axis=(1, 2)).all()
    if name == "B":
        vis = np.mean([IC.ref_ipd(f[IC.EYE_L], f[IC.EYE_R], fused_chain=False) != q for f, q in zip(fam["raw"], fam["ipd_q"])])
        inexact = np.mean([q * q != IC.ref_radicand(f[IC.EYE_L], f[IC.EYE_R]) for f, q in zip(fam["raw"], fam["ipd_q"])])
        print(f"family B: the fma chain's ipd differs from separately rounded squares on {vis:.1%} of the faces")
        assert vis >= 1 / 3 and inexact == 1.0
    print(f"family {name}: engineered quotients within {float(worst):.2f} f64 ulps of their midpoints")


def _variants(fam):
    """{variant: bool[n]}: the variant's f32 bits differ from the rational reference's on that engineered element."""
    raw = fam["raw"].reshape(len(fam["raw"]), -1)
    f, c = fam["eng_face"], fam["eng_col"]
    n = raw[f, c].astype(np.float64) - raw[f, 3 + c % 3].astype(np.float64)
    ipd = fam["ipd"][f]
    sep = np.array([float(IC.ref_ipd(r[IC.EYE_L], r[IC.EYE_R], fused_chain=False)) for r in fam["raw"]])[f]
    with np.errstate(over="ignore", under="ignore"):
        out = {
            "nofma": (n * (1.0 / ipd)).astype(np.float32),
            "ipd_up": (n / np.nextafter(ipd, np.inf)).astype(np.float32),
            "ipd_dn": (n / np.nextafter(ipd, 0.0)).astype(np.float32),
            "sepsq": (n / sep).astype(np.float32),
            "f32div": n.astype(np.float32) / ipd.astype(np.float32),
            "direct": np.array([IC.ref_element(float(raw[i, j]), float(raw[i, 3 + j % 3]), fam["ipd_q"][i], direct=True) for i, j in zip(f, c)],
                               np.float64).astype(np.float32),
        }
        assert np.array_equal(_bits((n / ipd).astype(np.float32)), _bits(fam["eng_want"]))      # the emulation's own baseline
    return {k: _bits(v) != _bits(fam["eng_want"]) for k, v in out.items()}


_power: dict = {}


def _power_of(name):
    if name not in _power:
        _power[name] = {k: float(v.mean()) for k, v in _variants(IC.family(name)).items()}
    return _power[name]


def test_power_against_the_wrong_variants():
    print("share of the engineered elements a wrong variant changes, %:")
    print(f"    {'variant':8s}" + "".join(f"{n:>7s}" for n in ENGINEERED))
    for v in VARIANTS:
        print(f"    {v:8s}" + "".join(f"{100 * _power_of(n)[v]:7.1f}" for n in ENGINEERED))
    for v in VARIANTS:
        assert max(_power_of(n)[v] for n in ENGINEERED) > 0, v
        for n in ENGINEERED:
            assert _power_of(n)[v] >= 0.5 * MEASURED[v][n], (v, n, _power_of(n)[v], MEASURED[v][n])
    for n in ("B", "C"):
        assert _power_of(n)["direct"] > 0, f"family {n} has no double-rounding case"


def test_readout_certificate():
    """The read-out network hands the engineered x to the pose, and a one-ulp nudge of x shows."""
    fam = IC.family("P")
    feats, _ = IC.reference("P")
    f, c = fam["eng_face"], fam["eng_col"]
    near = IC.nudged(feats, fam)
    assert (_bits(near[f, c]) != _bits(feats[f, c])).all() and (np.abs(feats[f, c]) >= 0.125).all() and (np.abs(feats[f, c]) <= 1).all()
    assert (np.sign(feats[f, c]) > 0).any() and (np.sign(feats[f, c]) < 0).any()
    mask = np.ones(feats.shape, bool)
    mask[f, c] = False
    mask[:, [99, 100, 101, 789, 790, 791]] = False
    assert not feats[mask].any()                                                   # everything else is exactly zero
    for shift in (IC.READOUT_EXACT_SHIFT, 0):
        P = EH.Params(*IC.readout_net(shift))
        a, b = CO.encoder_heads(feats, P, order=2), CO.encoder_heads(near, P, order=2)
        moved = (_bits(a) != _bits(b))[f, c % 3].mean()
        print(f"read-out net, shift {shift}: a one-ulp nudge of x moves the pose bits on {moved:.1%} of the engineered elements")
        assert moved >= 0.5
        if shift:
            assert np.array_equal(_bits(a[f, c % 3]), _bits(feats[f, c])) and np.array_equal(_bits(b[f, c % 3]), _bits(near[f, c]))
