"""CPU: ties tests/cr_reference.py -- the yardstick of tests/test_td_fvec_exact_gpu.py -- to the host build of csrc/cr_cos.h, and checks,
from the reference alone, the conditions those GPU tests rest on: that every tie / near-tie input really sends the header down its
double-double path (also with a library cos 2 ulp off, the header's premise for the device library), that the inputs fall on both
sides of and onto the float32 tie, and that a one-ulp error of the cos / sin would show in the float32 often enough to be seen."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cr_reference as CR


@pytest.fixture(scope="module")
def host(tmp_path_factory, repo_root):
    """The header compiled for the host, as tests/test_abi_and_host.py and tests/test_td_gradient_host.py build it."""
    d = tmp_path_factory.mktemp("cr_host")
    libs = []
    for name in ("cr_cos_host", "cr_sin_host"):
        so = d / f"{name}.so"
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so),
                        os.path.join(repo_root, "tests", "native", f"{name}.cpp")], check=True, capture_output=True, text=True)
        libs.append(C.CDLL(str(so)))
    return libs


@pytest.fixture(scope="module")
def hard():
    return CR.hard_arguments(0)


def _p(v):
    return v.ctypes.data_as(C.c_void_p)


def _array_fn(fn, x):
    x = np.ascontiguousarray(x, np.float64)
    y = np.empty_like(x)
    fn(_p(x), _p(y), C.c_long(len(x)))
    return y


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint64 if v.dtype == np.float64 else np.uint32)


def test_host_cr_cos_is_the_correctly_rounded_cos_on_the_hard_arguments(host, hard):
    import math
    got, want = _array_fn(host[0].cr_cos_array, hard), CR.cr_cos(hard)
    libm = np.fromiter((math.cos(v) for v in hard), np.float64, len(hard))
    print(f"cr_cos on {len(hard)} hard arguments: {int((_bits(got) != _bits(want)).sum())} differ from the correctly rounded value; "
          f"the host libm differs on {int((libm != want).sum())}")
    assert len(hard) >= 90_000
    assert np.array_equal(_bits(got), _bits(want))


def test_host_cr_sin_is_the_correctly_rounded_sin_on_the_hard_arguments(host, hard):
    import math
    got, want = _array_fn(host[1].cr_sin_array, hard), CR.cr_sin(hard)
    libm = np.fromiter((math.sin(v) for v in hard), np.float64, len(hard))
    print(f"cr_sin on {len(hard)} hard arguments: {int((_bits(got) != _bits(want)).sum())} differ from the correctly rounded value; "
          f"the host libm differs on {int((libm != want).sum())}")
    assert np.array_equal(_bits(got), _bits(want))


def test_mpmath_and_the_decimal_series_round_to_the_same_doubles(hard):
    pytest.importorskip("mpmath")
    t = hard[np.random.default_rng(3).choice(len(hard), 200, replace=False)]
    t = np.concatenate([t[:-6], [0.0, -0.0, 5e-324, -1e-310, 2.0 ** 20, CR.nearest_k_half_pi([CR.K_MAX])[0]]])
    assert np.array_equal(_bits(CR.cr_cos(t, "mpmath")), _bits(CR.cr_cos(t, "decimal")))
    assert np.array_equal(_bits(CR.cr_sin(t, "mpmath")), _bits(CR.cr_sin(t, "decimal")))
    assert np.isnan(CR.cr_cos(np.array([np.nan, np.inf, -np.inf]))).all() and np.isnan(CR.cr_sin(np.array([np.nan, np.inf]))).all()


def _check_set(name, exact_tie, v, m, f, f_up, f_dn, fails):
    below, on, above = float((v < m).mean()), float((v == m).mean()), float((v > m).mean())
    up, dn = float((f_up != f).mean()), float((f_dn != f).mean())
    print(f"{name}: {len(m)} inputs, all fail the fast-path predicate at -2/0/+2 ulp: {bool(fails.all())}; below/on/above the tie "
          f"{below:.2f}/{on:.2f}/{above:.2f}; one ulp up changes {up:.3f} of the float32s, one ulp down {dn:.3f}")
    assert len(m) == CR.N_TIE and fails.all()
    if exact_tie:
        assert min(below, on, above) >= 0.10
    assert up >= 0.05 and dn >= 0.05                      # either direction alone, so an error of one sign cannot hide


def test_cos_tie_sets_are_hard_and_the_host_entry_equals_the_reference_on_them(host, tucker_art):
    for name, _, _, (a, b, c, d), w, m in CR.tie_cases_cos(tucker_art):
        n = len(w)
        arg = CR.argument(b, w, c)
        full = lambda s: np.full(n, s)
        fails = np.ones(n, bool)
        for u in (-2, 0, 2):
            fails &= CR.slow_path_cos(full(a), arg, full(d), ulps=u)
        cc = CR.cr_cos(arg)
        f = CR.f_from_cos(a, cc, d)
        assert np.array_equal(_bits(f), _bits(CR.f_entry(a, b, w, c, d)))
        _check_set(name, name.startswith("tie"), a * cc + d, m, f, CR.f_from_cos(a, np.nextafter(cc, np.inf), d),
                   CR.f_from_cos(a, np.nextafter(cc, -np.inf), d), fails)
        assert (np.abs(f.astype(np.float64) - m) <= np.spacing(np.abs(m).astype(np.float32))).all()      # f is one of m's two neighbours
        fast, slow = np.empty(n, np.float32), np.empty(n, np.float32)
        host[0].cr_fvalue_arrays(_p(full(a)), _p(arg), _p(full(d)), _p(fast), _p(slow), C.c_long(n))
        assert np.array_equal(_bits(fast), _bits(f)) and np.array_equal(_bits(slow), _bits(f)), name


def test_sin_tie_sets_are_hard_and_the_host_entry_equals_the_reference_on_them(host, tucker_art):
    for name, (a, b, c, _), w, m in CR.tie_cases_sin(tucker_art):
        n = len(w)
        arg = CR.argument(b, w, c)
        full = lambda s: np.full(n, s)
        fails = np.ones(n, bool)
        for u in (-2, 0, 2):
            fails &= CR.slow_path_sin(full(a), full(b), arg, ulps=u)
        ss = CR.cr_sin(arg)
        f = CR.df_from_sin(a, b, ss)
        assert np.array_equal(_bits(f), _bits(CR.df_entry(a, b, w, c)))
        _check_set(name, name.startswith("tie") and b == 1.0, ((-a) * b) * ss, m, f, CR.df_from_sin(a, b, np.nextafter(ss, np.inf)),
                   CR.df_from_sin(a, b, np.nextafter(ss, -np.inf)), fails)
        fast, slow = np.empty(n, np.float32), np.empty(n, np.float32)
        host[1].cr_dfvalue_arrays(_p(full(a)), _p(full(b)), _p(arg), _p(fast), _p(slow), C.c_long(n))
        assert np.array_equal(_bits(fast), _bits(f)) and np.array_equal(_bits(slow), _bits(f)), name


def test_the_predicate_restatement_is_the_headers(host):
    """slow_path_cos says where cr_f32_a_cos_d leaves its fast path; the header cannot be asked, but where the restatement says
    'fast path' the float is the library's own, so there fast == float32(a libm_cos + d) must hold -- it would not if the restated
    delta were wider than the header's -- and overall the failing share of a random draw is the header's 'once in 2^21' order."""
    rng = np.random.default_rng(9)
    n = 400_000
    a, t, d = rng.uniform(-12, 12, n), rng.uniform(-3.5, 3.5, n), rng.uniform(-12, 12, n)
    fast, slow = np.empty(n, np.float32), np.empty(n, np.float32)
    host[0].cr_fvalue_arrays(_p(a), _p(t), _p(d), _p(fast), _p(slow), C.c_long(n))
    sp = CR.slow_path_cos(a, t, d)
    lib = CR.f_entry_libm(a, 1.0, t, 0.0, d)
    print(f"random rows: {int(sp.sum())} of {n} fail the fast-path predicate")
    assert np.array_equal(_bits(fast[~sp]), _bits(lib[~sp]))
    assert sp.sum() <= 20
