"""The shared inputs of tests/test_tucker_order_host.py and tests/test_tucker_order_gpu.py: the shapes at which the four primitives of
the Tucker decomposition (csrc/tucker_decompose.hip, K7a..K7d) take another path, the deterministic draws that go through them, and
the exact answers where the inputs are exactly summable.  The host file shows on the CPU that these inputs tell the kernels' summation
orders (oracle/csrc/oracle.c, "K7") from wrong ones; the GPU file holds the device to the models bit for bit.
"""
import itertools

import numpy as np

import tucker_cases as TC

KCH = 4096                       # NLML_GRAM_KCHUNK
TILE_BYTES = 128 * 128 * 8       # one workspace tile of K7a

# ---- the shapes -----------------------------------------------------------------------------------------------------------------
# K7a (I, K) -> (tile pairs, slices), by the header's rule; the workspace query must say pairs * slices tiles
K7A_EXACT = {(257, 40): (6, 1),            # three tile rows, the last tile has one row
             (257, 4129): (6, 2),          # the last slice has 33 columns
             (385, 8200): (10, 3),
             (4096, 4100): (528, 1),       # NLML_GRAM_I_MAX; one slice of 4,128
             (2049, 24600): (153, 6)}      # slices LENGTHENED to 4,128 (the last 3,960) together with split-K
K7A_EXACT_F64 = [(257, 40), (257, 4129), (385, 8200)]
K7A_EXACT_HOST = K7A_EXACT_F64            # the ones the host model runs in seconds
K7A_RANDOM = {(17, 2 * KCH + 7): (1, 3), (130, KCH + 33): (3, 2), (257, 4129): (6, 2)}
K7A_UNALIGNED = (17, KCH + 32)

K7B_EXACT = [(260, 3, 2, 2, 132),          # 1,300 f32 slabs and 2,340 f64 slabs over 1,024 workgroups: two and three trips
             (1, 32, 24, 1, 33),           # 768 cells (the LDS limit); n > 16 for yaw and pitch
             (1, 3, 8, 32, 5),             # 768 cells; n > 16 for roll, J = 1
             (3, 2, 17, 20, 36),           # 16 < n < 32 for pitch (O > 1, J > 1) and for roll
             (2, 17, 5, 9, 40)]            # 765 cells; n = 17 for yaw
K7B_RANDOM = [(37, 5, 4, 3, 100), (260, 3, 2, 2, 132), (1, 32, 2, 2, 33)]
K7B_UNALIGNED = (37, 5, 4, 3, 100)
K7B_WHICH = [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]   # what the driver asks for

K7C_EXACT = (17, 300)
K7C_RANDOM = [(37, 6000), (130, 300)]
K7C_RANKS = (1, 5, 16)

K7D_EXACT = (2, 4, 3, 5, 7)
K7D_RANDOM = [(37, 5, 4, 3, 100), (3, 11, 9, 7, 64)]
K7D_RANKS = [(3, 3, 3), (2, 1, 3)]
NULLS = list(itertools.product((0, 1), repeat=3))          # 1: that factor is None
DTYPES = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]   # (in, out)

# the wrong orders of the C models, by variant number
K7A_VARIANTS = {1: "k descending", 2: "multiply and add rounded separately", 3: "one chain over K, no slices", 4: "slices added descending"}
K7B_VARIANTS = {1: "a contiguous quarter of (o, j) per wave", 2: "32-column slabs for f64 input", 3: "partials added descending"}
K7C_VARIANTS = {1: "i descending", 2: "multiply and add rounded separately", 3: "U rounded to f32"}
K7D_VARIANTS = {1: "descending", 2: "multiply and add rounded separately", 3: "Kronecker form", 4: "yaw innermost"}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def mismatches(a, b) -> int:
    """Words that differ (shapes and dtypes must agree; no NaN is expected on either side)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((bits(a) != bits(b)).sum())


def slabs(shape, tc):
    return shape[0] * -(-shape[4] // tc)


# ---- exactly summable inputs ----------------------------------------------------------------------------------------------------------
def exact_tensor(shape):
    """Integer-valued f32, |x| <= 1024 (tucker_cases.exact_ints), by a seed of the shape."""
    return TC.exact_ints(shape, seed=7 + sum(s * 31 ** k for k, s in enumerate(shape)) % 2 ** 31)


def exact_factor(n, r, seed):
    """Integer-valued f64 [n,r], |u| <= 64."""
    return np.random.default_rng(seed).integers(-64, 65, size=(n, r)).astype(np.float64)


def exact_gram(A):
    """A integer-valued, |a| <= 1024, K < 2^33: every partial sum is an integer below 2^53, so the f64 product is the integer Gram
    whatever order BLAS adds in; small cases go through int64 itself."""
    if A.shape[0] ** 2 * A.shape[1] <= 5e7:
        Ai = A.astype(np.int64)
        G = (Ai @ Ai.T).astype(np.float64)
    else:
        A64 = A.astype(np.float64)
        G = A64 @ A64.T
    assert np.all(G == np.rint(G)) and np.abs(G).max() < 2.0 ** 53
    return G


def exact_pose_grams(X):
    return [exact_gram(TC.unfold(X, m)) for m in (1, 2, 3)]


def contract_pose(T, Us):
    """T x_2 Uy^T x_3 Up^T x_4 Ur^T in T's own arithmetic (int64 for the exact cases, f64 for the reference), None keeping a mode."""
    for m, U in zip((1, 2, 3), Us):
        if U is not None:
            T = TC.contract(T, U.astype(T.dtype), m)
    return T


def exact_pose(X, Us, out_dtype):
    """The int64 contraction of exactly summable X and integer factors, cast once: below 2^53 (1024 * 64^3 * 32 * 24 terms at the
    very most) the f64 image is the integer itself, and the f32 output is its one rounding."""
    T = contract_pose(X.astype(np.int64), Us)
    assert np.abs(T).max() < 2 ** 53
    return T.astype(np.float64).astype(out_dtype)


def exact_identity(A, U, out_dtype):
    T = U.astype(np.int64).T @ A.astype(np.int64)
    assert np.abs(T).max() < 2 ** 53
    return T.astype(np.float64).astype(out_dtype)


def pose_factors(shape, ranks, nulls, make):
    """The three factors of ranks `ranks`, None where nulls says so; make(n, r, mode) builds one."""
    return [None if z else make(n, r, k) for k, (n, r, z) in enumerate(zip(shape[1:4], ranks, nulls))]


# ---- random inputs --------------------------------------------------------------------------------------------------------------
def random_matrix(shape):
    """Standard normal f32 [I,K]."""
    return np.random.default_rng(shape[0] * 100003 + shape[1]).normal(size=shape).astype(np.float32)


def random_matrix64(shape):
    """Standard normal f64 [I,K], unrounded: what the f64 form of K7a takes from a projection."""
    return np.random.default_rng(shape[0] * 100019 + shape[1]).normal(size=shape)


def random_tensor(shape):
    """-> (f32 tensor, f64 tensor): standard normal draws unrounded (what the f64 forms of K7d take) and their f32 rounding."""
    X64 = np.random.default_rng(sum(s * 37 ** k for k, s in enumerate(shape)) % 2 ** 31).normal(size=shape)
    return X64.astype(np.float32), X64


def random_factor(n, r, seed):
    return np.random.default_rng(seed).normal(size=(n, r))


def random_pose_factors(shape, ranks, nulls):
    full = [random_factor(n, 3, 1000 + 10 * sum(shape) + k) for k, n in enumerate(shape[1:4])]
    return pose_factors(shape, ranks, nulls, lambda n, r, k: np.ascontiguousarray(full[k][:, :r]))


def exact_pose_factors(shape, ranks, nulls):
    full = [exact_factor(n, 3, 2000 + 10 * sum(shape) + k) for k, n in enumerate(shape[1:4])]
    return pose_factors(shape, ranks, nulls, lambda n, r, k: np.ascontiguousarray(full[k][:, :r]))


def one_past(flat, numel):
    """A buffer of numel + 2 elements holding `flat` from element 1, NaN before and after it: the contiguous view [1 : 1 + numel] of
    a 16-byte aligned buffer starts 4 bytes past the alignment."""
    buf = np.full(numel + 2, np.nan, np.float32)
    buf[1:1 + numel] = np.asarray(flat, np.float32).reshape(-1)
    return buf
