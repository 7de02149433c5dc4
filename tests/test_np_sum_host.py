"""numpy's pairwise np.sum as the library states it (nlml_hpe_amd/csrc/np_sum.h), built for the host (tests/native/np_sum_host.cpp) -- no GPU.

np_pairwise_sum against np.sum itself, bit for bit, on rows whose sum depends on the order of the additions (sixteen decimal orders of
magnitude between the elements): every length up to 299 and the lengths around the trees the kernels are laid out for (468 landmarks,
1,404 features) and around powers of two.  A left-to-right sum of the same rows gives other bits, which is asserted too: the comparison
cannot pass on an input that does not care about the order.  No row is made of negative zeros alone, the one case in which the
header is not np.sum by design (its comment).  Then the leaf tables of NpTree<N> against the same recursion written here."""
import os
import subprocess

import numpy as np
import pytest

from nlml_hpe_amd import synth

LENGTHS = list(range(1, 300)) + [467, 468, 469, 1023, 1024, 1025, 1403, 1404, 1405, 2047, 2048, 2049, 4097]
ROWS_PER_LENGTH = 3
TREES = (129, 136, 468, 1000, 1404)


@pytest.fixture(scope="module")
def program(repo_root, tmp_path_factory):
    exe = tmp_path_factory.mktemp("np_sum") / "np_sum_host"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", str(exe), os.path.join(repo_root, "tests", "native", "np_sum_host.cpp")],
                   check=True, capture_output=True, text=True)
    return exe


def _rows():
    g = synth.rng(47, 0)
    return [g.standard_normal(n) * 10.0 ** g.integers(-8, 8, n) for n in LENGTHS for _ in range(ROWS_PER_LENGTH)]


def _run(program, rows, tmp_path):
    with open(tmp_path / "rows.bin", "wb") as f:
        for r in rows:
            f.write(np.int32(len(r)).tobytes())
            f.write(np.ascontiguousarray(r, np.float64).tobytes())
    res = subprocess.run([str(program), str(tmp_path / "rows.bin"), str(tmp_path / "sums.f64")], check=True, capture_output=True, text=True)
    return np.fromfile(tmp_path / "sums.f64", np.float64), res.stdout


def test_pairwise_sum_is_np_sum_bit_for_bit(program, tmp_path):
    rows = _rows()
    assert not any((r == 0).all() and np.signbit(r).all() for r in rows)
    got, _ = _run(program, rows, tmp_path)
    want = np.array([np.sum(r) for r in rows])
    assert got.shape == want.shape == (len(LENGTHS) * ROWS_PER_LENGTH,)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, [(len(rows[i]), got[i], want[i]) for i in bad[:5]]
    # the input does its job: summed left to right, the rows give other bits (np.cumsum adds in sequence)
    seq = np.array([np.cumsum(r)[-1] for r in rows])
    differs = seq.view(np.uint64) != want.view(np.uint64)
    long_rows = np.array([len(r) >= 64 for r in rows])
    print(f"left to right differs from np.sum on {int(differs.sum())} of {len(rows)} rows, {int(differs[long_rows].sum())} of the "
          f"{int(long_rows.sum())} with 64 elements or more")
    assert differs[long_rows].mean() > 0.5
    for n in (468, 1404, 4097):
        assert differs[[i for i, r in enumerate(rows) if len(r) == n]].any(), n


def _leaves(n, base=0):
    """[(offset, length, depth)] of numpy's recursion over n elements."""
    if n <= 128:
        return [(base, n, 0)]
    h = n // 2 - (n // 2) % 8
    return [(o, k, d + 1) for o, k, d in _leaves(h, base) + _leaves(n - h, base + h)]


def test_leaf_tables_are_the_recursions(program, tmp_path):
    _, text = _run(program, [np.ones(8)], tmp_path)
    lines = [list(map(int, line.split())) for line in text.splitlines()]
    assert [line[0] for line in lines] == list(TREES)
    for n, leaves, balanced, *offs in lines:
        want = _leaves(n)
        assert leaves == len(want) and offs == [o for o, _, _ in want] + [n], n
        assert bool(balanced) == (len({d for _, _, d in want}) == 1), n
        assert all(8 <= k <= 128 for _, k, _ in want)
    by_n = {line[0]: line for line in lines}
    assert by_n[468][3:] == [0, 112, 232, 344, 468] and by_n[468][2] == 1
    assert by_n[1404][3:] == [0] + [80 + 88 * k for k in range(15)] + [1404] and by_n[1404][1:3] == [16, 1]
    assert by_n[129][1:] == [2, 1, 0, 64, 129] and by_n[136][3:] == [0, 64, 136] and by_n[1000][1] == 8
