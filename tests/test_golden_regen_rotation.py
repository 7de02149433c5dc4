"""FX12's recipe is reproducible: tests/golden/make_golden_rotation.py, run against /root/reference, regenerates the committed
fixture bit for bit.  Skipped where the reference is absent (the GPU box): the fixture itself travels, the reference does not."""
import os
import subprocess
import sys

import numpy as np
import pytest

REF = "/root/reference"
FX12 = "fx12_rotation_tensor.npz"


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference checkout")
def test_fx12_regenerates_bit_identically(tmp_path, repo_root, golden_dir):
    env = dict(os.environ, NLML_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    # run from the repo root ON PURPOSE: it holds files named like the reference's modules, which must not shadow them
    res = subprocess.run([sys.executable, os.path.join(golden_dir, "make_golden_rotation.py")], cwd=repo_root, env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "ms per cell" in res.stdout
    a, b = np.load(os.path.join(str(tmp_path), FX12)), np.load(os.path.join(golden_dir, FX12))
    assert set(a.files) == set(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), k          # floats are stored as their bit patterns; the rest are integers and poses
