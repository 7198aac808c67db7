"""The committed periodic leaf-parameter fixtures ARE what the reference produces (build container only; skipped where /root/reference is
absent).

tests/golden/make_golden_rj_periodic.py imports the real reference and writes tests/golden/rj_periodic/*.npz.  This test runs it into a
temporary directory and requires key-for-key, bit-for-bit equality with the committed files, doubles compared as their bit patterns: a
wrapped multiple of the period is +0.0.  Nothing here runs on the GPU box."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/src/eryn"), reason="the reference tree is not on this machine")


def test_generator_reproduces_every_committed_periodic_fixture(tmp_path):
    out = tmp_path / "rj_periodic"
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_rj_periodic.py")], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", GOLDEN_OUT=str(out)))
    assert r.returncode == 0, f"{r.stdout}\n{r.stderr}"
    made = sorted(os.path.basename(p) for p in glob.glob(str(out / "*.npz")))
    committed = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "rj_periodic", "*.npz")))
    assert made == committed and len(committed) == 4, (made, committed)
    narrays = 0
    for name in committed:
        new, old = np.load(out / name, allow_pickle=False), np.load(os.path.join(GOLDEN, "rj_periodic", name), allow_pickle=False)
        assert sorted(new.files) == sorted(old.files), f"{name}: keys differ ({set(new.files) ^ set(old.files)})"
        for k in old.files:
            a, b = new[k], old[k]
            assert a.dtype == b.dtype and a.shape == b.shape, f"{name}[{k}]: dtype / shape"
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f"{name}[{k}] differs from the reference's output"
            if a.dtype == np.float64:
                assert np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.int64), np.ascontiguousarray(b).reshape(-1).view(np.int64)), \
                    f"{name}[{k}]: a zero of the other sign"
            narrays += 1
        assert os.path.getsize(os.path.join(GOLDEN, "rj_periodic", name)) < 1 << 20
    assert narrays > 500
