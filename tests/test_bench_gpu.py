"""bench.py --dump-outputs on the GPU: two runs with the same arguments write the same arrays up to the rounding of the
step's float atomics (the inputs are seeded and the timed Adam pass keeps the weights, bench.TIMED_LR)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out_dir], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return {f[:-4]: np.load(os.path.join(out_dir, f)).astype(np.float64) for f in sorted(os.listdir(out_dir))}


def test_dump_outputs_repeat(gpu_device, tmp_path):
    a, b = _run(str(tmp_path / "a")), _run(str(tmp_path / "b"))
    assert a.keys() == b.keys() and "loss" in a and "disp_0" in a
    for k in a:
        assert a[k].shape == b[k].shape, k
        rel = np.linalg.norm(a[k] - b[k]) / max(np.linalg.norm(a[k]), 1e-30)
        assert rel < 1e-5, (k, rel)                     # measured <= 4e-7; a drifting trajectory of weights gives ~1e-1
