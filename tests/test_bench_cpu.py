"""bench.py's host side: what --dump-outputs writes (dtypes, size limit, seeded samples, no materialisation of the lazy
outputs) and the argument checks that run before any GPU work."""
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT

import bench
from deep_visual_slam_amd.learner_new import LazyOutputs


def _step_outputs(B, H, W):
    g = torch.Generator().manual_seed(0)
    out = LazyOutputs({("disp", s): torch.rand(B, 1, H >> s, W >> s, generator=g) for s in range(4)})
    for f in (-1, 1):
        out[("axisangle", 0, f)] = torch.rand(B, 1, 1, 3, generator=g)
        out[("translation", 0, f)] = torch.rand(B, 1, 1, 3, generator=g)
        out[("cam_T_cam", 0, f)] = torch.rand(B, 4, 4, generator=g)

    def fill(o):
        raise AssertionError("dump_outputs materialised the lazy outputs")
    out._thunk = fill
    losses = {"loss/%d" % s: torch.tensor(0.1 * (s + 1)) for s in range(4)}
    losses["loss"] = torch.tensor(0.25)
    return out, losses


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_headline_shapes(tmp_path):
    out, losses = _step_outputs(12, bench.H, bench.W)
    bench.dump_outputs(str(tmp_path / "a"), out, losses)
    bench.dump_outputs(str(tmp_path / "b"), out, losses)
    a, b = _read(tmp_path / "a"), _read(tmp_path / "b")
    assert set(a) == {"loss", "loss_0", "loss_1", "loss_2", "loss_3", "disp_0", "disp_1", "disp_2", "disp_3",
                      "axisangle_0_-1", "axisangle_0_1", "translation_0_-1", "translation_0_1", "cam_T_cam_0_-1", "cam_T_cam_0_1"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    assert a["loss"].dtype == np.float64 and float(a["loss"]) == float(losses["loss"])
    assert np.array_equal(a["disp_0"], out[("disp", 0)].numpy())                        # written whole at the bench's batch
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_dump_outputs_samples_large_outputs(tmp_path):
    out, losses = _step_outputs(48, bench.H, bench.W)                                   # a --batch override: disp_0 is 14.7 M
    bench.dump_outputs(str(tmp_path / "a"), out, losses)
    bench.dump_outputs(str(tmp_path / "b"), out, losses)
    a, b = _read(tmp_path / "a"), _read(tmp_path / "b")
    assert "disp_0" not in a and a["disp_0_sample"].shape == (bench.DUMP_SAMPLE,)
    assert np.isin(a["disp_0_sample"], out[("disp", 0)].numpy()).all()
    assert np.array_equal(a["disp_0_sample"], b["disp_0_sample"])                      # same positions run after run
    assert a["disp_1"].shape == (48, 1, bench.H // 2, bench.W // 2)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       cwd=ROOT, timeout=300)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr
