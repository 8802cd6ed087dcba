"""CPU-side checks of the RAFT correlation block: the restatement tests/corr_ref.py against the fixture recorded from the
reference's own CorrBlock (tests/golden/make_golden_corr.py), the tap order spelled out, the argument checks of the C-ABI
entries (they fail before any launch), and the drop-in import path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import corr_ref as R
from conftest import ROOT, load_golden

FIXTURE = "corr_b2_c24_17x23.npz"
DROPIN = os.path.join(ROOT, "deep-visual-slam_amd", "dropin")
REFERENCE = "/root/reference"


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


def t64(a):
    return torch.from_numpy(np.asarray(a)).double()


def test_ref_fp64_reproduces_the_reference_block(rec):
    """Outputs of both lookups and both gradients; the fixture is the reference's fp32 run, so the bound is 3 x the error that
    run had against the reference's own fp64 run (recorded by the generator)."""
    B, Cn, H, W, L, r = (int(v) for v in rec["meta/shape"])
    coords = [t64(rec["in/coords0"]), t64(rec["in/coords1"])]
    dout = t64(rec["in/dout"])
    outs, g1, g2 = R.grads(t64(rec["in/fmap1"]), t64(rec["in/fmap2"]), coords, [dout, dout], L, r)
    b_out, b_grad = 3.0 * float(rec["meta/ref_fp32_err_out"]), 3.0 * float(rec["meta/ref_fp32_err_grad"])
    for k, o in enumerate(outs):
        want = rec["ref/out%d" % k]
        assert tuple(o.shape) == want.shape == (B, L * (2 * r + 1) ** 2, H, W)
        for i, sl in enumerate(R.level_slices(L, r)):
            err = float((o[:, sl] - t64(want[:, sl])).abs().max())
            print("lookup %d level %d: |err| %.3e, bound %.3e" % (k, i, err, b_out))
            assert err <= b_out, (k, i, err, b_out)
    for name, g, want in (("dfmap1", g1, rec["ref/dfmap1"]), ("dfmap2", g2, rec["ref/dfmap2"])):
        err = float((g - t64(want)).abs().max())
        print("%s: |err| %.3e, bound %.3e" % (name, err, b_grad))
        assert err <= b_grad, (name, err, b_grad)


def test_tap_order():
    """One level, r = 1, integer coordinates: channel a * 3 + e of pixel (y, x) is vol[y + e - 1, x + a - 1] -- the x offset is
    the slow index (corr.py:37-43 stacks meshgrid(dy, dx) onto (x, y) coordinates)."""
    gen = torch.Generator().manual_seed(3)
    B, Cn, H, W = 1, 4, 5, 6
    f1, f2 = torch.randn(B, Cn, H, W, generator=gen).double(), torch.randn(B, Cn, H, W, generator=gen).double()
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    coords = torch.stack([xs, ys])[None].double()
    out = R.corr_block(f1, f2, [coords], 1, 1)[0]
    vol = R.volume(f1, f2).reshape(B, H, W, H, W)
    for y in range(H):
        for x in range(W):
            for a in range(3):
                for e in range(3):
                    yy, xx = y + e - 1, x + a - 1
                    want = float(vol[0, y, x, yy, xx]) if 0 <= yy < H and 0 <= xx < W else 0.0
                    assert abs(float(out[0, a * 3 + e, y, x]) - want) <= 1e-12, (y, x, a, e)


def test_floor_not_truncation():
    """A coordinate in (-1, 0) blends column -1 (zero padding) with column 0; truncation would read column 0 at full weight."""
    f1 = torch.zeros(1, 4, 2, 2, dtype=torch.float64)
    f1[0, 0, 0, 0] = 2.0
    f2 = torch.ones(1, 4, 2, 2, dtype=torch.float64)
    coords = torch.zeros(1, 2, 2, 2, dtype=torch.float64)
    coords[0, 0] = -0.25
    out = R.corr_block(f1, f2, [coords], 1, 0)[0]
    assert abs(float(out[0, 0, 0, 0]) - 0.75) <= 1e-15           # volume row of pixel 0 is all 1: weight 0.75 on column 0


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


def test_abi_rejects_bad_shapes_before_any_launch(built):
    l = built.lib()
    sizes = lambda cfg: l.dvs_corr_sizes(C.byref(cfg), None, None, None)
    cfg = built.CorrCfg()
    cfg.B, cfg.C, cfg.H, cfg.W, cfg.num_levels, cfg.radius = 2, 24, 17, 23, 4, 3
    floats, ws = C.c_size_t(), C.c_size_t()
    offs = (C.c_size_t * 4)()
    assert l.dvs_corr_sizes(C.byref(cfg), C.byref(floats), offs, C.byref(ws)) == 0
    n = 17 * 23
    assert floats.value == 2 * n * (n + 88 + 20 + 4) and list(offs) == [0, 2 * n * n, 2 * n * (n + 88), 2 * n * (n + 108)]
    assert ws.value >= 2 * 2 * 112 * 24 * 4
    cfg.C = 6
    assert sizes(cfg) < 0 and b"multiple of 4" in l.dvs_last_error()
    cfg.C, cfg.H = 24, 15
    assert sizes(cfg) < 0 and b"fewer than 2" in l.dvs_last_error()
    cfg.H, cfg.radius = 17, 9
    assert sizes(cfg) < 0 and b"radius" in l.dvs_last_error()
    cfg.radius = 3
    assert l.dvs_corr_build(C.byref(cfg), None, None, None, None, None) < 0 and b"null" in l.dvs_last_error()
    assert l.dvs_corr_lookup_fwd(C.byref(cfg), None, None, None, 0, None) < 0 and b"null" in l.dvs_last_error()
    assert l.dvs_corr_lookup_bwd(C.byref(cfg), None, None, 0, None, None) < 0 and b"null" in l.dvs_last_error()
    assert l.dvs_corr_volume_bwd(C.byref(cfg), None, None, None, None, None, None, None) < 0 and b"null" in l.dvs_last_error()


def test_cpu_tensors_are_rejected(built):
    from deep_visual_slam_amd import raft_corr
    with pytest.raises(built.DvsError):
        raft_corr.CorrBlock(torch.zeros(1, 4, 16, 16), torch.zeros(1, 4, 16, 16))


SHIM = r"""
import model.raft.core.corr as c
assert c.CorrBlock.__module__.startswith("deep_visual_slam_amd"), c.CorrBlock.__module__
try:
    c.AlternateCorrBlock(None, None)
except NotImplementedError:
    print("SHIM-OK")
"""

RAFT = r"""
import model.raft.core.raft as r
import model.raft.core.update as u
assert r.CorrBlock.__module__.startswith("deep_visual_slam_amd"), r.CorrBlock.__module__
assert not u.__file__.startswith(%r), u.__file__
assert hasattr(r, "SmallRAFT") and hasattr(r, "coords_grid")
print("RAFT-OK")
"""


def _run(script, path):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join(path)
    return subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, cwd="/tmp", timeout=300)


def test_dropin_corr_resolves_to_this_package():
    r = _run(SHIM, [DROPIN])
    assert "SHIM-OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "model", "raft", "core")), reason="the reference tree is not here")
def test_reference_raft_imports_through_the_shim():
    r = _run(RAFT % DROPIN, [DROPIN, REFERENCE])
    assert "RAFT-OK" in r.stdout, r.stdout + r.stderr
