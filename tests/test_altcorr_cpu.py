"""CPU-side checks of the on-the-fly correlation block: the windowed restatement tests/altcorr_ref.py against the all-pairs
restatement tests/corr_ref.py (pooling is linear, so in fp64 they are one function), the argument checks of the dvs_altcorr_*
entries (they fail before any launch), and the error AlternateCorrBlock raises without a GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import altcorr_ref as A
import corr_ref as R
from conftest import ROOT

NEW = ["dvs_altcorr_sizes", "dvs_altcorr_pool", "dvs_altcorr_fwd", "dvs_altcorr_bwd", "dvs_altcorr_unpool"]


@pytest.mark.parametrize("shape", [(2, 24, 17, 23, 4, 3), (3, 36, 33, 31, 4, 4)], ids=["17x23", "33x31"])
def test_windowed_restatement_is_the_all_pairs_restatement(shape):
    """Outputs of two lookups and both gradients in fp64, to 1e-12 of the largest |value| of each."""
    B, Cn, H, W, L, r = shape
    f1, f2, coords, douts = R.make_case(B, Cn, H, W, L, r, n_lookups=2, seed=3)
    want = R.grads(f1.double(), f2.double(), coords, douts, L, r)
    got = A.grads(f1.double(), f2.double(), coords, douts, L, r)
    pairs = [("out%d" % k, g, w) for k, (g, w) in enumerate(zip(got[0], want[0]))]
    pairs += [("dfmap1", got[1], want[1]), ("dfmap2", got[2], want[2])]
    for name, g, w in pairs:
        assert g.dtype == torch.float64 and g.shape == w.shape, name
        err, top = float((g - w).abs().max()), float(w.abs().max())
        print("%s: |err| %.3e of max %.3e" % (name, err, top))
        assert err <= 1e-12 * top, (name, err, top)
    assert any(bool((o == 0).any()) for o in got[0])                # the zero padding is exercised, and exact


def test_windowed_restatement_runs_in_fp32():
    f1, f2, coords, douts = R.make_case(1, 8, 9, 10, 2, 1)
    outs, g1, g2 = A.grads(f1, f2, coords, douts, 2, 1)
    assert outs[0].dtype == g1.dtype == g2.dtype == torch.float32


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


def test_new_symbols_are_exported_and_declared(built):
    l = built.lib()
    src = open(os.path.join(ROOT, "include", "dvslam.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert hasattr(l, name), name
        assert name in built.exported_symbols(), name
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert built.ABI_VERSION == 12 and l.dvs_abi_version() == 12


def _cfg(built, B, Cn, H, W, L, r):
    cfg = built.CorrCfg()
    cfg.B, cfg.C, cfg.H, cfg.W, cfg.num_levels, cfg.radius = B, Cn, H, W, L, r
    return cfg


def test_sizes_has_no_volume_limit(built):
    l = built.lib()
    cfg = _cfg(built, 1, 8, 184, 256, 4, 2)
    floats, ws = C.c_size_t(), C.c_size_t()
    assert l.dvs_altcorr_sizes(C.byref(cfg), C.byref(floats), C.byref(ws)) == 0, l.dvs_last_error()
    assert floats.value == 8 * (92 * 128 + 46 * 64 + 23 * 32) and ws.value >= 256
    assert l.dvs_corr_sizes(C.byref(cfg), None, None, None) < 0 and b"2^31" in l.dvs_last_error()
    cfg.fmap1_nchw = cfg.fmap2_nchw = 1
    assert l.dvs_altcorr_sizes(C.byref(cfg), None, C.byref(ws)) == 0 and ws.value >= 2 * 4 * 8 * 184 * 256
    one = _cfg(built, 2, 8, 16, 16, 1, 4)
    assert l.dvs_altcorr_sizes(C.byref(one), C.byref(floats), None) == 0 and floats.value == 4


def test_sizes_rejects_what_the_all_pairs_form_rejects(built):
    l = built.lib()
    sizes = lambda cfg: l.dvs_altcorr_sizes(C.byref(cfg), None, None)
    cfg = _cfg(built, 2, 24, 17, 23, 4, 3)
    assert sizes(cfg) == 0
    cfg.C = 6
    assert sizes(cfg) < 0 and b"multiple of 4" in l.dvs_last_error()
    cfg.C, cfg.H = 24, 15
    assert sizes(cfg) < 0 and b"fewer than 2" in l.dvs_last_error()
    cfg.H, cfg.radius = 17, 9
    assert sizes(cfg) < 0 and b"radius" in l.dvs_last_error()
    cfg.radius, cfg.num_levels = 3, 9
    assert sizes(cfg) < 0 and b"num_levels" in l.dvs_last_error()
    big = _cfg(built, 64, 4, 1024, 1024, 4, 4)                      # B * L * (2r+1)^2 * H * W = 2.2e10
    assert sizes(big) < 0 and b"2^31" in l.dvs_last_error()


def test_null_pointers_fail_before_any_launch(built):
    l = built.lib()
    cfg = _cfg(built, 2, 24, 17, 23, 4, 3)
    calls = [
        lambda: l.dvs_altcorr_sizes(None, None, None),
        lambda: l.dvs_altcorr_pool(C.byref(cfg), None, None, None, None, None),
        lambda: l.dvs_altcorr_fwd(C.byref(cfg), None, None, None, None, None, None, 0, None),
        lambda: l.dvs_altcorr_bwd(C.byref(cfg), None, None, None, None, None, None, 0, None, None, None, None),
        lambda: l.dvs_altcorr_unpool(C.byref(cfg), None, None, None),
    ]
    for name, call in zip(NEW, calls):
        assert call() < 0 and b"null" in l.dvs_last_error(), name


def test_cpu_tensors_are_rejected(built):
    from deep_visual_slam_amd import raft_corr
    with pytest.raises(built.DvsError, match="no CPU path"):
        raft_corr.AlternateCorrBlock(torch.zeros(1, 4, 16, 16), torch.zeros(1, 4, 16, 16))
    with pytest.raises(NotImplementedError):                        # what the drop-in's callers caught before the block existed
        raft_corr.AlternateCorrBlock(None, None)
    with pytest.raises(built.DvsError) as e:                        # CorrBlock's own exceptions are what they were
        raft_corr.CorrBlock(torch.zeros(1, 4, 16, 16), torch.zeros(1, 4, 16, 16))
    assert not isinstance(e.value, NotImplementedError)


def test_altcorr_bytes():
    from deep_visual_slam_amd import raft_corr
    assert raft_corr.altcorr_bytes(1, 32, 48, 64, 4, 3) == 4 * 32 * (24 * 32 + 12 * 16 + 6 * 8) + 4 * 4 * 49 * 48 * 64
