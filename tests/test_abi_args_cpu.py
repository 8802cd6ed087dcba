"""Argument checks of the entry points that ABI 12 merged (include/dvslam.h): the BatchNorm backward pair now takes the forward's
[G][4][C] table and a y-mask flag, and the ordered weight gradient shares dvs_conv2d_wgrad's name.  Every check runs on the host
before any launch, so a bad call must come back negative, with its own name in dvs_last_error(), on a machine without a GPU."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


P = 4096          # a non-NULL "device pointer": nothing dereferences it before the checks fail
M, CH = 90, 64


def _reduce(l, dz=P, z=None, y=P, fin=P, ymask=0, du=None, sums=P, ws=P, m=M, c=CH, groups=1):
    return l.dvs_bn_bwd_reduce(dz, z, y, fin, ymask, du, sums, ws, m, c, groups, None)


def _apply(l, du=P, y=P, fin=P, ymask=0, gamma=P, sums=P, dy=P, m=M, c=CH, dgamma=None, dbeta=None, groups=1):
    return l.dvs_bn_bwd_apply(du, y, fin, ymask, gamma, sums, dy, m, c, dgamma, dbeta, groups, None)


BAD_CALLS = [
    ("reduce: y-mask with z", _reduce, dict(ymask=1, z=P)),
    ("reduce: y-mask with du", _reduce, dict(ymask=1, du=P)),
    ("reduce: C = 12", _reduce, dict(c=12)),
    ("reduce: groups = 0", _reduce, dict(groups=0)),
    ("reduce: NULL fin", _reduce, dict(fin=None)),
    ("apply: C = 12", _apply, dict(c=12)),
    ("apply: groups = 0", _apply, dict(groups=0)),
    ("apply: d gamma sink alone", _apply, dict(dgamma=P)),
    ("apply: d beta sink alone", _apply, dict(dbeta=P)),
    ("apply: NULL fin", _apply, dict(fin=None)),
]


@pytest.mark.parametrize("name,call,kw", BAD_CALLS, ids=[b[0] for b in BAD_CALLS])
def test_bn_backward_refuses(built, name, call, kw):
    l = built.lib()
    assert call(l, **kw) < 0
    assert (b"dvs_bn_bwd_reduce" if call is _reduce else b"dvs_bn_bwd_apply") in l.dvs_last_error()


def test_bn_backward_messages_say_what_is_wrong(built):
    l = built.lib()
    assert _reduce(l, ymask=1, z=P) < 0 and b"y-mask" in l.dvs_last_error()
    assert _reduce(l, c=12) < 0 and b"C/4 must divide 256 (C=12)" in l.dvs_last_error()
    assert _apply(l, dgamma=P) < 0 and b"gradient sinks come together" in l.dvs_last_error()


def test_conv2d_wgrad_refuses_a_short_workspace(built):
    l = built.lib()
    d = built.ConvDesc(2, 24, 32, 64, 128, 3, 3, 2, 1, 0)         # a split-K implicit-GEMM layer: it has a slab path
    need = l.dvs_conv2d_wgrad_workspace(C.byref(d), None, 0, 0)
    assert need > 0
    assert l.dvs_conv2d_wgrad(P, P, P, None, C.byref(d), None, None, 0, P, 0, None) < 0
    err = l.dvs_last_error()
    assert b"dvs_conv2d_wgrad" in err and b"workspace of 0 bytes" in err
