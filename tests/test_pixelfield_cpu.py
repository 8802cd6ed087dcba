"""The view rule of csrc/pixelfield.h holds in every entry that takes the family's views: dvs_flow_consistency,
dvs_rigid_flow and dvs_pose_fit are offered the same bad flow view, the two that take a depth the same bad depth view, all three
the same bad shapes.  Each refuses before any launch (the pointers are fake, this needs no device), names itself, and says the same
thing as the others up to the name of the argument."""
import re

import pytest

P = 1 << 20       # non-NULL, 16-byte aligned "device pointers" a MiB apart: nothing dereferences them before the checks fail
N, H, W = 2, 5, 7
EXTENT = (H - 1) * W + W                                                               # of one plane whose rows are dense


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib.lib()


def _flow(p=5 * P, image=2 * EXTENT, plane=EXTENT, row=W):
    return (p, image, plane, row)


def _depth(p=P, image=EXTENT, row=W):
    return (p, image, row)


def _consistency(l, flow=_flow(), N=N, H=H, W=W):
    return l.dvs_flow_consistency(*flow, 2 * P, 2 * EXTENT, EXTENT, W, 3 * P, 4 * P, 6 * P, 7 * P, N, H, W, 0.01, 0.5, None)


def _rigid(l, flow=_flow(), depth=_depth(), N=N, H=H, W=W):
    return l.dvs_rigid_flow(*depth, 2 * P, 3 * P, 4 * P, *flow, 6 * P, 7 * P, 8 * P, 9 * P, N, H, W, 0.01, 0.5, 1e-7, None)


def _pose(l, flow=_flow(), depth=_depth(), N=N, H=H, W=W):
    return l.dvs_pose_fit(*depth, 2 * P, 3 * P, 4 * P, *flow, 6 * P, 7 * P, 8 * P, 9 * P, 10 * P, 480, N, H, W, 4, 1.0, 1e-6, 1e-7, None)


FLOW_ENTRIES = [("dvs_flow_consistency", _consistency, "a"), ("dvs_rigid_flow", _rigid, "flow"), ("dvs_pose_fit", _pose, "flow")]
DEPTH_ENTRIES = [("dvs_rigid_flow", _rigid, "depth"), ("dvs_pose_fit", _pose, "depth")]

BAD_FLOWS = [
    ("row stride W - 1", _flow(row=W - 1), "<arg> row stride 6 is below W=7"),
    ("plane stride one below the extent", _flow(plane=EXTENT - 1), "<arg> plane stride 34 is below (H - 1) * row stride + W = 35"),
    ("image stride one below plane + extent", _flow(image=2 * EXTENT - 1),
     "<arg> image stride 69 is below plane stride + (H - 1) * row stride + W = 70"),
    ("a stride of 2^41", _flow(row=1 << 41), "<arg> strides 70, 35, 2199023255552 out of range"),
    ("a pointer off by 2 bytes", _flow(p=5 * P + 2), "misaligned pointer (<arg>)"),
]
BAD_DEPTHS = [
    ("row stride W - 1", _depth(row=W - 1), "<arg> row stride 6 is below W=7"),
    ("image stride one below the extent", _depth(image=EXTENT - 1), "<arg> image stride 34 is below (H - 1) * row stride + W = 35"),
    ("a stride of 2^41", _depth(row=1 << 41), "<arg> strides 35, 2199023255552 out of range"),
    ("a pointer off by 2 bytes", _depth(p=P + 2), "misaligned pointer (<arg>)"),
]
BAD_SHAPES = [
    ("N = 0", dict(N=0), "N=0 images must be in 1 .. 65535"),
    ("N = 65536", dict(N=65536), "N=65536 images must be in 1 .. 65535"),
    ("W = 2^24 + 1", dict(W=(1 << 24) + 1), "H=5, W=16777217 must be in 1 .. 2^24 (pixel coordinates are exact in fp32)"),
]


def _refusals(l, entries, **kw):
    """What every entry says after its own name, with the argument's name taken out; each call must be refused."""
    said = []
    for entry, call, arg in entries:
        assert call(l, **kw) < 0
        message = l.dvs_last_error().decode()
        assert message.startswith(entry + ": "), message
        said.append(re.sub(r"\b%s\b" % arg, "<arg>", message[len(entry) + 2:], count=1))
    return said


@pytest.mark.parametrize("name,view,want", BAD_FLOWS, ids=[b[0] for b in BAD_FLOWS])
def test_every_entry_refuses_the_same_bad_flow_view(lib, name, view, want):
    assert _refusals(lib, FLOW_ENTRIES, flow=view) == [want] * 3


@pytest.mark.parametrize("name,view,want", BAD_DEPTHS, ids=[b[0] for b in BAD_DEPTHS])
def test_every_entry_refuses_the_same_bad_depth_view(lib, name, view, want):
    assert _refusals(lib, DEPTH_ENTRIES, depth=view) == [want] * 2


@pytest.mark.parametrize("name,kw,want", BAD_SHAPES, ids=[b[0] for b in BAD_SHAPES])
def test_every_entry_refuses_the_same_bad_shape(lib, name, kw, want):
    assert _refusals(lib, FLOW_ENTRIES, **kw) == [want] * 3


def test_the_good_views_pass_the_checks(lib):
    """The defaults the cases above vary are themselves accepted: with no output to write, the entries that can return before a
    launch do so with DVS_OK; dvs_pose_fit always launches, so it is shown past every view check by a fault it looks for later."""
    assert lib.dvs_flow_consistency(*_flow(), 2 * P, 2 * EXTENT, EXTENT, W, None, None, None, None, N, H, W, 0.01, 0.5, None) == 0
    assert lib.dvs_rigid_flow(*_depth(), 2 * P, 3 * P, 4 * P, *_flow(), 6 * P, None, None, None, N, H, W, 0.01, 0.5, 1e-7, None) == 0
    args = (*_depth(), 2 * P, 3 * P, 4 * P, *_flow(), 6 * P, 7 * P, 8 * P, 9 * P, 10 * P, 480, N, H, W, -1, 1.0, 1e-6, 1e-7, None)
    assert lib.dvs_pose_fit(*args) < 0 and lib.dvs_last_error() == b"dvs_pose_fit: iters=-1 must be in 0 .. 64"
