"""Guard-band runs (tests/guard.py) of dvs_rigid_flow (csrc/rigidflow.hip) at ragged shapes: depth, flow, the mask and the three
matrices sit between POISON (NaN) bands -- and, for a strided view, depth and flow inside a frame of NaN, so that an element read
outside the view turns a finite result into NaN -- and the three outputs between CANARY bands.  No band byte may change, and the
values are exact (tests/test_rigidflow_gpu.py states why)."""
import numpy as np
import pytest
import torch

import guard
import rigidflow_ref as R

pytestmark = pytest.mark.gpu

# dense; a window at odd offsets of a wider frame (scalar form); a window at offsets of 4 (the vector form where W % 4 == 0)
FRAMES = {"dense": None, "view": (2, 3, 1, 2), "view4": (1, 4, 4, 4)}      # rows above, below, columns left, right
SHAPES = [(H, W) for H in (1, 7) for W in (3, 4, 5, 64, 131)]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


def placed(g, t, frame):
    """The view the kernel reads of `t` [N,C,H,W] in guarded memory: dense, or a window of a NaN frame."""
    N, C, H, W = t.shape
    if frame is None:
        return g.place(torch.from_numpy(t))
    above, below, left, right = frame
    full = torch.full((N, C, above + H + below, left + W + right), float("nan"))
    full[:, :, above:above + H, left:left + W] = torch.from_numpy(t)
    return g.place(full)[:, :, above:above + H, left:left + W]


@pytest.mark.parametrize("with_flow", [True, False], ids=["flow", "rigid_only"])
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_rigid_flow_stays_inside_its_buffers(gpu_device, L, H, W, frame, with_flow):
    s = R.scene(H, W)
    N = s.N
    flow, valid = (R.measured(s), R.mask(H, W, N)) if with_flow else (None, None)
    want = R.rigid(s.depth, s.T, s.K, s.iK, flow, valid, eps=s.eps)
    g = guard.Bands(gpu_device)
    depth = placed(g, s.depth, FRAMES[frame])
    mats = [g.place(torch.from_numpy(np.broadcast_to(m, (N, 4, 4)).copy())) for m in (s.K, s.iK, s.T)]
    rigid = g.empty((N, 2, H, W))
    vector = W % 4 == 0 and frame != "view"
    ptr = lambda t: t.data_ptr() if t is not None else None
    f = v = excess = label = None
    f_strides = (0, 0, 0)
    if with_flow:
        f = placed(g, flow, FRAMES[frame])
        f_strides = (f.stride(0), f.stride(1), f.stride(2))
        v = g.place(torch.from_numpy(valid))
        excess, label = g.empty((N, H, W)), g.empty((N, H, W), dtype=torch.uint8)
    if vector:                                              # what the entry's choice of the vector form rests on
        assert all(t.data_ptr() % 16 == 0 for t in (depth, rigid) + ((f, v, excess, label) if with_flow else ()))
        assert depth.stride(0) % 4 == 0 and depth.stride(2) % 4 == 0 and all(st % 4 == 0 for st in f_strides)
    L.check(L.lib().dvs_rigid_flow(depth.data_ptr(), depth.stride(0), depth.stride(2), mats[0].data_ptr(), mats[1].data_ptr(),
                                   mats[2].data_ptr(), ptr(f), *f_strides, ptr(v), rigid.data_ptr(), ptr(excess), ptr(label), N, H, W,
                                   R.ALPHA, R.BETA, s.eps, L.stream()), "dvs_rigid_flow")
    g.check()
    assert np.array_equal(R.bits(rigid.cpu().numpy()), R.bits(want.rigid))
    if with_flow:
        assert np.array_equal(label.cpu().numpy(), want.label)
        assert np.array_equal(R.bits(excess.cpu().numpy()), R.bits(want.excess))
