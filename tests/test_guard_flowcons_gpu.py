"""Guard-band runs (tests/guard.py) of dvs_flow_consistency (csrc/flowcons.hip) at ragged shapes: both flows sit between POISON (NaN)
bands -- and, for a strided view, inside a frame of NaN, so that a tap read outside the view turns a finite excess into +inf -- and
the four outputs between CANARY bands.  No band byte may change, and the values are exact (tests/test_flowcons_gpu.py states why)."""
import numpy as np
import pytest
import torch

import flowcons_ref as R
import guard

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


def placed(g, flow, frame):
    """(the view the kernel reads, its image / plane / row strides) of `flow` [N,2,H,W] in guarded memory."""
    N, _, H, W = flow.shape
    if frame is None:
        v = g.place(torch.from_numpy(flow))
        return v, 2 * H * W, H * W, W
    above, below, left, right = frame
    full = torch.full((N, 2, above + H + below, left + W + right), float("nan"))
    full[:, :, above:above + H, left:left + W] = torch.from_numpy(flow)
    v = g.place(full)[:, :, above:above + H, left:left + W]
    return v, v.stride(0), v.stride(1), v.stride(2)


@pytest.mark.parametrize("scale", [0.7, 3.0])
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_consistency_stays_inside_its_buffers(gpu_device, L, H, W, frame, scale):
    a, b = R.noise(H, W, scale)
    N = a.shape[0]
    want = R.consistency(a, b)
    g = guard.Bands(gpu_device)
    va, a_image, a_plane, a_row = placed(g, a, FRAMES[frame])
    vb, b_image, b_plane, b_row = placed(g, b, FRAMES["dense" if frame == "view4" else frame])      # view4: the partner is dense
    valid = [g.empty((N, H, W), dtype=torch.uint8) for _ in range(2)]
    excess = [g.empty((N, H, W)) for _ in range(2)]
    vector = W % 4 == 0 and frame != "view"
    if vector:                                              # what the entry's choice of the vector form rests on
        assert all(t.data_ptr() % 16 == 0 for t in (va, vb, *valid, *excess)) and a_row % 4 == 0 and a_plane % 4 == 0 and a_image % 4 == 0
    L.check(L.lib().dvs_flow_consistency(va.data_ptr(), a_image, a_plane, a_row, vb.data_ptr(), b_image, b_plane, b_row,
                                         valid[0].data_ptr(), valid[1].data_ptr(), excess[0].data_ptr(), excess[1].data_ptr(),
                                         N, H, W, R.ALPHA, R.BETA, L.stream()), "dvs_flow_consistency")
    g.check()
    for i in range(2):
        assert np.array_equal(valid[i].cpu().numpy(), want[i].valid)
        assert np.array_equal(R.bits(excess[i].cpu().numpy()), R.bits(want[i].excess))
