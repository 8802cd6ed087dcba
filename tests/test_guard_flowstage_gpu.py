"""Guard-band runs (tests/guard.py) of the three entries of csrc/flowstage.hip at the ragged shapes of tests/test_flowstage_gpu.py.
Inputs sit between POISON (NaN) bands -- and, for a strided view, inside a frame of NaN: a read outside them turns radmax NaN or
changes a byte -- and every output between CANARY bands."""
import numpy as np
import pytest
import torch

import flowstage_ref as R
import guard
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec():
    return load_golden("flowstage.npz")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("h,w", R.FI_SHAPES, ids=["%dx%d" % s for s in R.FI_SHAPES])
def test_forward_interp_stays_inside_its_buffers(gpu_device, rec, L, h, w, N):
    k = R.fi_key(h, w)
    g = guard.Bands(gpu_device)
    flow = g.place(torch.from_numpy(rec[k + "/flow"][:N]))
    out = g.empty((N, 2, h, w))
    L.check(L.lib().dvs_forward_interp(flow.data_ptr(), out.data_ptr(), N, h, w, L.stream()), "dvs_forward_interp")
    g.check()
    assert torch.equal(out.cpu(), torch.from_numpy(rec[k + "/out"][:N]))


def run_colouring(L, g, flow, view, clip, bgr):
    """(radmax, image) of `view` [N,2,H,W] (a window of the guarded `flow`, or `flow` itself), outputs guarded."""
    N, _, H, W = view.shape
    radmax, image = g.empty((N,)), g.empty((N, H, W, 3), dtype=torch.uint8)
    plane, row = view.stride(1), (view.stride(2) if H > 1 else max(W, 1))
    if N > 1:
        assert view.stride(0) == 2 * plane
    c = -1.0 if clip is None else clip
    L.check(L.lib().dvs_flow_radmax(view.data_ptr(), plane, row, N, H, W, c, radmax.data_ptr(), L.stream()), "dvs_flow_radmax")
    L.check(L.lib().dvs_flow_to_image(view.data_ptr(), plane, row, radmax.data_ptr(), image.data_ptr(), N, H, W, c, int(bgr),
                                      L.stream()), "dvs_flow_to_image")
    g.check()
    return radmax, image


def check_colouring(flows, clip, bgr, radmax, image, fixture):
    want = np.array([R.flow_radius(f, clip)[2] for f in flows])
    assert np.array_equal(radmax.cpu().numpy().view(np.int32), want.view(np.int32))
    diff = np.abs(image.cpu().numpy().astype(np.int32) - fixture.astype(np.int32))
    assert diff.max() <= 1 and (diff > 0).mean() <= R.MAX_EXEMPT          # the byte rule itself: tests/test_flowstage_gpu.py


FV_CASES = [(H, W, N) for H, W in R.FV_SIZES for N in (1, 3)] + [R.FV_BIG + (1,)]      # 131x77 is a single image


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "view"])
@pytest.mark.parametrize("H,W,N", FV_CASES, ids=["%dx%d_n%d" % c for c in FV_CASES])
def test_colouring_stays_inside_its_buffers(gpu_device, rec, L, H, W, N, strided):
    if (H, W) == R.FV_BIG:
        flows, fixture = rec["fv/big/large"][None], rec["fv/big/large_image"][None]
    else:
        flows, fixture = rec[R.fv_key(H, W) + "/flow"][:N], rec[R.fv_key(H, W) + "/image"][:N]
    g = guard.Bands(gpu_device)
    if strided:
        frame = torch.full((N, 2, H + 5, W + 3), float("nan"))
        frame[:, :, 2:2 + H, 1:1 + W] = torch.from_numpy(flows)
        placed = g.place(frame)
        view = placed[:, :, 2:2 + H, 1:1 + W]
    else:
        placed = view = g.place(torch.from_numpy(flows))
    radmax, image = run_colouring(L, g, placed, view, None, False)
    check_colouring(flows, None, False, radmax, image, fixture)


@pytest.mark.parametrize("name", R.FV_SPECIAL_NAMES)
def test_colouring_special_cases_stay_inside_their_buffers(gpu_device, rec, L, name):
    flow, clip, bgr = R.fv_special(name)
    g = guard.Bands(gpu_device)
    placed = g.place(torch.from_numpy(flow[None]))
    radmax, image = run_colouring(L, g, placed, placed, clip, bgr)
    check_colouring(flow[None], clip, bgr, radmax, image, rec["fv/%s/image" % name][None])
