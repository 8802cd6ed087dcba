"""Guard-band runs (tests/guard.py) of dvs_pose_fit (csrc/posefit.hip) at ragged shapes: depth, flow, the mask and the three
matrices sit between POISON (NaN) bands -- and, for a strided view, depth and flow inside a frame of NaN, so that an element read
outside the view turns a finite sum into NaN -- and T, status, the sums and the workspace between CANARY bands.  The workspace is
exactly dvs_pose_fit_workspace bytes.  No band byte may change, the judged count is exact and the sums lie within the summation
bound of tests/posefit_ref.py; the vector and the scalar form are both reached."""
import numpy as np
import pytest
import torch

import guard
import posefit_ref as P
import rigidflow_ref as R
from test_guard_rigidflow_gpu import FRAMES, placed

pytestmark = pytest.mark.gpu

SHAPES = [(H, W) for H in (1, 7) for W in (3, 4, 5, 64, 131)]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


@pytest.mark.parametrize("masked", [True, False], ids=["valid", "no_mask"])
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_pose_fit_stays_inside_its_buffers(gpu_device, L, H, W, frame, masked):
    s = P.scene(H, W, noise=0.3, outliers=0.1)
    N = s.N
    valid = R.mask(H, W, N) if masked else None
    T0 = P.start(N)
    g = guard.Bands(gpu_device)
    depth, flow = placed(g, s.depth, FRAMES[frame]), placed(g, s.flow, FRAMES[frame])
    mats = [g.place(torch.from_numpy(np.broadcast_to(m, (N, 4, 4)).copy())) for m in (s.K, s.iK, T0)]
    v = g.place(torch.from_numpy(valid)) if masked else None
    need = L.lib().dvs_pose_fit_workspace(N, H, W)
    assert need % 240 == 0 and need >= 240 * N
    T, status, row = g.empty((N, 4, 4)), g.empty((N,), dtype=torch.int32), g.empty((N, 30), dtype=torch.float64)
    ws = g.empty((need,), dtype=torch.uint8)
    vector = W % 4 == 0 and frame != "view"
    if vector:                                              # what the entry's choice of the vector form rests on
        assert depth.data_ptr() % 16 == 0 and flow.data_ptr() % 16 == 0 and (v is None or v.data_ptr() % 4 == 0)
        assert all(st % 4 == 0 for st in (depth.stride(0), depth.stride(2), flow.stride(0), flow.stride(1), flow.stride(2)))

    def call(iters, T_in):
        L.check(L.lib().dvs_pose_fit(depth.data_ptr(), depth.stride(0), depth.stride(2), mats[0].data_ptr(), mats[1].data_ptr(),
                                     T_in.data_ptr(), flow.data_ptr(), flow.stride(0), flow.stride(1), flow.stride(2),
                                     v.data_ptr() if masked else None, T.data_ptr(), status.data_ptr(), row.data_ptr(), ws.data_ptr(),
                                     need, N, H, W, iters, 0.5, 1e-6, s.eps, L.stream()), "dvs_pose_fit")
        g.check()

    call(0, mats[2])                                        # the sums at T0
    want = P.terms(s.depth, s.flow, s.K, s.iK, T0, valid, 0.5, s.eps)
    got, ref = row.cpu().numpy(), P.normal(want)
    assert np.array_equal(got[:, 29], ref[:, 29]) and (np.abs(got - ref) <= P.sum_bound(want)).all()
    assert np.array_equal(P.bits(T.cpu().numpy()), P.bits(T0)) and not status.any()
    call(2, mats[2])                                        # two steps and the sums at the final T
    got = row.cpu().numpy()
    assert np.isfinite(got).all() and set(status.tolist()) <= {0, 1} and np.isfinite(T.cpu().numpy()).all()
    call(1, T)                                              # in place
