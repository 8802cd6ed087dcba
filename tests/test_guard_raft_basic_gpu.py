"""Guard-band runs (tests/guard.py) of the convex-upsampling and shift-stack entries at the ragged cases of
tests/test_raft_basic_gpu.py, and of one RAFT forward + backward whose every own allocation sits between CANARY bands.  Inputs are
placed between POISON (NaN) bands: a read outside them that reaches arithmetic turns an output NaN; every output buffer sits
between CANARY bands."""
import numpy as np
import pytest
import torch

import guard
import raft_basic_ref as R
from test_raft_basic_gpu import STACK_SHAPES, make_raft

pytestmark = pytest.mark.gpu
CL = torch.channels_last
EPS = float(np.finfo(np.float32).eps)

CONVEX = [(h, w, N) for (h, w) in R.CONVEX_SHAPES for N in (1, 3)]


@pytest.mark.parametrize("h,w,N", CONVEX, ids=["%dx%d_n%d" % c for c in CONVEX])
def test_convex_up_entries_stay_inside_their_buffers(gpu_device, h, w, N):
    from deep_visual_slam_amd import _lib
    lib = _lib.lib()
    flow, mask, cot = R.convex_case(N, h, w, R.convex_seed(h, w, N))
    g = guard.Bands(gpu_device)
    fd, md, gd = g.place(flow), g.place(mask.permute(0, 2, 3, 1).contiguous()), g.place(cot)
    out, dflow, dmask = g.empty((N, 2, 8 * h, 8 * w)), g.empty((N, 2, h, w)), g.empty((N, h, w, 576))
    nbytes = int(lib.dvs_convex_up_workspace(N, h, w))
    assert nbytes == N * h * w * 18 * 4
    ws = g.empty((nbytes // 4,))
    _lib.check(lib.dvs_convex_up_fwd(fd.data_ptr(), md.data_ptr(), out.data_ptr(), N, h, w, 0.25, _lib.stream()), "dvs_convex_up_fwd")
    _lib.check(lib.dvs_convex_up_bwd(gd.data_ptr(), fd.data_ptr(), md.data_ptr(), dflow.data_ptr(), dmask.data_ptr(), ws.data_ptr(),
                                     nbytes, N, h, w, 0.25, _lib.stream()), "dvs_convex_up_bwd")
    g.check()
    assert all(torch.isfinite(t).all() for t in (out, dflow, dmask, ws))
    o64, df64, dm64 = R.run_convex(flow, mask, cot, 0.25, torch.float64)
    assert float((out.cpu().double() - o64).abs().max()) <= 32 * EPS * 8 * float(flow.abs().max())
    assert float((dflow.cpu().double() - df64).abs().max()) <= R.GRAD_TOL * float(df64.abs().max())
    assert float((dmask.cpu().permute(0, 3, 1, 2).double() - dm64).abs().max()) <= R.GRAD_TOL * float(dm64.abs().max())


@pytest.mark.parametrize("H,W", STACK_SHAPES, ids=["%dx%d" % s for s in STACK_SHAPES])
@pytest.mark.parametrize("axis", [0, 1])
def test_shift_stack_entries_stay_inside_their_buffers(gpu_device, axis, H, W):
    from deep_visual_slam_amd import _lib
    lib = _lib.lib()
    for Cn in (4, 128):
        for N in (1, 3):
            gen = torch.Generator().manual_seed(100 * H + 10 * W + Cn + N)
            x, dy = torch.randn(N, H, W, Cn, generator=gen), torch.randn(N, H, W, 5 * Cn, generator=gen)
            g = guard.Bands(gpu_device)
            xd, gd = g.place(x), g.place(dy)
            x5, dx = g.empty((N, H, W, 5 * Cn)), g.empty((N, H, W, Cn))
            _lib.check(lib.dvs_shift_stack_fwd(xd.data_ptr(), x5.data_ptr(), N, H, W, Cn, axis, _lib.stream()), "dvs_shift_stack_fwd")
            _lib.check(lib.dvs_shift_stack_bwd(gd.data_ptr(), dx.data_ptr(), N, H, W, Cn, axis, _lib.stream()), "dvs_shift_stack_bwd")
            g.check()
            assert torch.isfinite(x5).all() and torch.isfinite(dx).all()
            assert torch.equal(x5.cpu().permute(0, 3, 1, 2), R.shift_stack(x.permute(0, 3, 1, 2), axis))


def test_raft_under_guarded_allocations(gpu_device):
    """One forward + backward at 128x136, iters=2, BatchNorm in train mode: what raft, raft_encoder, raft_update, raft_corr, bn and
    conv allocate is guarded."""
    from deep_visual_slam_amd import bn, conv, raft, raft_corr, raft_encoder, raft_update, zeropool
    w, im1, im2, cot, _ = R.g6_case("noinit")
    model = make_raft(w, gpu_device, False, True)
    g = guard.Bands(gpu_device)
    a, b = g.place(im1), g.place(im2)
    with guard.allocations(raft, raft_encoder, raft_update, raft_corr, bn, conv, zeropool) as rec:
        flows = model(a, b, iters=2)
        loss = sum((f * c.to(gpu_device)).sum() for f, c in zip(flows, cot))
        grads = torch.autograd.grad(loss, list(model.parameters()))
        torch.cuda.synchronize()
    g.check()
    assert rec.count >= 100, rec.count
    assert all(torch.isfinite(f).all() for f in flows) and all(torch.isfinite(t).all() for t in grads)
