"""Guard-band runs (tests/guard.py) of the instance-norm and upflow8 entries at the ragged cases of tests/test_raft_gpu.py, and of
one SmallRAFT forward + backward whose every own allocation sits between CANARY bands.  Inputs are placed between POISON (NaN)
bands: a read outside them that reaches arithmetic turns an output NaN; every output buffer sits between CANARY bands."""
import pytest
import torch

import guard
import raft_ref as R
from test_raft_gpu import FLAGS, T, inorm_forward_refs, inorm_operands, make_raft

pytestmark = pytest.mark.gpu
CL = torch.channels_last

INORM_CASES = [(Cn, N, HW, f) for Cn in (24, 96) for N in (1, 3) for HW in (2, T - 1, T + 1, 2 * T + 77) for f in FLAGS]


@pytest.mark.parametrize("Cn,N,HW,flags", INORM_CASES, ids=["c%d_n%d_hw%d_%s" % c for c in INORM_CASES])
def test_inorm_entries_stay_inside_their_buffers(gpu_device, Cn, N, HW, flags):
    from deep_visual_slam_amd import _lib
    lib = _lib.lib()
    norm, relu, residual = FLAGS[flags]
    y, res, dout = inorm_operands(N, HW, Cn, residual, seed=Cn + HW + N)
    g = guard.Bands(gpu_device)
    yd, gd = g.place(y), g.place(dout)
    rd = g.place(res) if residual else None
    out, dy = g.empty((N, HW, Cn)), g.empty((N, HW, Cn))
    dres = g.empty((N, HW, Cn)) if residual else None
    table = g.empty((N, 2, Cn)) if norm else None
    nbytes = int(lib.dvs_inorm_workspace(N, HW, Cn))
    ws = g.empty((nbytes // 4,)) if norm else None
    p = lambda t: t.data_ptr() if t is not None else None
    _lib.check(lib.dvs_inorm_fwd(p(yd), p(rd), p(out), p(table), p(ws), nbytes if norm else 0, N, HW, Cn, norm, relu, _lib.stream()),
               "dvs_inorm_fwd")
    _lib.check(lib.dvs_inorm_bwd(p(gd), p(yd), p(out) if residual else None, p(table), p(dy), p(dres), p(ws), nbytes if norm else 0,
                                 N, HW, Cn, norm, relu, _lib.stream()), "dvs_inorm_bwd")
    g.check()
    for t in (out, dy, dres, table):
        assert t is None or torch.isfinite(t).all()
    r64, r32 = inorm_forward_refs(y, res, norm, relu)["out"]
    assert float((out.cpu().double() - r64).abs().max()) <= R.bound(r64, r32)


UP_CASES = [(h, w, N, nchw) for (h, w) in ((1, 1), (1, 5), (5, 7), (16, 17)) for N in (1, 3) for nchw in (1, 0)]


@pytest.mark.parametrize("h,w,N,nchw", UP_CASES, ids=["%dx%d_n%d_%s" % (h, w, N, "nchw" if p else "nhwc") for h, w, N, p in UP_CASES])
def test_upflow8_entries_stay_inside_their_buffers(gpu_device, h, w, N, nchw):
    from deep_visual_slam_amd import _lib
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(h * 100 + w)
    flow, dout = torch.randn(N, 2, h, w, generator=gen), torch.randn(N, 2, 8 * h, 8 * w, generator=gen)
    g = guard.Bands(gpu_device)
    fd = g.place(flow if nchw else flow.permute(0, 2, 3, 1).contiguous())
    gd = g.place(dout)
    up = g.empty((N, 2, 8 * h, 8 * w))
    dflow = g.empty((N, 2, h, w) if nchw else (N, h, w, 2))
    _lib.check(lib.dvs_upflow8_fwd(fd.data_ptr(), up.data_ptr(), N, h, w, nchw, _lib.stream()), "dvs_upflow8_fwd")
    _lib.check(lib.dvs_upflow8_bwd(gd.data_ptr(), dflow.data_ptr(), N, h, w, nchw, _lib.stream()), "dvs_upflow8_bwd")
    g.check()
    f64 = flow.double().requires_grad_(True)
    u64 = R.upflow8(f64)
    (g64,) = torch.autograd.grad(u64, f64, dout.double())
    u32 = R.upflow8(flow)
    assert torch.isfinite(up).all() and torch.isfinite(dflow).all()
    assert float((up.cpu().double() - u64.detach()).abs().max()) <= R.bound(u64.detach(), u32)
    have = dflow.cpu() if nchw else dflow.cpu().permute(0, 3, 1, 2)
    assert float((have.double() - g64).abs().max()) <= 1e-4 * float(g64.abs().max())


def test_small_raft_under_guarded_allocations(gpu_device):
    """One forward + backward at 128x136, iters=2: what raft, raft_encoder, raft_update, raft_corr and conv allocate is guarded."""
    from deep_visual_slam_amd import conv, raft, raft_corr, raft_encoder, raft_update, zeropool
    w, im1, im2, cot, _ = R.g6_case("noinit")
    model = make_raft(w, gpu_device, False)
    g = guard.Bands(gpu_device)
    a, b = g.place(im1), g.place(im2)
    with guard.allocations(raft, raft_encoder, raft_update, raft_corr, conv, zeropool) as rec:
        flows = model(a, b, iters=2)
        loss = sum((f * c.to(gpu_device)).sum() for f, c in zip(flows, cot))
        grads = torch.autograd.grad(loss, list(model.parameters()))
        torch.cuda.synchronize()
    g.check()
    assert rec.count >= 100, rec.count
    assert all(torch.isfinite(f).all() for f in flows) and all(torch.isfinite(t).all() for t in grads)
