"""Guard-band runs (tests/guard.py) of the pooling-head entries at the ragged cases of tests/test_flowpose_gpu.py, and of one
FlowPoseNet forward + backward whose own allocations sit between CANARY bands.  Inputs are placed between POISON (NaN) bands: a
read outside them that reaches arithmetic turns an output NaN; every output buffer and the workspace sit between CANARY bands."""
import pytest
import torch

import flowpose_ref as P
import guard
import raft_ref as R
from test_flowpose_gpu import T, make_net, pool_fc_operands, pool_fc_refs

pytestmark = pytest.mark.gpu

POOL_CASES = [(Cn, J, N, Pn, relu) for Cn in (4, 24, 128) for J in (1, 6) for N in (1, 3) for Pn in (1, T - 1, T, T + 1, 2 * T + 5)
              for relu in (0, 1)]


@pytest.mark.parametrize("Cn,J,N,Pn,relu", POOL_CASES, ids=["c%d_j%d_n%d_p%d_relu%d" % c for c in POOL_CASES])
def test_pool_fc_entries_stay_inside_their_buffers(gpu_device, Cn, J, N, Pn, relu):
    from deep_visual_slam_amd import _lib
    lib = _lib.lib()
    y, W, b, dout = pool_fc_operands(N, Pn, Cn, J, seed=Cn + Pn + N + J)
    g = guard.Bands(gpu_device)
    yd, Wd, bd, gd = g.place(y), g.place(W), g.place(b), g.place(dout)
    out, mean, dy, dW, db = g.empty((N, J)), g.empty((N, Cn)), g.empty((N, Pn, Cn)), g.empty((J, Cn)), g.empty((J,))
    nbytes = int(lib.dvs_pool_fc_workspace(N, Pn, Cn))
    ws = g.empty((nbytes // 4,))
    p = lambda t: t.data_ptr()
    _lib.check(lib.dvs_pool_fc_fwd(p(yd), p(Wd), p(bd), p(out), p(mean), p(ws), nbytes, N, Pn, Cn, J, relu, P.POSE_SCALE, _lib.stream()),
               "dvs_pool_fc_fwd")
    _lib.check(lib.dvs_pool_fc_bwd(p(gd), p(yd), p(mean), p(Wd), p(dy), p(dW), p(db), N, Pn, Cn, J, relu, P.POSE_SCALE, _lib.stream()),
               "dvs_pool_fc_bwd")
    g.check()
    refs = pool_fc_refs(y, W, b, dout, relu, P.POSE_SCALE)
    for name, t in (("out", out), ("mean", mean), ("d/y", dy), ("d/W", dW), ("d/b", db)):
        assert torch.isfinite(t).all(), name
        R.U.check_rel(name, t, refs[name][0], extra=R.bound(*refs[name]))


def test_flowposenet_under_guarded_allocations(gpu_device):
    """One forward + backward at 128x136, iters=2: what posenet_single allocates (the head's outputs, workspace and gradients) is
    guarded; the images sit between POISON bands."""
    from deep_visual_slam_amd import posenet_single
    w, images, cot = P.g4_case()
    model = make_net(w, gpu_device, iters=2)
    g = guard.Bands(gpu_device)
    x = g.place(images)
    with guard.allocations(posenet_single) as rec:
        aa, t = model(x)
        loss = (aa * cot[0].to(gpu_device)).sum() + (t * cot[1].to(gpu_device)).sum()
        grads = torch.autograd.grad(loss, list(model.parameters()))
        torch.cuda.synchronize()
    g.check()
    assert rec.count >= 6, rec.count
    assert torch.isfinite(aa).all() and torch.isfinite(t).all() and all(torch.isfinite(v).all() for v in grads)
