"""Guard bands around every tensor of the five on-the-fly correlation entry points (dvs_altcorr_* of csrc/corr.hip): feature
maps, coordinates and the cotangents sit between POISON bands, and the calls run inside guard.allocations(), so the workspace,
the pooled rows, the lookup outputs and every gradient buffer sit between CANARY bands (the canary, unlike a NaN, changes under
an atomic add: dfmap2 and the pooled rows' gradient are added into atomically).  The coordinates reach r + 3 beyond the map and
no further: a window that forgot a bounds check reads inside the bands (NaN in the output), not beyond them.  Values are compared
with tests/corr_ref.py in fp64 at the bound of test_altcorr_gpu.py.  See tests/guard.py."""
import pytest
import torch

import guard
from corr_ref import check, make_case, reference

pytestmark = pytest.mark.gpu
CL = torch.channels_last

CASES = [
    # name, B, C, H, W, levels, radius, channels_last inputs, channels_last output and cotangent
    ("17x23_nchw", 2, 24, 17, 23, 4, 3, False, False),
    ("17x23_cl", 2, 24, 17, 23, 4, 3, True, True),
    ("33x31_nchw_in_cl_out", 2, 36, 33, 31, 4, 4, False, True),
    ("33x31_cl_in_nchw_out", 2, 36, 33, 31, 4, 4, True, False),
    ("5x13_one_past_the_tile", 1, 36, 5, 13, 2, 2, False, False),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_altcorr_entry_points_stay_inside_their_buffers(gpu_device, case):
    from deep_visual_slam_amd import raft_corr
    name, B, Cn, H, W, L, r, cl_in, cl_out = case
    f1, f2, coords, douts = make_case(B, Cn, H, W, L, r, n_lookups=2, seed=11, sigma=3.0)
    for c in coords:                                        # r + 3 beyond the map on every side, and no further
        c[:, 0].clamp_(-(r + 3.0), W - 1 + r + 3.0)
        c[:, 1].clamp_(-(r + 3.0), H - 1 + r + 3.0)
        c[0, :, 2, 0:2] = torch.tensor([[-(r + 3.0), W - 1 + r + 3.0], [-(r + 3.0), H - 1 + r + 3.0]])
    ref = reference(f1, f2, coords, douts, L, r)
    g = guard.Bands(gpu_device)
    fmt = lambda t, cl: t.contiguous(memory_format=CL) if cl else t.contiguous()
    g1 = g.place(fmt(f1, cl_in)).requires_grad_(True)
    g2 = g.place(fmt(f2, cl_in)).requires_grad_(True)
    gc = [g.place(c) for c in coords]
    gd = [g.place(fmt(d, cl_out)) for d in douts]
    with guard.allocations(raft_corr) as rec:
        block = raft_corr.AlternateCorrBlock(g1, g2, num_levels=L, radius=r)
        outs = [block(c, memory_format=CL if cl_out else None) for c in gc]
        d1, d2 = torch.autograd.grad(outs, [g1, g2], gd)
        torch.cuda.synchronize()
    # workspace, pooled rows, 2 outputs, per lookup backward (dfmap1, dfmap2, pooled rows' gradient), the unpooled dfmap2
    assert rec.count >= 11, rec.count
    g.check()
    (o64, a64, b64), (o32, a32, b32) = ref[torch.float64], ref[torch.float32]
    for k in range(2):
        check("%s lookup %d" % (name, k), outs[k], o64[k], o32[k])
    check(name + " dfmap1", d1, a64, a32)
    check(name + " dfmap2", d2, b64, b32)
