"""Guard bands around one step of SmallRAFT's update block (raft_update.py, csrc/gru.hip and the convolutions under it): the four
inputs and both cotangents sit between POISON bands, and the step runs inside guard.allocations(), so every matrix the gate kernels
write (z, r, r*h, q, h', dpre, dah, dq, dh_a, dh), every convolution output and every gradient buffer sits between CANARY bands.
B = 1 with P = H * W one below, at and one past the pixels a gate workgroup covers (the last a one-row image), and a prime away
from the tile edge (131 = 2.5 workgroups; a prime P at B = 1 is a one-column image).
Values are compared with tests/raft_update_ref.py in fp64 at the one-step tolerances.  See tests/guard.py."""
import pytest
import torch

import guard
import raft_update_ref as R

pytestmark = pytest.mark.gpu
HIDDEN, PLANES = 20, 36
T = -(-1024 // HIDDEN)              # 52 pixels per gate workgroup (test_raft_update_gpu.tile_pixels)
CASES = [("P51_below", 3, 17), ("P52_tile", 4, 13), ("P53_past", 1, 53), ("P131_prime_column", 131, 1)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_update_block_stays_inside_its_buffers(gpu_device, case):
    from deep_visual_slam_amd import conv, raft_update, zeropool
    name, H, W = case
    assert (T - 1, T, T + 1) == (51, 52, 53)
    weights = R.make_weights(HIDDEN, PLANES, seed=H)
    x, cot = R.make_case(HIDDEN, PLANES, 1, H, W, seed=W)
    ref = R.run(weights, x, cot, torch.float64)
    block = raft_update.SmallUpdateBlock(hidden_dim=HIDDEN, corr_levels=4, corr_radius=1)
    block.load_state_dict(weights)
    block = block.to(gpu_device)
    g = guard.Bands(gpu_device)
    d = {k: g.place(v).requires_grad_(True) for k, v in x.items()}
    dn, dd = g.place(cot[0][0]), g.place(cot[0][1])
    with guard.allocations(raft_update, conv, zeropool) as rec:
        net, _, delta = block(d["net"], d["inp"], d["corr"], d["flow"])
        grads = torch.autograd.grad([net, delta], [d[k] for k in R.INPUTS] + list(block.parameters()), [dn, dd])
        torch.cuda.synchronize()
    # the gate kernels' ten matrices, and at least the outputs of the ten convolutions
    assert rec.count >= 20, rec.count
    g.check()
    got = {"net0": net, "delta0": delta}
    got.update({"d/" + n: v for n, v in zip(list(R.INPUTS) + [k for k, _ in block.named_parameters()], grads)})
    assert sorted(got) == sorted(ref)
    for k in sorted(ref):
        R.check_rel(name + " " + k, got[k], ref[k])
