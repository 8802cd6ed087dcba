"""Guard gaps in the two packed layouts a training step really uses: the step's scratch pool (zeropool) and the
parameter / gradient arena (dp.FlatParams).  Both pack tensors back to back, so a kernel that writes one element
past its tensor corrupts its neighbour; here the neighbours are moved apart by a zero-filled gap and every gap
must still be all-zero bytes after a full forward + backward (+ optimiser) step."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GAP = 1024                  # floats between two pool hand-outs (4 KiB)
ALIGN = 4124                # 4 * 1031 (prime): no layer's element count is a multiple, every arena slot ends in a gap


def _cfg(B, H, W):
    return {"Train": dict(num_source=1, batch_size=B, img_h=H, img_w=W, smoothness_ratio=0.001, auto_mask=True,
                          ssim_ratio=0.85, min_depth=0.1, max_depth=10.0, use_compile=False)}


def _inputs(dev, B, H, W):
    from deep_visual_slam_amd import synth
    sample = {k: v.to(dev) for k, v in synth.parity_sample(B, H, W).items()}
    g = torch.Generator().manual_seed(11)
    noise = torch.stack([torch.randn(B, 2, H, W, generator=g) for _ in range(4)]).to(dev)
    return sample, noise


def _nets(dev):
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.posenet_single import PoseNet
    torch.manual_seed(5)
    return (DepthNet(18, pretrained=False).to(dev).train(),
            PoseNet(18, pretrained=False, num_input_images=2).to(dev).train())


def _dirty(flat_f32, lo, hi):
    """(changed 4-byte words, index of the first) of flat_f32[lo:hi], compared as raw bits with zero."""
    bits = flat_f32[lo:hi].view(torch.int32) != 0
    n = int(bits.sum())
    return n, (int(bits.nonzero()[0]) + lo if n else -1)


@pytest.mark.parametrize("H,W", [(96, 128), (480, 640)])
def test_scratch_pool_neighbours_are_not_touched(gpu_device, H, W):
    from deep_visual_slam_amd import gradsink, zeropool
    from deep_visual_slam_amd.learner_new import MonodepthTrainer
    B = 2
    sample, noise = _inputs(gpu_device, B, H, W)
    dn, pn = _nets(gpu_device)
    tr = MonodepthTrainer(dn, pn, _cfg(B, H, W), gpu_device)
    pool, orig = zeropool._pool, zeropool.zeros
    handed, gaps = [], []                   # (first float, floats, shape) of each hand-out; (first, end) of the gap behind it

    def spaced_zeros(shape, device, channels_last=False, pooled=True):
        before = pool.off
        t = orig(shape, device, channels_last=channels_last, pooled=pooled)
        if pool.off != before:              # served from the pool: leave a gap from its exact last float on
            handed.append((before, t.numel(), tuple(shape)))
            pool.off += GAP
            gaps.append((before + t.numel(), pool.off))
        return t

    zeropool.zeros = spaced_zeros
    try:
        tr._noise = noise
        _, losses = tr.process_batch(dict(sample))
        losses["loss"].backward()
        gradsink.join()
        torch.cuda.synchronize()
    finally:
        zeropool.zeros = orig
    assert torch.isfinite(losses["loss"].detach()).all()
    assert len(handed) >= 50, len(handed)                  # the step's BatchNorm statistics, slot tables, split-K scratch
    assert len(gaps) >= len(handed) - 1 and pool.off < pool.buf.numel()
    assert all(e - s >= GAP for s, e in gaps)
    bad = []
    for (s, e), (first, n, shape) in zip(gaps, handed):
        cnt, at = _dirty(pool.buf, s, e)
        if cnt:
            bad.append("hand-out %s at float %d: %d words changed behind it, first %d floats past its end" % (shape, first, cnt, at - (first + n)))
    assert not bad, "\n".join(bad[:10])
    cnt, at = _dirty(pool.buf, pool.off, pool.buf.numel())
    assert cnt == 0, "pool written beyond the handed-out prefix at float %d" % at
    print("scratch pool %dx%d: %d hand-outs, %d gaps clean" % (H, W, len(handed), len(gaps)))


def _step(dev, align, sample, noise, B, H, W):
    from deep_visual_slam_amd import dp, gradsink
    from deep_visual_slam_amd.learner_new import MonodepthTrainer
    dn, pn = _nets(dev)
    flat = dp.FlatParams(dp.trainable_parameters(dn, pn), align=align, grad_sinks=True)
    opt = dp.FusedAdam(flat, lr=1e-4)
    tr = MonodepthTrainer(dn, pn, _cfg(B, H, W), dev)
    assert tr.arena is None                                # the trainer uses the caller's arena
    tr._noise = noise
    _, losses = tr.process_batch(dict(sample))
    losses["loss"].backward()
    gradsink.join()
    torch.cuda.synchronize()
    return flat, opt, float(losses["loss"].detach())


def _arena_gaps(flat):
    ends = flat.offsets[1:] + [flat.numel]
    return [(o + p.numel(), e) for o, p, e in zip(flat.offsets, flat.tensors, ends)]


def test_arena_slots_do_not_leak_into_their_neighbours(gpu_device):
    from deep_visual_slam_amd import _lib
    B, H, W = 2, 96, 128
    sample, noise = _inputs(gpu_device, B, H, W)
    _lib.set_deterministic(True)           # same ReLU / max-pool branches in both runs: what is left is the atomics' rounding noise
    try:
        ref_flat, _, ref_loss = _step(gpu_device, 4, sample, noise, B, H, W)
        ref_grads = [ref_flat.grads[o:o + p.numel()].double().clone() for o, p in zip(ref_flat.offsets, ref_flat.tensors)]
        flat, opt, loss = _step(gpu_device, ALIGN, sample, noise, B, H, W)
    finally:
        _lib.set_deterministic(False)
    gaps = _arena_gaps(flat)
    assert len(gaps) == len(flat.offsets) and all(e > s for s, e in gaps)
    assert all(o % 4 == 0 for o in flat.offsets)           # slots keep the 16-byte alignment of the C ABI

    def clean(arena, what):
        bad = []
        for (s, e), n, o in zip(gaps, flat.names, flat.offsets):
            cnt, at = _dirty(arena, s, e)
            if cnt:
                bad.append("%s: %d words changed behind slot %s (%d floats), first %d floats past its end" % (what, cnt, n, s - o, at - s))
        assert not bad, "\n".join(bad[:10])

    clean(flat.grads, "grads after backward")
    clean(flat.params, "params after backward")
    assert abs(loss - ref_loss) <= 2e-5 * abs(ref_loss), (loss, ref_loss)
    assert flat.names == ref_flat.names
    for n, p, o, r in zip(flat.names, flat.tensors, flat.offsets, ref_grads):
        g = flat.grads[o:o + p.numel()].double()
        assert torch.isfinite(g).all(), n
        err = float((g - r).norm()) / (float(r.norm()) + 1e-30)
        assert err <= 2e-5, (n, err, float(r.norm()))
    before = flat.params.clone()
    opt.step(zero_grad=False)
    torch.cuda.synchronize()
    clean(flat.params, "params after the optimiser step")
    clean(flat.grads, "grads after the optimiser step")
    clean(opt.exp_avg, "exp_avg")
    clean(opt.exp_avg_sq, "exp_avg_sq")
    for n, p, o in zip(flat.names, flat.tensors, flat.offsets):
        assert torch.isfinite(flat.params[o:o + p.numel()]).all(), n
    assert float((flat.params - before).abs().max()) > 0.0
    print("arena: %d slots, %d gaps clean, loss %.8f vs %.8f" % (len(flat.offsets), len(gaps), loss, ref_loss))
