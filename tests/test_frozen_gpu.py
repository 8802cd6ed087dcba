"""Frozen-parameter training steps at the level a user sees: DepthNet / PoseNet with part of the parameters not requiring a
gradient (frozen encoder, frozen decoder, frozen BatchNorm affine parameters and biases, BatchNorm-only fine-tuning).

Freezing changes ctx.needs_input_grad of every convolution and with it the backward kernels (tests/test_conv_sequences_gpu.py
checks those one layer at a time); here whole networks run at 96 x 128, batch 2, training-mode BatchNorm, with a random
cotangent on the four disparities (DepthNet) or on (axis-angle, translation) (PoseNet).  The yardstick is
test_posenet_pairs_in_one_pass_equal_two_calls': the oracle network (oracle.networks) runs once in fp64 and once in fp32 on the
CPU, and every trainable parameter's gradient must be within 3 x (worst fp32-oracle rel-L2 error against fp64) + 2 x flip of
the fp64 one, flip = 1 / sqrt(elements of the smallest ReLU map): one ReLU branch flipped by rounding.  Frozen parameters must
end with .grad None, and the BatchNorm running statistics must move exactly as in the all-trainable control (same forward).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
B, H, W = 2, 96, 128


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _is_bn_affine(name, p):
    return p.dim() == 1 and "encoder." in name          # the encoders' convolutions have no bias: every vector there is BatchNorm's


def _frozen(scenario, name, p):
    if ".fc." in name:
        return False                                    # torchvision's unused head: never runs, left as it is
    return {"encoder": name.startswith("encoder."),
            "decoder": not name.startswith("encoder."),
            "bn_and_bias": p.dim() == 1,
            "only_bn": not _is_bn_affine(name, p),
            "control": False}[scenario]


def _make(kind, dev):
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.posenet_single import PoseNet
    torch.manual_seed(0)
    net = DepthNet(18, pretrained=False) if kind == "depth" else PoseNet(18, pretrained=False, num_input_images=2)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    return net.to(dev).train(), sd


def _loss(kind, out, cots, dev=None):
    if kind == "depth":
        return sum((out[("disp", s)] * (c.to(dev) if dev is not None else c).to(out[("disp", s)].dtype)).sum() for s, c in enumerate(cots))
    aa, t = out
    c = cots[0].to(dev) if dev is not None else cots[0]
    return (torch.cat([aa, t], -1) * c.to(aa.dtype)).sum()


@pytest.fixture(scope="module")
def truth(gpu_device):
    """Per network: the input, the cotangents, the fp64 oracle gradients of every parameter, the fp32 oracle's worst rel-L2
    error against them, the flip term, and the all-trainable control's BatchNorm buffers after one forward.  Computed once."""
    from oracle import networks as ON
    out = {}
    for kind in ("depth", "pose"):
        net, sd = _make(kind, gpu_device)
        gen = torch.Generator().manual_seed(31)
        x = torch.rand(B, 3 if kind == "depth" else 6, H, W, generator=gen)
        if kind == "depth":
            cots = [torch.randn(B, 1, H >> s, W >> s, generator=gen) for s in range(4)]
        else:
            cots = [torch.randn(B, 1, 1, 6, generator=gen)]
        grads = {}
        for dtype in (torch.float64, torch.float32):
            s = {k: (v.to(dtype) if v.is_floating_point() else v).clone().requires_grad_(
                v.is_floating_point() and ".fc." not in k and "running" not in k) for k, v in sd.items()}
            o = (ON.depthnet if kind == "depth" else ON.posenet)(x.to(dtype), s, train=True)
            _loss(kind, o, cots).backward()
            grads[dtype] = {k: v.grad for k, v in s.items() if v.requires_grad}
        worst_cpu = max(rel(grads[torch.float32][k], grads[torch.float64][k]) for k in grads[torch.float64])
        # smallest ReLU map: layer 4 of the encoder (512 channels at H/32 x W/32) / the pose decoder (256 channels there)
        flip = 1.0 / (B * (H // 32) * (W // 32) * (512 if kind == "depth" else 256)) ** 0.5
        net(x.to(gpu_device))
        buffers = {n: b.detach().clone() for n, b in net.named_buffers()}
        out[kind] = dict(x=x, cots=cots, g64=grads[torch.float64], bound=3.0 * worst_cpu + 2.0 * flip, worst_cpu=worst_cpu,
                         buffers=buffers)
    return out


def _step(kind, scenario, dev, t, arena):
    """One forward + backward of a fresh network with the scenario's parameters frozen; returns what the checks need."""
    from deep_visual_slam_amd import dp, gradsink
    net, _ = _make(kind, dev)
    frozen = {n for n, p in net.named_parameters() if _frozen(scenario, n, p)}
    for n, p in net.named_parameters():
        p.requires_grad_(n not in frozen)
    flat = opt = None
    if arena:
        flat = dp.FlatParams(dp.trainable_parameters(net), grad_sinks=True)
        opt = dp.FusedAdam(flat, lr=1e-3)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    out = net(t["x"].to(dev))
    _loss(kind, out, t["cots"], dev).backward()
    gradsink.join()
    torch.cuda.synchronize()
    return net, frozen, flat, opt, before


def _check(kind, scenario, net, frozen, t):
    trainable = [(n, p) for n, p in net.named_parameters() if n not in frozen and ".fc." not in n]
    assert trainable and (frozen or scenario == "control")
    for n, p in net.named_parameters():
        if n in frozen:
            assert p.grad is None, "frozen parameter %s received a gradient" % n
    for n, p in trainable:
        assert p.grad is not None, "trainable parameter %s has no gradient" % n
    worst = max((rel(p.grad, t["g64"][n]), n) for n, p in trainable)
    print("%s / %s: worst gradient error vs fp64 %.2e at %s over %d tensors (bound %.2e; fp32 CPU oracle %.2e)"
          % (kind, scenario, worst[0], worst[1], len(trainable), t["bound"], t["worst_cpu"]))
    assert worst[0] <= t["bound"], (scenario, worst, t["bound"])
    for n, b in net.named_buffers():
        if "num_batches_tracked" in n:
            assert int(b) == int(t["buffers"][n]), n
        elif ".fc." not in n:
            assert rel(b, t["buffers"][n]) < 1e-5, n


SCENARIOS = [("depth", "encoder"), ("depth", "decoder"), ("depth", "bn_and_bias"), ("depth", "only_bn"), ("depth", "control"),
             ("pose", "encoder")]


@pytest.mark.parametrize("kind,scenario", SCENARIOS, ids=["%s-%s" % s for s in SCENARIOS])
def test_frozen_parameters(gpu_device, truth, kind, scenario):
    t = truth[kind]
    net, frozen, _, _, _ = _step(kind, scenario, gpu_device, t, arena=False)
    _check(kind, scenario, net, frozen, t)


@pytest.mark.parametrize("scenario", ["encoder", "decoder"])
def test_frozen_parameters_with_a_gradient_arena(gpu_device, truth, scenario):
    """dp.FlatParams over the trainable parameters only, gradient sinks on: the arena holds exactly the trainable tensors, its
    gradients meet the same bound, and one dp.FusedAdam step leaves every frozen weight bit-identical."""
    t = truth["depth"]
    net, frozen, flat, opt, before = _step("depth", scenario, gpu_device, t, arena=True)
    params = dict(net.named_parameters())
    want = [n for n in params if n not in frozen and ".fc." not in n]
    assert sorted(n.split(".", 1)[1] for n in flat.names) == sorted(want)
    assert flat.numel == sum((params[n].numel() + 3) // 4 * 4 for n in want)
    for n in want:                                           # the gradients live in the arena
        o = flat.offsets[flat.names.index("0." + n)]
        assert params[n].grad.data_ptr() == flat.grads.data_ptr() + 4 * o
    _check("depth", scenario + " (arena)", net, frozen, t)
    opt.step()
    torch.cuda.synchronize()
    for n, p in params.items():
        if n in frozen or ".fc." in n:
            assert torch.equal(p.detach(), before[n]), "frozen weight %s changed in the optimiser step" % n
    moved = sum(not torch.equal(params[n].detach(), before[n]) for n in want)
    assert moved == len(want), "%d of %d trainable tensors did not move" % (len(want) - moved, len(want))
