"""Inference path (eval() + no_grad: BatchNorm folded into the convolutions, identity + ReLU in the conv epilogue,
optional HIP-graph replay) against the CPU oracle's eval-mode networks.  SURVEY.md section 8(f) rank 2."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _randomise_bn(net, seed):
    """Non-trivial running statistics and affine parameters, as a trained checkpoint has."""
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.5 + 0.25)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)


@pytest.fixture(scope="module")
def eval_nets(gpu_device):
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.posenet_single import PoseNet
    torch.manual_seed(0)
    dn, pn = DepthNet(18, pretrained=False), PoseNet(18, pretrained=False, num_input_images=2)
    _randomise_bn(dn, 1)
    _randomise_bn(pn, 2)
    sd_d = {k: v.clone() for k, v in dn.state_dict().items()}
    sd_p = {k: v.clone() for k, v in pn.state_dict().items()}
    return dn.to(gpu_device).eval(), pn.to(gpu_device).eval(), sd_d, sd_p


def test_eval_networks_match_oracle(gpu_device, eval_nets):
    from oracle import networks as ON
    dn, pn, sd_d, sd_p = eval_nets
    torch.manual_seed(5)
    x = torch.rand(1, 3, 96, 128)
    x6 = torch.rand(1, 6, 96, 128)
    ref = ON.depthnet(x, sd_d, train=False)
    aa_r, t_r = ON.posenet(x6, sd_p, train=False)
    with torch.no_grad():
        out = dn(x.to(gpu_device))
        aa, t = pn(x6.to(gpu_device))
    for s in range(4):
        assert out[("disp", s)].shape == ref[("disp", s)].shape
        assert rel(out[("disp", s)], ref[("disp", s)]) < 2e-4
    assert rel(aa, aa_r) < 2e-4 and rel(t, t_r) < 2e-4
    # buffers are untouched in eval mode
    assert int(dn.state_dict()["encoder.encoder.bn1.num_batches_tracked"]) == 0
    assert torch.equal(dn.state_dict()["encoder.encoder.bn1.running_mean"].cpu(), sd_d["encoder.encoder.bn1.running_mean"])


def test_fold_follows_weight_updates(gpu_device, eval_nets):
    """The cached fold is refreshed when a weight or a running statistic changes in place (load_state_dict, optimiser)."""
    from oracle import networks as ON
    dn, _, sd_d, _ = eval_nets
    x = torch.rand(1, 3, 64, 96)
    with torch.no_grad():
        before = dn(x.to(gpu_device))[("disp", 0)].clone()
        sd2 = {k: v.clone() for k, v in sd_d.items()}
        sd2["encoder.encoder.layer1.0.bn1.running_var"] *= 3.0
        sd2["encoder.encoder.layer2.0.conv1.weight"] *= 0.5
        dn.load_state_dict(sd2)
        after = dn(x.to(gpu_device))[("disp", 0)]
    ref = ON.depthnet(x, sd2, train=False)[("disp", 0)]
    assert rel(after, ref) < 2e-4 and rel(before, ref) > 1e-3
    dn.load_state_dict(sd_d)


def test_graph_replay_and_scale_selection(gpu_device, eval_nets):
    from deep_visual_slam_amd import inference
    dn, pn, _, _ = eval_nets
    inference.prepare(dn, pn, scales=(0,))
    try:
        torch.manual_seed(6)
        x = torch.rand(1, 3, 96, 128, device=gpu_device)
        x6 = torch.rand(1, 6, 96, 128, device=gpu_device)
        with torch.no_grad():
            eager = dn(x)
            assert list(eager) == [("disp", 0)]
            d0 = eager[("disp", 0)].clone()
            aa0, t0 = [v.clone() for v in pn(x6)]
        gd, gp = inference.Graphed(dn, torch.zeros_like(x)), inference.Graphed(pn, torch.zeros_like(x6))
        for _ in range(2):                       # a replay depends on the copied-in input only (the graphs were captured
            out = gd(x)                          # on zeros); split-K layers sum with atomics, so not bit-for-bit
            aa, t = gp(x6)
            assert rel(out[("disp", 0)], d0) < 1e-5
            assert rel(aa, aa0) < 1e-5 and rel(t, t0) < 1e-5
        with pytest.raises(Exception):
            gd(torch.zeros(1, 3, 64, 64, device=gpu_device))
    finally:
        dn.inference_scales = None


def test_eval_with_grad_keeps_autograd(gpu_device, eval_nets):
    """eval() without no_grad (frozen-BatchNorm fine-tuning) stays differentiable: the fold is an inference-only path."""
    dn, _, _, _ = eval_nets
    x = torch.rand(1, 3, 64, 96, device=gpu_device)
    out = dn(x)[("disp", 0)]
    assert out.requires_grad
    out.mean().backward()
    assert dn.encoder.encoder.layer1[0].conv1.weight.grad is not None
    dn.zero_grad()


def worst(a, b):
    """max |a - b| / max |b|: one wrong row at a tile edge shows here, not in an L2 norm over the map."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _oracle(kind, x, sd, dtype, grad=False):
    from oracle import networks as ON
    s = {k: (v.to(dtype) if v.is_floating_point() else v).clone() for k, v in sd.items()}
    if grad:
        for k, v in s.items():
            v.requires_grad_(v.is_floating_point() and ".fc." not in k and "running" not in k)
    out = (ON.depthnet if kind == "depth" else ON.posenet)(x.to(dtype), s, train=False)
    return out, s


def _named_outputs(kind, out):
    if kind == "depth":
        return {"disp%d" % s: out[("disp", s)] for s in range(4) if ("disp", s) in out}
    return {"axisangle": out[0], "translation": out[1]}


@pytest.mark.parametrize("B,H,W", [(3, 64, 96), (1, 96, 128)], ids=["b3_64x96", "b1_96x128"])
def test_eval_networks_worst_element(gpu_device, eval_nets, B, H, W):
    """DepthNet and PoseNet under eval() + no_grad, every output by its worst element against the fp64 oracle: the four
    disparities (also with inference_scales = (0,) and (0, 2), which must return exactly those heads with the same values),
    axis-angle and translation.  Bound: the larger of 2e-5 and 3 x the same measure of the oracle run in fp32 on the CPU.

    Measured on the MI355X, GPU / fp32 CPU oracle (3 x the oracle's figure stays below 2e-5, so every bound is 2e-5):
                       b3 64x96              b1 96x128
        disp0          1.4e-07 / 1.4e-07     1.3e-07 / 1.5e-07      (scales (0,): 1.3e-07, 1.3e-07; (0, 2): 1.3e-07, 1.2e-07)
        disp1          1.7e-07 / 2.5e-07     1.7e-07 / 2.3e-07
        disp2          4.6e-07 / 7.3e-07     5.3e-07 / 7.2e-07      (scales (0, 2): 4.4e-07, 3.9e-07)
        disp3          1.1e-06 / 2.2e-06     8.3e-07 / 2.0e-06
        axis-angle     7.8e-07 / 8.2e-07     1.6e-07 / 1.2e-07
        translation    4.0e-07 / 7.2e-07     3.0e-07 / 5.2e-07"""
    dn, pn, sd_d, sd_p = eval_nets
    gen = torch.Generator().manual_seed(40 + B)
    inputs = {"depth": torch.rand(B, 3, H, W, generator=gen), "pose": torch.rand(B, 6, H, W, generator=gen)}
    bad = []
    for kind, net, sd in (("depth", dn, sd_d), ("pose", pn, sd_p)):
        x = inputs[kind]
        with torch.no_grad():
            o64 = _named_outputs(kind, _oracle(kind, x, sd, torch.float64)[0])
            o32 = _named_outputs(kind, _oracle(kind, x, sd, torch.float32)[0])
            runs = [(None, _named_outputs(kind, net(x.to(gpu_device))))]
            if kind == "depth":
                try:
                    for scales in ((0,), (0, 2)):
                        dn.inference_scales = scales
                        got = _named_outputs(kind, net(x.to(gpu_device)))
                        assert sorted(got) == ["disp%d" % s for s in scales]
                        runs.append((scales, got))
                finally:
                    dn.inference_scales = None
        for scales, got in runs:
            assert scales is not None or sorted(got) == sorted(o64)
            for name, v in got.items():
                yard = worst(o32[name], o64[name])
                bound = max(2e-5, 3.0 * yard)
                err = worst(v, o64[name])
                print("b%d %dx%d %s%s: GPU %.2e  fp32 CPU oracle %.2e  bound %.2e" % (B, H, W, name, "" if scales is None else " scales=%s" % (scales,),
                                                                                     err, yard, bound))
                if not err <= bound:
                    bad.append((name, scales, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("kind", ["depth", "pose"])
def test_eval_with_grad_gradients_match_oracle(gpu_device, eval_nets, kind):
    """eval() with autograd (frozen-BatchNorm fine-tuning, a validation loss without no_grad): whole networks at batch 2,
    96 x 128, random cotangents as in tests/test_frozen_gpu.py; every parameter's gradient against the fp64 oracle with
    train=False.  Yardstick of that file, unchanged: rel-L2 per tensor <= 3 x (worst fp32-oracle error against fp64) + 2 x flip,
    flip = 1 / sqrt(elements of the smallest ReLU map).  The BatchNorm buffers must stay bit-identical.

    Measured on the MI355X: DepthNet worst 3.5e-06 (layer4.1.bn1.weight; fp32 oracle 1.7e-05, flip 9.0e-03, bound 1.8e-02);
    PoseNet worst 2.4e-04 (layer2.0.downsample.1.weight; fp32 oracle 2.0e-06, flip 1.3e-02, bound 2.6e-02)."""
    from deep_visual_slam_amd import gradsink
    from test_frozen_gpu import _loss, rel as rel_checked
    dn, pn, sd_d, sd_p = eval_nets
    net, sd = (dn, sd_d) if kind == "depth" else (pn, sd_p)
    B, H, W = 2, 96, 128
    gen = torch.Generator().manual_seed(31)
    x = torch.rand(B, 3 if kind == "depth" else 6, H, W, generator=gen)
    cots = ([torch.randn(B, 1, H >> s, W >> s, generator=gen) for s in range(4)] if kind == "depth"
            else [torch.randn(B, 1, 1, 6, generator=gen)])
    grads = {}
    for dtype in (torch.float64, torch.float32):
        o, s = _oracle(kind, x, sd, dtype, grad=True)
        _loss(kind, o, cots).backward()
        grads[dtype] = {k: v.grad for k, v in s.items() if v.requires_grad}
    worst_cpu = max(rel_checked(grads[torch.float32][k], grads[torch.float64][k]) for k in grads[torch.float64])
    flip = 1.0 / (B * (H // 32) * (W // 32) * (512 if kind == "depth" else 256)) ** 0.5
    bound = 3.0 * worst_cpu + 2.0 * flip
    before = {n: b.detach().clone() for n, b in net.named_buffers()}
    net.zero_grad()
    try:
        assert not net.training and torch.is_grad_enabled()
        _loss(kind, net(x.to(gpu_device)), cots, gpu_device).backward()
        gradsink.join()
        torch.cuda.synchronize()
        params = [(n, p) for n, p in net.named_parameters() if ".fc." not in n]
        assert sorted(n for n, _ in params) == sorted(grads[torch.float64])
        for n, p in params:
            assert p.grad is not None, n
        got = max((rel_checked(p.grad, grads[torch.float64][n]), n) for n, p in params)
    finally:
        net.zero_grad()
    print("%s eval() with autograd: worst gradient error vs fp64 %.2e at %s over %d tensors (bound %.2e; fp32 CPU oracle %.2e, flip %.2e)"
          % (kind, got[0], got[1], len(params), bound, worst_cpu, flip))
    assert got[0] <= bound, (got, bound)
    for n, b in net.named_buffers():
        assert torch.equal(b, before[n]), n
        if ".fc." not in n and n in sd:
            assert torch.equal(b.cpu(), sd[n]), n


def test_frame_predictor_two_streams(gpu_device, eval_nets):
    """PoseNet and DepthNet side by side (eager and as one graph with a fork / join) equal the sequential calls."""
    from deep_visual_slam_amd import inference
    from deep_visual_slam_amd.layers import disp_to_depth, transformation_from_parameters
    dn, pn, _, _ = eval_nets
    inference.prepare(dn, pn, scales=(0,))
    try:
        torch.manual_seed(8)
        x = torch.rand(1, 3, 96, 128, device=gpu_device)
        x6 = torch.rand(1, 6, 96, 128, device=gpu_device)
        with torch.no_grad():
            aa, t = pn(x6)
            T0 = transformation_from_parameters(aa[:, 0], t[:, 0], invert=False).clone()
            d0 = disp_to_depth(dn(x)[("disp", 0)], 0.1, 10.0)[1].clone()
        for graph in (False, True):
            fp = inference.FramePredictor(dn, pn, torch.zeros_like(x), torch.zeros_like(x6), graph=graph)
            for _ in range(2):
                T, depth, disp = fp(x, x6)
                torch.cuda.synchronize()
                assert rel(T, T0) < 1e-5 and rel(depth, d0) < 1e-5 and disp.shape == (1, 1, 96, 128)
    finally:
        dn.inference_scales = None
