"""FlowPoseNet on the GPU (posenet_single.py, csrc/posehead.hip) against tests/flowpose_ref.py in fp64: the three regressor
convolutions alone, the pooling-head entries alone through the C ABI and their edges, the regressor's gradients element-wise, the
whole network, the fixture the reference's own FlowPoseNet produced, and the network as pose_net of MonodepthTrainer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flowpose_ref as P
import raft_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
CL = torch.channels_last
FIXTURE = "flowposenet_b2_128x136.npz"
# Pixels of one slice of csrc/posehead.hip: one workgroup's share of a sample.  A literal, because the cases below are
# built at import, before a library can be loaded; test_slice_constant_is_the_library_s pins it to dvs_pool_fc_slice_pixels(), so a
# change of the kernel's constant fails there and cannot silently un-rag the cases.
T = 256


def make_net(weights, dev, strict=True, **kw):
    from deep_visual_slam_amd.posenet_single import FlowPoseNet
    model = FlowPoseNet(None, **kw)
    model.load_state_dict(weights, strict=strict)
    return model.to(dev)


# ---- 1: the regressor's convolutions alone --------------------------------------------------------------------------------------
def layer_input_size(size, layer):
    h, w = size
    for _, _, _, k, s, p in P.REGRESSOR[:layer]:
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return h, w


@pytest.mark.parametrize("layer", [0, 1, 2], ids=["7x7s2_c4", "5x5s2_c32", "3x3s2_c64"])
@pytest.mark.parametrize("size", [(10, 14), (33, 37)], ids=["10x14", "33x37"])
def test_regressor_convolutions_against_fp64(gpu_device, size, layer):
    """Each of the three strided convolutions through nn_ops.conv2d as FlowPoseNet calls it (layer 0: Cin = 4 with two zero
    channels and a zero-padded filter; ReLU on layers 0 and 1), N = 2, at the size the layer sees for a flow of `size`: y, dx,
    dW, db within max(OUT_TOL / GRAD_TOL of the tensor's max, bound).  The backward is judged on the kernel's own ReLU mask, so the
    forward's rounding is not charged to it."""
    from deep_visual_slam_amd import nn_ops
    name, co, ci, k, stride, pad = P.REGRESSOR[layer]
    relu = layer != 2
    h, w = layer_input_size(size, layer)
    gen = torch.Generator().manual_seed(100 * layer + size[0])
    wts = P.make_regressor_weights(31 + layer)
    x = (2.0 if layer == 0 else 1.0) * torch.randn(2, ci, h, w, generator=gen)
    wt, b = wts[name + ".weight"], wts[name + ".bias"]
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    dy = torch.randn(2, co, ho, wo, generator=gen)
    if layer == 0:
        xd = F.pad(x.permute(0, 2, 3, 1), (0, 2)).permute(0, 3, 1, 2).to(gpu_device).requires_grad_(True)
        wparam = wt.to(gpu_device).requires_grad_(True)
        wd = F.pad(wparam, (0, 0, 0, 0, 0, 2)).contiguous(memory_format=CL)
    else:
        xd = x.contiguous(memory_format=CL).to(gpu_device).requires_grad_(True)
        wparam = wt.contiguous(memory_format=CL).to(gpu_device).requires_grad_(True)
        wd = wparam
    bd = b.to(gpu_device).requires_grad_(True)
    y = nn_ops.conv2d(xd, wd, bd, stride, pad, act="relu" if relu else None)
    g = torch.autograd.grad(y, [xd, wparam, bd], dy.to(gpu_device))
    torch.cuda.synchronize()
    assert tuple(y.shape) == (2, co, ho, wo)
    mask = (y.detach().cpu() > 0) if relu else torch.ones_like(dy, dtype=torch.bool)
    ref = {}
    for dt in (torch.float64, torch.float32):
        r = [t.to(dt).requires_grad_(True) for t in (x, wt, b)]
        pre = F.conv2d(r[0], r[1], r[2], stride=stride, padding=pad)
        grads = torch.autograd.grad(pre, r, dy.to(dt) * mask.to(dt))
        ref[dt] = [(F.relu(pre) if relu else pre).detach()] + [t.detach() for t in grads]
    got = [y, g[0][:, :ci], g[1], g[2]]
    for i, nm in enumerate(("y", "d/x", "d/W", "d/b")):
        R.U.check_rel("%s %s" % (nm, name), got[i], ref[torch.float64][i], extra=R.bound(ref[torch.float64][i], ref[torch.float32][i]))
    assert torch.isfinite(g[0]).all()


# ---- 2: the pooling head alone, through the C ABI ------------------------------------------------------------------------------
def run_pool_fc(y, W, b, dout, relu, scale, dev, fill=float("nan")):
    """Forward and backward entry on CPU tensors y [N,P,C], W [J,C], b [J] or None, dout [N,J]; every output buffer starts as NaN."""
    from deep_visual_slam_amd import _lib
    lib = _lib.lib()
    N, Pn, Cn = y.shape
    J = W.shape[0]
    d = lambda t: t.to(dev).contiguous() if t is not None else None
    yd, Wd, bd, gd = d(y), d(W), d(b), d(dout)
    new = lambda *s: torch.full(s, fill, device=dev)
    out, mean, dy, dW = new(N, J), new(N, Cn), new(N, Pn, Cn), new(J, Cn)
    db = new(J) if b is not None else None
    nbytes = int(lib.dvs_pool_fc_workspace(N, Pn, Cn))
    assert nbytes == N * -(-Pn // T) * Cn * 4
    ws = new(nbytes // 4)
    p = lambda t: t.data_ptr() if t is not None else None
    _lib.check(lib.dvs_pool_fc_fwd(p(yd), p(Wd), p(bd), p(out), p(mean), p(ws), nbytes, N, Pn, Cn, J, relu, scale, _lib.stream()),
               "dvs_pool_fc_fwd")
    _lib.check(lib.dvs_pool_fc_bwd(p(gd), p(yd), p(mean), p(Wd), p(dy), p(dW), p(db), N, Pn, Cn, J, relu, scale, _lib.stream()),
               "dvs_pool_fc_bwd")
    torch.cuda.synchronize()
    got = {"out": out.cpu(), "mean": mean.cpu(), "d/y": dy.cpu(), "d/W": dW.cpu()}
    if b is not None:
        got["d/b"] = db.cpu()
    return got


def pool_fc_refs(y, W, b, dout, relu, scale):
    """{name: (fp64, fp32)}: the issue's formulas by torch autograd on the CPU."""
    refs = {}
    for dt in (torch.float64, torch.float32):
        ops = [t.to(dt).requires_grad_(True) for t in (y, W) + ((b,) if b is not None else ())]
        out, mean = P.pool_fc(ops[0], ops[1], ops[2] if b is not None else None, relu, scale)
        grads = torch.autograd.grad(out, ops, dout.to(dt))
        o = {"out": out.detach(), "mean": mean.detach(), "d/y": grads[0], "d/W": grads[1]}
        if b is not None:
            o["d/b"] = grads[2]
        for k, v in o.items():
            refs.setdefault(k, []).append(v)
    return refs


def pool_fc_operands(N, Pn, Cn, J, seed):
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(N, Pn, Cn, generator=gen) * (0.5 + torch.rand(1, 1, Cn, generator=gen)) + 0.5 * torch.randn(1, 1, Cn, generator=gen)
    return y, torch.randn(J, Cn, generator=gen) / np.sqrt(Cn), 0.1 * torch.randn(J, generator=gen), torch.randn(N, J, generator=gen)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_slice_constant_is_the_library_s(gpu_device):
    from deep_visual_slam_amd import posenet_single
    assert posenet_single.pool_fc_slice_pixels() == T


POOL_CASES = [(Cn, J, N, Pn) for Cn in (4, 24, 128) for J in (1, 6) for N in (1, 3) for Pn in (1, T - 1, T, T + 1, 2 * T + 5)]


@pytest.mark.parametrize("Cn,J,N,Pn", POOL_CASES, ids=["c%d_j%d_n%d_p%d" % c for c in POOL_CASES])
def test_pool_fc_entries_against_fp64(gpu_device, Cn, J, N, Pn):
    """relu in {0, 1}, b NULL and not: out, mean, dy, dW, db within max(OUT_TOL / GRAD_TOL of the tensor's max, bound) of the fp64
    formulas; NaN-filled buffers end finite; two runs agree bit for bit."""
    y, W, b, dout = pool_fc_operands(N, Pn, Cn, J, seed=Cn * 100003 + Pn * 7 + N * 3 + J)
    for relu in (0, 1):
        for bias in (None, b):
            tag = "C%d J%d N%d P%d relu%d %s" % (Cn, J, N, Pn, relu, "b" if bias is not None else "nob")
            got = run_pool_fc(y, W, bias, dout, relu, P.POSE_SCALE, gpu_device)
            again = run_pool_fc(y, W, bias, dout, relu, P.POSE_SCALE, gpu_device)
            refs = pool_fc_refs(y, W, bias, dout, relu, P.POSE_SCALE)
            assert sorted(got) == sorted(refs)
            for k, (r64, r32) in refs.items():
                assert torch.isfinite(got[k]).all(), (tag, k, "not every element was written, or not finite")
                assert same_bits(got[k], again[k]), "%s %s differs between two runs" % (tag, k)
                R.U.check_rel(k + " " + tag, got[k], r64, extra=R.bound(r64, r32))


def test_pool_fc_all_negative(gpu_device):
    """relu = 1 on an all-negative y: the mean is 0, out is scale * b exactly, dy is 0 exactly."""
    y, W, b, dout = pool_fc_operands(3, 2 * T + 5, 24, 6, seed=3)
    y = -y.abs() - 1e-3
    got = run_pool_fc(y, W, b, dout, 1, P.POSE_SCALE, gpu_device)
    assert torch.equal(got["mean"], torch.zeros(3, 24))
    assert torch.equal(got["out"], (torch.tensor(P.POSE_SCALE, dtype=torch.float32) * b)[None].repeat(3, 1))
    assert torch.equal(got["d/y"], torch.zeros_like(y)) and torch.equal(got["d/W"], torch.zeros(6, 24))
    got = run_pool_fc(y, W, None, dout, 1, P.POSE_SCALE, gpu_device)
    assert torch.equal(got["out"], torch.zeros(3, 6))


def test_pool_fc_zero_elements_get_no_gradient(gpu_device):
    y, W, b, dout = pool_fc_operands(2, T + 9, 24, 6, seed=4)
    zero = torch.rand(y.shape, generator=torch.Generator().manual_seed(5)) < 0.25
    y[zero] = 0.0
    y[0, 3, 5] = -0.0
    got = run_pool_fc(y, W, b, dout, 1, P.POSE_SCALE, gpu_device)
    assert torch.equal(got["d/y"][y == 0], torch.zeros(int((y == 0).sum())))
    assert (got["d/y"][y > 0] != 0).all()
    refs = pool_fc_refs(y, W, b, dout, 1, P.POSE_SCALE)
    R.U.check_rel("d/y with zeros", got["d/y"], refs["d/y"][0], extra=R.bound(*refs["d/y"]))


@pytest.mark.parametrize("Pn", [1, T - 1, 2 * T + 5, 60 * 80])
def test_pool_fc_constant_channel(gpu_device, Pn):
    """A channel that is constant over a sample gets its value back to within 2 ulp, whatever its sign with relu = 0; with relu = 1
    a negative constant gives exactly 0."""
    y, W, b, dout = pool_fc_operands(2, Pn, 24, 6, seed=6)
    values = {(0, 3): 0.1, (1, 8): -7.3, (0, 20): 0.0, (1, 21): 1e6, (0, 13): 1.0 / 3.0}
    for (n, c), v in values.items():
        y[n, :, c] = v
    for relu in (0, 1):
        got = run_pool_fc(y, W, b, dout, relu, P.POSE_SCALE, gpu_device)
        for (n, c), v in values.items():
            want = np.float32(max(v, 0.0) if relu else v)
            err = abs(float(got["mean"][n, c]) - float(want))
            assert err <= 2.0 * float(np.spacing(np.abs(want))), (relu, n, c, v, float(got["mean"][n, c]))


def test_pool_fc_samples_do_not_see_each_other(gpu_device):
    """Row n of a batch of 3 is, bit for bit, the N = 1 call on that sample (out, mean, dy); one sample is all zeros."""
    y, W, b, dout = pool_fc_operands(3, 2 * T + 5, 128, 6, seed=7)
    y[1] = 0
    both = run_pool_fc(y, W, b, dout, 1, P.POSE_SCALE, gpu_device)
    for n in range(3):
        one = run_pool_fc(y[n:n + 1], W, b, dout[n:n + 1], 1, P.POSE_SCALE, gpu_device)
        for k in ("out", "mean", "d/y"):
            assert same_bits(both[k][n:n + 1], one[k]), (n, k)


def test_pool_fc_takes_operands_that_are_not_16_byte_aligned(gpu_device):
    """posenet_single.pool_fc with a bias and a cotangent that are slices of larger tensors (rows of 6 floats: 8-byte aligned
    only): the entries demand 16-byte alignment, the wrapper copies; values against the fp64 formulas."""
    from deep_visual_slam_amd import posenet_single
    y, W, b, dout = pool_fc_operands(2, T + 9, 24, 6, seed=8)
    refs = pool_fc_refs(y, W, b, dout, 1, P.POSE_SCALE)
    yd = y.view(2, T + 9, 1, 24).permute(0, 3, 1, 2).to(gpu_device).requires_grad_(True)
    Wd = W.to(gpu_device).requires_grad_(True)
    bd = torch.cat([torch.zeros(2), b]).to(gpu_device)[2:].requires_grad_(True)
    gd = torch.cat([torch.zeros(1, 6), dout]).to(gpu_device)[1:]
    assert bd.data_ptr() % 16 and gd.data_ptr() % 16 and gd.is_contiguous()
    out = posenet_single.pool_fc(yd, Wd, bd, relu=True, scale=P.POSE_SCALE)
    g = torch.autograd.grad(out, [yd, Wd, bd], gd)
    torch.cuda.synchronize()
    got = {"out": out, "d/y": g[0].permute(0, 2, 3, 1).reshape(2, T + 9, 24), "d/W": g[1], "d/b": g[2]}
    for k, have in got.items():
        R.U.check_rel(k, have, refs[k][0], extra=R.bound(*refs[k]))


# ---- 3: the regressor's gradients, element-wise, where that is well posed -----------------------------------------------------
# seeds: tests/golden/make_golden_flowpose.py --search (the first seed per case that meets the margin condition checked below)
G3_SEEDS = {(16, 24): 2, (24, 40): 1}


@pytest.mark.parametrize("size", P.G3_SIZES, ids=["%dx%d" % s for s in P.G3_SIZES])
def test_regressor_gradients_elementwise(gpu_device, size):
    """2 flows, random cotangent: the pose, the gradient of the flow and of every regressor parameter within
    max(OUT_TOL / GRAD_TOL * max |ref|, bound).  Well posed only when no ReLU mask can flip: the test first checks that the fp64
    run's smallest relative ReLU margin is at least 16 x the largest relative pre-activation difference between the restatement's
    fp32 and fp64 runs."""
    w, flow, cot = P.g3_case(size, G3_SEEDS[size])
    margin, diff = P.regressor_margins(w, flow)
    print("margin %.3e, fp32-vs-fp64 pre-activation difference %.3e" % (margin, diff))
    assert margin >= 16 * diff, "seed does not qualify: run tests/golden/make_golden_flowpose.py --search"
    r64, r32 = P.run_regressor(w, flow, cot, torch.float64), P.run_regressor(w, flow, cot, torch.float32)
    model = make_net(w, gpu_device, strict=False)
    fd = flow.to(gpu_device).requires_grad_(True)
    params = [(k, p) for k, p in model.named_parameters() if not k.startswith("flow_net.")]
    assert [k for k, _ in params] == list(w)
    out = model.regress(fd)
    grads = torch.autograd.grad(out, [fd] + [p for _, p in params], cot.to(gpu_device))
    torch.cuda.synchronize()
    R.U.check_rel("out", out, r64["out"], extra=R.bound(r64["out"], r32["out"]))
    for k, g in zip(["flow"] + [k for k, _ in params], grads):
        R.U.check_rel("d/" + k, g, r64["d/" + k], extra=R.bound(r64["d/" + k], r32["d/" + k]))


# ---- 4: FlowPoseNet end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net_refs():
    """(inputs, fp64 run, fp32 run) of the restatement: computed once, never modified."""
    w, images, cot = P.g4_case()
    it = P.G4["iters"]
    return (w, images, cot), P.run_net(w, images, cot, torch.float64, it), P.run_net(w, images, cot, torch.float32, it)


def check_zero_bias(tag, key, got, ref32, weight_grad64):
    """test_raft_gpu.py's rule for the conv biases in front of an instance norm, whose gradients are mathematically zero."""
    b = max(3.0 * float(ref32.abs().max()), R.ulp_floor(float(weight_grad64.abs().max())))
    err = float(got.detach().double().cpu().abs().max())
    print("%s %s (zero-gradient bias): max |value| %.3e, bound %.3e" % (tag, key, err, b))
    assert err <= b, (tag, key, err, b)


@pytest.mark.parametrize("alternate", [False, True], ids=["corr", "altcorr"])
def test_flowposenet_end_to_end(gpu_device, net_refs, alternate):
    """B=2, 128x136, iters=3.  Both outputs within max(OUT_TOL * max, bound).  Gradients: per parameter tensor the relative L2 error
    is held to max(GRAD_TOL, 3 e32) + sqrt(K) f with e32, K, f from the fixture (make_golden_flowpose.py); the zero-gradient biases
    of fnet follow their own rule.  A batch [a; b] with pairs=2 equals a and b run separately within OUT_TOL of the max.  The
    forward under no_grad in eval() equals the training forward bit for bit in the deterministic mode."""
    from deep_visual_slam_amd import _lib
    rec = load_golden(FIXTURE)
    assert [int(v) for v in rec["g4/config"]] == [P.G4[k] for k in ("image_seed", "weight_seed", "cot_seed")]
    (w, images, cot), r64, r32 = net_refs
    model = make_net(w, gpu_device, iters=P.G4["iters"], alternate_corr=alternate)
    x = images.to(gpu_device)
    aa, t = model(x)
    assert tuple(aa.shape) == tuple(t.shape) == (2, 1, 1, 3)
    loss = (aa * cot[0].to(gpu_device)).sum() + (t * cot[1].to(gpu_device)).sum()
    grads = torch.autograd.grad(loss, list(model.parameters()))
    torch.cuda.synchronize()
    got = {"d/" + k: g.cpu() for (k, _), g in zip(model.named_parameters(), grads)}
    for name, have in (("aa", aa), ("t", t)):
        R.U.check_rel(name, have, r64[name], extra=R.bound(r64[name], r32[name]))
    K, f = int(rec["g4/K"]), float(rec["g4/f"])
    keys = [str(k) for k in rec["meta/keys"]]
    assert keys == [k for k, _ in model.named_parameters()]
    zero = R.zero_gradient_biases("flow_net.fnet.")
    print("K %d, f %.3e" % (K, f))
    for key, e32 in zip(keys, rec["g4/e32"]):
        if key in zero:
            check_zero_bias("g4", key, got["d/" + key], torch.tensor(float(rec["g4/zb32"][zero.index(key)])),
                            r64["d/" + key.replace(".bias", ".weight")])
            continue
        err, b = R.rel_l2(got["d/" + key], r64["d/" + key]), max(R.GRAD_TOL, 3.0 * float(e32)) + np.sqrt(K) * f
        print("d/%s: relative L2 error %.3e, bound %.3e (e32 %.3e)" % (key, err, b, float(e32)))
        assert err <= b, (key, err, b)
    # pairs: nothing couples the samples
    with torch.no_grad():
        both = torch.cat(model(x, pairs=2), -1)
        alone = torch.cat([torch.cat(model(x[n:n + 1]), -1) for n in range(2)], 0)
    top = float(both.abs().max())
    err = float((both - alone).abs().max())
    print("pairs=2 against separate calls: max |difference| %.3e, bound %.3e" % (err, R.OUT_TOL * top))
    assert err <= R.OUT_TOL * top
    # eval + no_grad against the training forward, in the deterministic mode (no split-K atomics)
    was = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        train = torch.cat(model.train()(x), -1).detach()
        with torch.no_grad():
            infer = torch.cat(model.eval()(x), -1)
    finally:
        _lib.set_deterministic(was)
        model.train()
    assert same_bits(train, infer)


# ---- 5: the fixture the reference produced ---------------------------------------------------------------------------------------
def test_reference_fixture_through_the_gpu_module(gpu_device):
    """The reference's recorded fp32 outputs (B=2, 128x136, its 12 iterations) with the fixture's weights: within
    max(OUT_TOL * max, 3 x the recorded reference-fp32-vs-restatement-fp64 difference)."""
    rec = load_golden(FIXTURE)
    B, H, W, iters, seed = (int(v) for v in rec["meta/config"])
    w = P.make_weights(seed)
    for k, v in w.items():
        assert np.allclose(R.checksum(v), rec["w/cs/" + k], rtol=1e-12, atol=0), "make_weights changed: " + k
    model = make_net(w, gpu_device)
    assert model.iters == iters == 12
    with torch.no_grad():
        aa, t = model((torch.from_numpy(rec["in/images"]).float() / 255).to(gpu_device))
    for name, have in (("aa", aa), ("t", t)):
        R.U.check_rel("fixture " + name, have, torch.from_numpy(rec["ref32/" + name]).double(), extra=3.0 * float(rec["err/" + name]))


# ---- 6: in the trainer -----------------------------------------------------------------------------------------------------------
def test_flowposenet_is_the_trainer_s_pose_net(gpu_device):
    """MonodepthTrainer(DepthNet, FlowPoseNet(None, iters=2)) at 128x160, batch 1, default arena: one process_batch + backward, one
    dp.FusedAdam step, a second process_batch that sees the new weights (through the update block's derived-weight cache)."""
    from deep_visual_slam_amd import dp, gradsink, ops, synth
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.learner_new import MonodepthTrainer
    from deep_visual_slam_amd.posenet_single import FlowPoseNet
    B, H, W = 1, 128, 160
    cfg = {"Train": dict(num_source=1, batch_size=B, img_h=H, img_w=W, smoothness_ratio=0.001, auto_mask=True, ssim_ratio=0.85,
                         min_depth=0.1, max_depth=10.0, use_compile=False)}
    torch.manual_seed(5)
    dn = DepthNet(18, False).to(gpu_device).train()
    pn = FlowPoseNet(None, iters=2).to(gpu_device).train()
    tr = MonodepthTrainer(dn, pn, cfg, gpu_device)
    assert tr.arena is not None and any(p is pn.fc.weight for p in tr.arena.tensors)
    sample = {k: v.to(gpu_device) for k, v in synth.parity_sample(B, H, W).items()}
    left, tgt, right = sample[("source_left", 0)], sample[("target_image", 0)], sample[("source_right", 0)]

    def separate():
        with torch.no_grad():
            aa_l, t_l = pn(torch.cat([left, tgt], 1))
            aa_r, t_r = pn(torch.cat([tgt, right], 1))
            return {-1: ops.pose_to_mat(aa_l[:, 0], t_l[:, 0], invert=True), 1: ops.pose_to_mat(aa_r[:, 0], t_r[:, 0], invert=False)}

    def step():
        outputs, losses = tr.process_batch(dict(sample))
        torch.cuda.synchronize()
        assert all(torch.isfinite(v.detach()).all() for v in losses.values()), losses
        want = separate()
        torch.cuda.synchronize()
        mats = {}
        for f in (-1, 1):
            have = outputs[("cam_T_cam", 0, f)].detach()
            top, err = float(want[f].abs().max()), float((have - want[f]).abs().max())
            print("cam_T_cam %+d: max |difference| %.3e, bound %.3e" % (f, err, R.OUT_TOL * top))
            assert err <= R.OUT_TOL * top
            mats[f] = have.clone()
        return losses, mats

    losses, first = step()
    losses["loss"].backward()
    gradsink.join()
    torch.cuda.synchronize()
    for k, p in pn.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if not k.startswith("flow_net.") or k.startswith("flow_net.update_block."):
            assert float(p.grad.abs().max()) > 0, k
    opt = dp.FusedAdam(tr.arena, lr=1e-3)
    before = {k: p.detach().clone() for k, p in pn.named_parameters() if k in ("fc.weight", "flow_net.update_block.gru.convz.weight")}
    opt.step()
    torch.cuda.synchronize()
    for k, old in before.items():
        assert not torch.equal(dict(pn.named_parameters())[k].detach(), old), k + " did not move"
    _, second = step()
    assert not torch.equal(first[-1], second[-1]) and not torch.equal(first[1], second[1])
