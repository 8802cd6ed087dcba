"""The full-size RAFT on the GPU (raft.py, raft_encoder.py, raft_update.py, csrc/convexup.hip, csrc/shiftstack.hip) against
tests/raft_basic_ref.py in fp64: the shift-stack and convex-upsampling entries alone, their edges, the 1x1 convolution shapes that
are new to the route, BasicEncoder in its four forms, BasicUpdateBlock, and the whole model against the restatement and against
the fixture the reference's own RAFT produced."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import raft_basic_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
CL = torch.channels_last
FIXTURE = "raft_basic_b2_128x136.npz"
EPS = float(np.finfo(np.float32).eps)           # 2^-23
U = R.S.U                                       # raft_update_ref: check_rel and the convolution tolerances


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- 1: dvs_shift_stack_* alone, through the C ABI -------------------------------------------------------------------------------
def run_stack(x, g, axis, dev):
    """x [N,H,W,C], g [N,H,W,5C] CPU tensors -> (x5, dx) from the two entries; every output buffer starts as NaN."""
    from deep_visual_slam_amd import _lib
    lib = _lib.lib()
    N, H, W, Cn = x.shape
    xd, gd = x.to(dev).contiguous(), g.to(dev).contiguous()
    x5, dx = torch.full((N, H, W, 5 * Cn), float("nan"), device=dev), torch.full((N, H, W, Cn), float("nan"), device=dev)
    _lib.check(lib.dvs_shift_stack_fwd(xd.data_ptr(), x5.data_ptr(), N, H, W, Cn, axis, _lib.stream()), "dvs_shift_stack_fwd")
    _lib.check(lib.dvs_shift_stack_bwd(gd.data_ptr(), dx.data_ptr(), N, H, W, Cn, axis, _lib.stream()), "dvs_shift_stack_bwd")
    torch.cuda.synchronize()
    return x5.cpu(), dx.cpu()


STACK_SHAPES = ((1, 1), (1, 3), (2, 5), (5, 2), (7, 9))       # extents 1 and 2: the window is wider than the map


@pytest.mark.parametrize("H,W", STACK_SHAPES, ids=["%dx%d" % s for s in STACK_SHAPES])
@pytest.mark.parametrize("axis", [0, 1])
def test_shift_stack_entries(gpu_device, axis, H, W):
    """C in {4, 128}, N in {1, 3}.  Forward: bit for bit against indexing.  Adjoint: against fp64 within 4 eps sum |terms| per
    element (eps = 2^-23; at most five terms added in order, four roundings of half an eps each).  Two runs agree bit for bit."""
    for Cn in (4, 128):
        for N in (1, 3):
            gen = torch.Generator().manual_seed(1000 * axis + 100 * H + 10 * W + Cn + N)
            x, g = torch.randn(N, H, W, Cn, generator=gen), torch.randn(N, H, W, 5 * Cn, generator=gen)
            x5, dx = run_stack(x, g, axis, gpu_device)
            again = run_stack(x, g, axis, gpu_device)
            assert torch.equal(bits(x5), bits(again[0])) and torch.equal(bits(dx), bits(again[1]))
            nchw = lambda t: t.permute(0, 3, 1, 2)
            assert torch.equal(bits(nchw(x5)), bits(R.shift_stack(nchw(x), axis))), (Cn, N)
            x64 = nchw(x).double().requires_grad_(True)
            y64 = R.shift_stack(x64, axis)
            want, = torch.autograd.grad(y64, x64, nchw(g).double(), retain_graph=True)
            terms, = torch.autograd.grad(y64, x64, nchw(g).double().abs())
            err = (nchw(dx).double() - want).abs()
            assert torch.isfinite(dx).all() and bool((err <= 4 * EPS * terms).all()), (Cn, N, float(err.max()))


# ---- 2: dvs_convex_up_* through raft.upsample_flow --------------------------------------------------------------------------------
def run_convex_gpu(flow, mask, cot, scale, dev):
    from deep_visual_slam_amd import raft
    f = flow.to(dev).requires_grad_(True)
    m = mask.to(dev).contiguous(memory_format=CL).requires_grad_(True)
    out = raft.upsample_flow(f, m, scale)
    assert out.is_contiguous()
    df, dm = torch.autograd.grad(out, [f, m], cot.to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu(), df.cpu(), dm.cpu()


def convex_out_bound(flow):
    """32 eps * 8 * max |flow|: the forward bound derived in test_convex_upsampling_against_fp64."""
    return 32 * EPS * 8 * float(flow.abs().max())


CONVEX_GRAD_FACTOR = 4          # gradients: within this many times the error of torch's fp32 CPU run of the restatement


@pytest.mark.parametrize("h,w,N,scale", R.CONVEX_CASES, ids=["%dx%d_n%d_s%g" % c for c in R.CONVEX_CASES])
def test_convex_upsampling_against_fp64(gpu_device, h, w, N, scale):
    """Forward: every element within 32 eps * 8 * max |flow| of fp64 (eps = 2^-23).  The result is a convex combination of nine
    values 8 * flow_k, each of magnitude at most F = 8 max |flow|: p_k = e_k / s carries expf's 2 ulp twice (in e_k and, through s,
    at most once more), the eight additions of s (4 eps), one division (eps / 2): under 9 eps relative; the nine products add
    eps / 2 each and the nine-term sum 4 eps, all on terms that sum to at most F: 14 eps F at the very worst, and the rounding of
    mask_scale * mask - max moves p_k by |x| e^-|x| eps / 2 <= eps / 5 more.  32 eps F leaves a factor of two.
    Gradients: within 4 x the error torch's fp32 CPU run of the restatement makes on the same inputs (recorded by
    tests/golden/make_golden_raft_basic.py).  Two runs agree bit for bit, backward included."""
    rec = load_golden(FIXTURE)
    flow, mask, cot = R.convex_case(N, h, w, R.convex_seed(h, w, N))
    out, df, dm = run_convex_gpu(flow, mask, cot, scale, gpu_device)
    again = run_convex_gpu(flow, mask, cot, scale, gpu_device)
    for a, b in zip((out, df, dm), again):
        assert torch.equal(bits(a), bits(b))
    o64, df64, dm64 = R.run_convex(flow, mask, cot, scale, torch.float64)
    b = convex_out_bound(flow)
    err = float((out.double() - o64).abs().max())
    print("out: max |err| %.3e, bound %.3e" % (err, b))
    assert torch.isfinite(out).all() and err <= b
    e32 = rec["cvx/%dx%d_n%d_s%g" % (h, w, N, scale)]
    for name, have, want, e in (("dflow", df, df64, e32[0]), ("dmask", dm, dm64, e32[1])):
        err = float((have.double() - want).abs().max())
        print("%s: max |err| %.3e, torch fp32 on the CPU %.3e, bound %.3e" % (name, err, float(e), CONVEX_GRAD_FACTOR * float(e)))
        assert have.shape == want.shape and torch.isfinite(have).all() and err <= CONVEX_GRAD_FACTOR * float(e), (name, err, float(e))


def test_convex_upsampling_one_gradient_alone(gpu_device):
    """Only flow, or only the mask, requires a gradient: the backward computes that one alone (dvs_convex_up_bwd with the other
    pointer NULL) and it equals the one of the full backward bit for bit."""
    from deep_visual_slam_amd import raft
    flow, mask, cot = R.convex_case(3, 5, 7, 11)
    _, df, dm = run_convex_gpu(flow, mask, cot, 0.25, gpu_device)
    for k, want in ((0, df), (1, dm)):
        t = [flow.to(gpu_device), mask.to(gpu_device).contiguous(memory_format=CL)]
        t[k].requires_grad_(True)
        got, = torch.autograd.grad(raft.upsample_flow(t[0], t[1], 0.25), t[k], cot.to(gpu_device))
        assert torch.equal(bits(got.cpu()), bits(want))


def test_convex_upsampling_one_hot_mask(gpu_device):
    """One tap at +100 and the rest at -100: exp(-200) is 0 in fp32, the softmax is one-hot, the output is exactly 8 * flow of that
    tap (0 where the tap is outside the map) and dmask is exactly zero."""
    N, h, w = 2, 5, 7
    gen = torch.Generator().manual_seed(9)
    flow, cot = 3.0 * torch.randn(N, 2, h, w, generator=gen), torch.randn(N, 2, 8 * h, 8 * w, generator=gen)
    tap = torch.randint(0, 9, (N, 8, 8, h, w), generator=gen)                       # per output pixel
    mask = torch.full((N, 9, 8, 8, h, w), -100.0).scatter_(1, tap[:, None], 100.0).reshape(N, 576, h, w)
    out, df, dm = run_convex_gpu(flow, mask, cot, 1.0, gpu_device)
    padded = F.pad(8 * flow, (1, 1, 1, 1))
    taps = torch.stack([padded[:, :, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 2)       # [N,2,9,h,w]
    pick = tap[:, None, None].expand(N, 2, 1, 8, 8, h, w)
    want = taps[:, :, :, None, None].expand(N, 2, 9, 8, 8, h, w).gather(2, pick)[:, :, 0]                   # [N,2,8,8,h,w]
    want = want.permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * h, 8 * w)
    assert torch.equal(out, want)
    assert torch.equal(dm, torch.zeros_like(dm))
    _, df64, _ = R.run_convex(flow, mask, cot, 1.0, torch.float64)
    assert float((df.double() - df64).abs().max()) <= R.GRAD_TOL * float(df64.abs().max())


@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_convex_upsampling_constant_flow_and_borders(gpu_device, scale):
    """A constant flow comes back as 8 * flow within 2 ulp wherever all nine taps are inside the map; at border pixels the zero
    padding shows, and the result follows fp64 within the forward bound."""
    N, h, w = 2, 6, 9
    gen = torch.Generator().manual_seed(10)
    value = torch.tensor([1.2345678, -0.87654321])
    flow = value[None, :, None, None].expand(N, 2, h, w).contiguous()
    mask, cot = 4.0 * torch.randn(N, 576, h, w, generator=gen), torch.randn(N, 2, 8 * h, 8 * w, generator=gen)
    out, _, _ = run_convex_gpu(flow, mask, cot, scale, gpu_device)
    inner = out[:, :, 8:-8, 8:-8]
    want = (8 * value)[None, :, None, None]
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy())))
    assert bool(((inner - want).abs() <= 2 * ulp).all()), float(((inner - want).abs() / ulp).max())
    o64, _, _ = R.run_convex(flow, mask, cot, scale, torch.float64)
    border = torch.ones_like(out, dtype=torch.bool)
    border[:, :, 8:-8, 8:-8] = False
    assert float((o64 - want.double()).abs()[border].max()) > 0.1                   # the padding is visible there
    assert float((out.double() - o64).abs()[border].max()) <= 32 * EPS * 8 * float(flow.abs().max())


# ---- 3: the 1x1 route at the shapes that are new to it ----------------------------------------------------------------------------
POINTWISE = [(640, 128), (640, 256), (640, 384), (256, 576)]


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 16, 17)], ids=["b2_5x7", "b1_16x17"])
@pytest.mark.parametrize("K,Cout", POINTWISE, ids=["k%d_n%d" % p for p in POINTWISE])
def test_pointwise_convolutions_new_to_the_route(gpu_device, K, Cout, shape):
    """K = 5 * 128 with Cout in {128, 256, 384} (the stacked GRU filters) and 256 -> 576 (the mask head): y, dx, dW, db against fp64
    at the project's convolution tolerances."""
    from deep_visual_slam_amd import conv
    B, H, W = shape
    gen = torch.Generator().manual_seed(K + Cout + H)
    x, w, b = torch.randn(B, K, H, W, generator=gen), torch.randn(Cout, K, 1, 1, generator=gen) / np.sqrt(K), 0.1 * torch.randn(Cout, generator=gen)
    dy = torch.randn(B, Cout, H, W, generator=gen)
    r = [t.double().requires_grad_(True) for t in (x, w, b)]
    y64 = F.conv2d(r[0], r[1], r[2])
    g64 = torch.autograd.grad(y64, r, dy.double())
    d = [t.to(gpu_device).requires_grad_(True) for t in (x.contiguous(memory_format=CL), w.contiguous(memory_format=CL), b)]
    y = conv.conv2d(d[0], d[1], d[2])
    g = torch.autograd.grad(y, d, dy.to(gpu_device))
    U.check_rel("y", y, y64.detach())
    for name, got, want in zip(("d/x", "d/W", "d/b"), g, g64):
        U.check_rel(name, got, want)


# ---- 4: BasicEncoder ------------------------------------------------------------------------------------------------------------------
def make_encoder(norm, train, weights, dev, output_dim=128):
    from deep_visual_slam_amd import raft_encoder
    enc = raft_encoder.BasicEncoder(output_dim, norm)
    enc.load_state_dict(weights, strict=True)
    return enc.to(dev).train(train)


def check_stats(tag, module, ref, prefix=""):
    """The BatchNorm buffers a train-mode forward left behind against the fp64 restatement's: OUT_TOL of the buffer's max."""
    sd = module.state_dict()
    seen = 0
    for k, want in ref.items():
        if not k.startswith("stats/" + prefix):
            continue
        have = sd[k[len("stats/"):]].cpu()
        if k.endswith("num_batches_tracked"):
            assert int(have) == int(want), k
        else:
            U.check_rel(tag + " " + k, have, want.double())
        seen += 1
    return seen


ENC_IDS = ["%s_%s" % (n, "train" if t else "eval") for n, t in R.ENC_MODES]


@pytest.mark.parametrize("norm,train", R.ENC_MODES, ids=ENC_IDS)
def test_basic_encoder_forward(gpu_device, norm, train):
    """2 images at 40x56, as one tensor and (instance, none) as a list of two batches of one: the output within OUT_TOL of fp64;
    batch in train mode also leaves the running statistics and num_batches_tracked nn.BatchNorm2d leaves."""
    w = R.make_encoder_weights(128, norm, 21)
    x = torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(40)) * 2 - 1
    stats = {}
    with torch.no_grad():
        want = R.basic_encoder(R.cast(w, torch.float64), x.double(), norm, train, None, stats)
        enc = make_encoder(norm, train, w, gpu_device)
        xd = x.to(gpu_device)
        one = enc(xd)
    torch.cuda.synchronize()
    assert tuple(one.shape) == (2, 128, 5, 7)
    U.check_rel("%s tensor" % norm, one, want)
    if norm == "batch" and train:
        assert check_stats("stats", enc, {"stats/" + k: v for k, v in stats.items()}) == 3 * 15
    if norm == "batch":
        sd = enc.state_dict()
        assert all(torch.equal(sd[k], sd[k.replace(".downsample.1.", ".norm3.")]) for k in sd if ".downsample.1." in k)
    if not (norm == "batch" and train):                     # (batch statistics over two images are not those of one)
        with torch.no_grad():
            a, b = enc([xd[:1], xd[1:]])
            want2 = want if norm != "batch" else R.basic_encoder(R.cast(w, torch.float64), x.double(), norm, False)
        U.check_rel("%s list" % norm, torch.cat([a, b], 0), want2)


def check_zero_bias(tag, key, got, ref32, weight_grad64):
    b = max(3.0 * float(ref32.abs().max()), R.ulp_floor(float(weight_grad64.abs().max())))
    err = float(got.detach().double().cpu().abs().max())
    print("%s %s (zero-gradient bias): max |value| %.3e, bound %.3e" % (tag, key, err, b))
    assert err <= b, (tag, key, err, b)


ENC_CASES = [(n, t, s) for n, t in R.ENC_MODES for s in R.ENC_SIZES]
# no seed meets the margin condition (make_golden_raft_basic.py: ENC_SEEDS is None): a mask may flip, the relative-L2 rule applies
FLIP_CASES = ("instance_eval_24x40", "batch_train_24x40")


@pytest.mark.parametrize("norm,train,size", ENC_CASES, ids=["%s_%s_%dx%d" % (n, "train" if t else "eval", s[0], s[1]) for n, t, s in ENC_CASES])
def test_basic_encoder_gradients_elementwise(gpu_device, norm, train, size):
    """2 images whose features are 2x3 / 3x5, random cotangent: the gradients of the image and of every parameter within
    max(GRAD_TOL * max |ref|, bound) -- tests/test_raft_gpu.py's rule.  Well posed only when no ReLU mask can flip: the test first
    checks that the fp64 run's smallest relative ReLU margin is at least 16 x the largest relative pre-activation difference
    between the restatement's fp32 and fp64 runs (seeds: make_golden_raft_basic.py --search, recorded in the fixture).  For
    'instance' and 'batch' in train mode at 24x40 no seed qualifies (2 x 10^5 unit-scale ReLU inputs): there a mask may flip, and
    the case takes the end-to-end rule instead, per tensor a relative L2 error within max(GRAD_TOL, 3 e32) + sqrt(K) f with e32, K
    and f from the fixture."""
    rec = load_golden(FIXTURE)
    name = "%s_%s_%dx%d" % (norm, "train" if train else "eval", size[0], size[1])
    flip = name in FLIP_CASES
    assert ("encf/%s/seed" % name in rec) == flip and ("enc/" + name in rec) == (not flip), name
    seed = int(rec["encf/%s/seed" % name]) if flip else int(rec["enc/" + name][0])
    w, x, cot = R.enc_case(size, norm, seed)
    if not flip:
        margin, diff = R.encoder_margins(w, x, norm, train)
        print("margin %.3e, fp32-vs-fp64 pre-activation difference %.3e" % (margin, diff))
        assert margin >= 16 * diff, "seed does not qualify: run tests/golden/make_golden_raft_basic.py --search"
    r64, r32 = (R.run_encoder(w, x, cot, norm, dt, train) for dt in (torch.float64, torch.float32))
    enc = make_encoder(norm, train, w, gpu_device)
    xd = x.to(gpu_device).requires_grad_(True)
    out = enc(xd)
    grads = torch.autograd.grad(out, [xd] + list(enc.parameters()), cot.to(gpu_device))
    torch.cuda.synchronize()
    U.check_rel("out", out, r64["out"], extra=R.bound(r64["out"], r32["out"]))
    names = ["x"] + [k for k, _ in enc.named_parameters()]
    assert sorted(names[1:]) == sorted(k[2:] for k in r64 if k.startswith("d/") and k != "d/x")
    zero = R.zero_gradient_biases(norm, train)
    if flip:
        # the end-to-end rule: per tensor, relative L2 within max(GRAD_TOL, 3 e32) + sqrt(K) f
        K, f = int(rec["encf/%s/K" % name]), float(rec["encf/%s/f" % name])
        e32 = dict(zip((str(k) for k in rec["encf/%s/keys" % name]), rec["encf/%s/e32" % name]))
        assert sorted(e32) == sorted(names) and [str(k) for k in rec["encf/%s/zkeys" % name]] == zero
        print("K %d, f %.3e" % (K, f))
    for k, g in zip(names, grads):
        if k in zero:
            check_zero_bias(norm, k, g, r32["d/" + k], r64["d/" + k.replace(".bias", ".weight")])
        elif flip:
            err, b = R.rel_l2(g.cpu(), r64["d/" + k]), max(R.GRAD_TOL, 3.0 * float(e32[k])) + np.sqrt(K) * f
            print("d/%s: relative L2 error %.3e, bound %.3e (e32 %.3e)" % (k, err, b, float(e32[k])))
            assert err <= b, (k, err, b)
        else:
            U.check_rel("d/" + k, g, r64["d/" + k], extra=R.bound(r64["d/" + k], r32["d/" + k]))
    if norm == "batch" and train:
        assert check_stats("stats", enc, r64) == 3 * 15


# ---- 5: BasicUpdateBlock ------------------------------------------------------------------------------------------------------------
def make_block(weights, dev):
    from deep_visual_slam_amd import raft_update
    block = raft_update.BasicUpdateBlock()
    block.load_state_dict(weights, strict=True)
    return block.to(dev)


STEP_CASES = [("b2_5x7_nchw", 2, 5, 7, False), ("b1_16x17_cl", 1, 16, 17, True), ("b3_2x1_nchw", 3, 2, 1, False)]


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_basic_update_block_one_step(gpu_device, case):
    """net, the raw mask, delta_flow and the gradients of the four inputs and of every parameter: tests/test_raft_update_gpu.py's
    one-step tolerances, 2e-5 of the tensor's max on outputs, 1e-4 on gradients.  2x1: both windows are wider than the map."""
    name, B, H, W, corr_cl = case
    weights = R.make_update_weights(11 + H)
    x, cot = R.make_update_case(B, H, W, 12 + W)
    ref = R.run_update(weights, x, cot, torch.float64)
    block = make_block(weights, gpu_device)
    d = {k: v.to(gpu_device).requires_grad_(True) for k, v in x.items()}
    corr = d["corr"].contiguous(memory_format=CL) if corr_cl else d["corr"]
    net, mask, delta = block(d["net"], d["inp"], corr, d["flow"])
    assert tuple(mask.shape) == (B, 576, H, W) and mask.is_contiguous(memory_format=CL)
    loss = sum((o * c.to(gpu_device)).sum() for o, c in zip((net, mask, delta), cot))
    names = list(R.UPDATE_INPUTS) + [k for k, _ in block.named_parameters()]
    grads = torch.autograd.grad(loss, [d[k] for k in R.UPDATE_INPUTS] + list(block.parameters()))
    torch.cuda.synchronize()
    got = {"d/" + n: g for n, g in zip(names, grads)}
    got.update(net=net, mask=mask, delta=delta)
    assert sorted(got) == sorted(ref)
    for k in sorted(ref):
        U.check_rel(name + " " + k, got[k], ref[k])


def test_basic_update_block_hoists_both_context_terms(gpu_device):
    """One `inp` object, three calls: the two passes' context convolutions run once each, under autograd too; upsample=False
    skips the mask head; a changed inp or weight is noticed."""
    weights = R.make_update_weights(4)
    x, cot = R.make_update_case(1, 5, 7, 5)
    block = make_block(weights, gpu_device)
    calls = []
    inner = block._context_conv
    block._context_conv = lambda *a: calls.append(1) or inner(*a)
    d = {k: v.to(gpu_device) for k, v in x.items()}
    w64 = {k: v.double() for k, v in weights.items()}
    n64, m64, d64 = R.update_block(w64, *(x[k].double() for k in R.UPDATE_INPUTS))
    for _ in range(3):
        with torch.no_grad():
            net, mask, delta = block(d["net"], d["inp"], d["corr"], d["flow"], upsample=False)
        assert mask is None
        U.check_rel("net", net, n64)
        U.check_rel("delta", delta, d64)
    assert len(calls) == 2
    d["inp"].mul_(2)
    with torch.no_grad():
        block(d["net"], d["inp"], d["corr"], d["flow"])
    assert len(calls) == 4
    with torch.no_grad():
        block.gru.convz2.weight.mul_(0.5)
        block(d["net"], d["inp"], d["corr"], d["flow"])
    assert len(calls) == 6
    inp = d["inp"].requires_grad_(True)
    net = d["net"]
    for _ in range(3):
        net, mask, delta = block(net, inp, d["corr"], d["flow"])
    assert len(calls) == 8
    torch.autograd.grad(net.sum() + mask.sum(), [inp] + list(block.parameters()), allow_unused=True)
    block(d["net"], inp, d["corr"], d["flow"])
    assert len(calls) == 10                                  # the gradient's arrival dropped the entry


# ---- 6: RAFT end to end ------------------------------------------------------------------------------------------------------------
def make_raft(weights, dev, alternate, train):
    from deep_visual_slam_amd import raft
    model = raft.RAFT(SimpleNamespace(small=False, alternate_corr=alternate))
    model.load_state_dict(weights, strict=True)
    return model.to(dev).train(train)


def run_gpu_raft(model, im1, im2, cot, iters, init, dev):
    flows = model(im1.to(dev), im2.to(dev), iters=iters, flow_init=init.to(dev) if init is not None else None)
    low = model.flow_low
    loss = sum((f * c.to(dev)).sum() for f, c in zip(flows, cot))
    grads = torch.autograd.grad(loss, list(model.parameters()))
    torch.cuda.synchronize()
    res = {"d/" + k: g.cpu() for (k, _), g in zip(model.named_parameters(), grads)}
    for k in range(iters):
        res["low%d" % k], res["flow%d" % k] = low[k].cpu(), flows[k].detach().cpu()
    return res


G6_CASES = {"eval_noinit": (False, "noinit"), "train_init": (True, "init")}


@pytest.fixture(scope="module")
def raft_refs():
    """case -> (inputs, fp64 run, fp32 run) of the restatement: computed once, never modified."""
    out = {}
    for name, (train, case) in G6_CASES.items():
        w, im1, im2, cot, init = R.g6_case(case)
        it = R.G6["iters"]
        out[name] = ((w, im1, im2, cot, init), R.run_raft(w, im1, im2, cot, torch.float64, it, init, train),
                     R.run_raft(w, im1, im2, cot, torch.float32, it, init, train))
    return out


@pytest.mark.parametrize("alternate", [False, True], ids=["corr", "altcorr"])
@pytest.mark.parametrize("name", list(G6_CASES))
def test_raft_end_to_end(gpu_device, raft_refs, name, alternate):
    """B=2, 128x136 (features 16x17), iters=2; BatchNorm in eval mode without flow_init, in train mode with it.  Forward: every flow,
    low and full resolution, within max(OUT_TOL * max, bound); in train mode the BatchNorm buffers.  Gradients through both
    iterations: per parameter tensor the relative L2 error is held to max(GRAD_TOL, 3 e32) + sqrt(K) f with e32, K, f from the
    fixture (tests/test_raft_gpu.py's rule for a model with millions of ReLU inputs); zero-gradient biases follow their own rule.
    Then, in the deterministic mode: last_only and test_mode equal the last element of the full run bit for bit, and a train()
    model under freeze_bn() computes what the eval() model computes and leaves its buffers alone.
    The differentiated pass runs in the deterministic mode too (no float atomics in the convolutions' split-K and statistics
    epilogues), so which ReLU masks differ from the fp64 run's does not change from run to run; f is the largest effect of one
    forced flip over twelve (tests/golden/make_golden_raft_basic.py: g6_numbers)."""
    train, _ = G6_CASES[name]
    rec = load_golden(FIXTURE)
    assert [int(v) for v in rec["g6/config"]] == [R.G6[k] for k in ("image_seed", "weight_seed", "cot_seed", "init_seed")]
    (w, im1, im2, cot, init), r64, r32 = raft_refs[name]
    it = R.G6["iters"]
    model = make_raft(w, gpu_device, alternate, train)
    from deep_visual_slam_amd import _lib
    was = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        got = run_gpu_raft(model, im1, im2, cot, it, init, gpu_device)
    finally:
        _lib.set_deterministic(was)
    for k in range(it):
        for key in ("low%d" % k, "flow%d" % k):
            U.check_rel(name + " " + key, got[key], r64[key], extra=R.bound(r64[key], r32[key]))
    if train:
        assert check_stats("stats", model, r64) == 3 * 15
    K, f = int(rec["g6/%s/K" % name]), float(rec["g6/%s/f" % name])
    keys, zero = [str(k) for k in rec["g6/%s/keys" % name]], [str(k) for k in rec["g6/%s/zkeys" % name]]
    assert sorted(keys) == sorted(k for k, _ in model.named_parameters())
    print("K %d, f %.3e" % (K, f))
    for key, e32 in zip(keys, rec["g6/%s/e32" % name]):
        if key in zero:
            check_zero_bias(name, key, got["d/" + key], torch.tensor(float(rec["g6/%s/zb32" % name][zero.index(key)])),
                            r64["d/" + key.replace(".bias", ".weight")])
            continue
        err, b = R.rel_l2(got["d/" + key], r64["d/" + key]), max(R.GRAD_TOL, 3.0 * float(e32)) + np.sqrt(K) * f
        print("%s d/%s: relative L2 error %.3e, bound %.3e (e32 %.3e)" % (name, key, err, b, float(e32)))
        assert err <= b, (key, err, b)
    # forward passes are compared bit for bit: the deterministic mode again
    _lib.set_deterministic(True)
    try:
        with torch.no_grad():
            args = (im1.to(gpu_device), im2.to(gpu_device))
            kw = dict(iters=it, flow_init=init.to(gpu_device) if init is not None else None)
            every = model(*args, **kw)
            low = [t.clone() for t in model.flow_low]
            last = model(*args, last_only=True, **kw)
            flow_low, flow_up = model(*args, test_mode=True, **kw)
            if train:
                model.freeze_bn()
                before = {k: v.clone() for k, v in model.state_dict().items()}
                frozen = model(*args, **kw)
                after = model.state_dict()
                thawed = make_raft(w, gpu_device, alternate, False)
                thawed.load_state_dict(before)
                same = thawed(*args, **kw)
    finally:
        _lib.set_deterministic(was)
    assert len(last) == 1 and len(every) == it
    assert torch.equal(bits(last[0]), bits(every[-1]))
    assert torch.equal(bits(flow_up), bits(every[-1])) and torch.equal(bits(flow_low), bits(low[-1]))
    if train:
        assert model.training and all(torch.equal(before[k], after[k]) for k in before)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(frozen, same))


@pytest.mark.parametrize("alternate", [False, True], ids=["corr", "altcorr"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_reference_fixture_through_the_gpu_model(gpu_device, mode, alternate):
    """The reference's recorded fp32 flows (B=2, 128x136, iters=2) with the fixture's weights, in both BatchNorm modes and both
    correlation forms: within max(OUT_TOL * max, 3 x the recorded reference-fp32-vs-restatement-fp64 error); in train mode the
    buffers the reference's forward left behind."""
    rec = load_golden(FIXTURE)
    B, H, W, iters, seed = (int(v) for v in rec["meta/config"])
    w = R.make_weights(seed)
    for k, v in w.items():
        assert np.allclose(R.checksum(v), rec["w/cs/" + k], rtol=1e-12, atol=0), "make_weights changed: " + k
    im1, im2 = (torch.from_numpy(rec["in/image%d" % i]).float() / 255 for i in (1, 2))
    model = make_raft(w, gpu_device, alternate, mode == "train")
    with torch.no_grad():
        flows = model(im1.to(gpu_device), im2.to(gpu_device), iters=iters)
    for k in range(iters):
        for name, have in (("low%d" % k, model.flow_low[k]), ("flow%d" % k, flows[k])):
            want = rec["ref32/%s/%s" % (mode, name)]
            U.check_rel("fixture %s %s" % (mode, name), have, torch.from_numpy(want).double(),
                        extra=max(3.0 * float(rec["err/%s/%s" % (mode, name)]), R.ulp_floor(float(np.abs(want).max()))))
    if mode == "train":
        ref = {k[len("ref32/train/"):]: torch.from_numpy(np.asarray(v)) for k, v in rec.items() if k.startswith("ref32/train/stats/")}
        assert check_stats("fixture stats", model, ref) == 3 * 15


def test_context_terms_run_once_per_forward(gpu_device, raft_refs):
    (w, im1, im2, cot, init), _, _ = raft_refs["eval_noinit"]
    model = make_raft(w, gpu_device, False, False)
    calls = []
    inner = model.update_block._context_conv
    model.update_block._context_conv = lambda *a: calls.append(1) or inner(*a)
    flows = model(im1.to(gpu_device), im2.to(gpu_device), iters=3)
    assert len(flows) == 3 and len(calls) == 2                  # one per pass of the SepConvGRU
    with torch.no_grad():
        up = model(im1.to(gpu_device), im2.to(gpu_device), iters=3, upsample=False)
    assert len(calls) == 4 and len(up) == 3 and tuple(up[0].shape) == tuple(flows[0].shape)
