"""SmallRAFT end to end on the GPU (raft.py, raft_encoder.py, csrc/inorm.hip, csrc/upflow.hip) against tests/raft_ref.py in fp64:
the instance-norm entries alone through the C ABI, their numerical edges, upflow8 alone, the encoders' outputs and gradients, the
whole model, the fixture the reference's own SmallRAFT produced, and the hoisted context convolution."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import raft_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
CL = torch.channels_last
FIXTURE = "raft_small_b1_128x136.npz"
T = 1024        # pixels of one slice of csrc/inorm.hip (dvs_inorm_slice_pixels()): one workgroup's share of an image
FLAGS = {"norm_relu": (1, 1, 0), "norm": (1, 0, 0), "norm_relu_res": (1, 1, 1), "relu_res": (0, 1, 1)}     # norm, relu, residual


# ---- 1: the instance-norm kernels alone, through the C ABI --------------------------------------------------------------------
def run_inorm(y, res, dout, norm, relu, dev, seed_fill=float("nan")):
    """Forward and backward entry on NHWC CPU tensors [N,HW,C]; every output buffer starts as NaN.  CPU tensors back."""
    from deep_visual_slam_amd import _lib
    lib = _lib.lib()
    N, HW, Cn = y.shape
    d = lambda t: t.to(dev).contiguous() if t is not None else None
    yd, rd, gd = d(y), d(res), d(dout)
    new = lambda *s: torch.full(s, seed_fill, device=dev)
    out, dy = new(N, HW, Cn), new(N, HW, Cn)
    dres = new(N, HW, Cn) if res is not None else None
    table = new(N, 2, Cn) if norm else None
    nbytes = int(lib.dvs_inorm_workspace(N, HW, Cn))
    assert nbytes == N * -(-HW // T) * 2 * Cn * 4
    ws = torch.full((nbytes // 4,), seed_fill, device=dev) if norm else None
    p = lambda t: t.data_ptr() if t is not None else None
    _lib.check(lib.dvs_inorm_fwd(p(yd), p(rd), p(out), p(table), p(ws), nbytes if norm else 0, N, HW, Cn, norm, relu, _lib.stream()),
               "dvs_inorm_fwd")
    _lib.check(lib.dvs_inorm_bwd(p(gd), p(yd), p(out) if res is not None else None, p(table), p(dy), p(dres), p(ws),
                                 nbytes if norm else 0, N, HW, Cn, norm, relu, _lib.stream()), "dvs_inorm_bwd")
    torch.cuda.synchronize()
    got = {"out": out.cpu(), "dy": dy.cpu()}
    if norm:
        got["mean"], got["invstd"] = table[:, 0].cpu(), table[:, 1].cpu()
    if res is not None:
        got["dres"] = dres.cpu()
    return got


def inorm_forward_refs(y, res, norm, relu):
    """{name: (fp64, fp32)} of the forward: F.instance_norm / F.relu on the CPU in NCHW, brought back to [N,HW,C]."""
    refs = {}
    for dt in (torch.float64, torch.float32):
        x = y.to(dt).permute(0, 2, 1)[:, :, :, None]                        # [N,C,HW,1]
        z = F.instance_norm(x, eps=R.EPS) if norm else x
        z = F.relu(z) if relu else z
        if res is not None:
            z = F.relu(res.to(dt).permute(0, 2, 1)[:, :, :, None] + z)
        o = {"out": z[:, :, :, 0].permute(0, 2, 1)}
        if norm:
            yy = y.to(dt)
            o["mean"] = yy.mean(1)
            o["invstd"] = (yy.var(1, unbiased=False) + R.EPS).rsqrt()
        for k, v in o.items():
            refs.setdefault(k, []).append(v)
    return refs


def inorm_backward_refs(y, res, dout, got, norm, relu):
    """The issue's backward formulas in fp64 and fp32 on what the KERNEL's forward left: the masks [z > 0] and [out > 0] come from
    its output, mean and invstd from its table, so the forward's rounding is never charged to the backward."""
    refs = {}
    for dt in (torch.float64, torch.float32):
        yy, g = y.to(dt), dout.to(dt)
        if res is not None:
            g = g * (got["out"] > 0).to(dt)
        if norm:
            mean, invstd = got["mean"].to(dt)[:, None], got["invstd"].to(dt)[:, None]
            xhat = (yy - mean) * invstd
        if relu:
            if res is not None:             # out = relu(res + relu(z)): the kernel's z mask is not in its output; recompute it as it does
                zmask = ((y - got["mean"][:, None]) * got["invstd"][:, None] > 0) if norm else (y > 0)
            else:
                zmask = got["out"] > 0
            du = g * zmask.to(dt)
        else:
            du = g
        dy = invstd * (du - du.mean(1, keepdim=True) - xhat * (du * xhat).mean(1, keepdim=True)) if norm else du
        o = {"dy": dy}
        if res is not None:
            o["dres"] = g
        for k, v in o.items():
            refs.setdefault(k, []).append(v)
    return refs


def inorm_operands(N, HW, Cn, residual, seed, shift=0.0):
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(N, HW, Cn, generator=gen) * (0.5 + torch.rand(1, 1, Cn, generator=gen)) + torch.randn(1, 1, Cn, generator=gen) + shift
    res = torch.randn(N, HW, Cn, generator=gen) if residual else None
    return y, res, torch.randn(N, HW, Cn, generator=gen)


def check_inorm(tag, y, res, dout, norm, relu, dev, forward_only=False):
    got = run_inorm(y, res, dout, norm, relu, dev)
    again = run_inorm(y, res, dout, norm, relu, dev)
    for k in got:
        assert torch.isfinite(got[k]).all(), (tag, k, "not every element was written, or not finite")
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), "%s %s differs between two runs" % (tag, k)
    refs = inorm_forward_refs(y, res, norm, relu)
    if not forward_only:
        refs.update(inorm_backward_refs(y, res, dout, got, norm, relu))
    for k, (r64, r32) in refs.items():
        err, b = float((got[k].double() - r64).abs().max()), R.bound(r64, r32)
        print("%s %s: max |err| %.3e, bound %.3e" % (tag, k, err, b))
        assert err <= b, (tag, k, err, b)
    return got


INORM_CASES = [(Cn, N, HW, f) for Cn in (8, 24, 32, 96) for N in (1, 3) for HW in (2, T - 1, T, T + 1, 2 * T + 77) for f in FLAGS]


@pytest.mark.parametrize("Cn,N,HW,flags", INORM_CASES, ids=["c%d_n%d_hw%d_%s" % c for c in INORM_CASES])
def test_inorm_kernels_against_fp64(gpu_device, Cn, N, HW, flags):
    """Forward: out and the (mean, invstd) table against fp64 under `bound`, the fp32 side F.instance_norm / F.relu on the CPU.
    Backward: the fp64 formulas on the kernel's own masks and table.  Two runs agree bit for bit; NaN-filled buffers end finite."""
    norm, relu, residual = FLAGS[flags]
    y, res, dout = inorm_operands(N, HW, Cn, residual, seed=Cn * 100003 + HW * 7 + N)
    check_inorm("C%d N%d HW%d %s" % (Cn, N, HW, flags), y, res, dout, norm, relu, gpu_device)


# ---- 2: edges --------------------------------------------------------------------------------------------------------------------
def test_inorm_constant_channel(gpu_device):
    """Channels that are constant over an image (var = 0): the normalised value is exactly 0 and finite, dy is finite."""
    N, HW, Cn = 2, 2 * T + 5, 24
    y, _, dout = inorm_operands(N, HW, Cn, False, seed=5)
    y[0, :, 3], y[1, :, 8], y[0, :, 20], y[1, :, 21] = 0.1, -7.3, 0.0, 1e6
    got = run_inorm(y, None, dout, 1, 0, gpu_device)
    for n, c in ((0, 3), (1, 8), (0, 20), (1, 21)):
        assert torch.equal(got["out"][n, :, c], torch.zeros(HW)), (n, c, got["out"][n, :, c].abs().max())
        assert float(got["mean"][n, c]) == float(y[n, 0, c])
    for k in got:
        assert torch.isfinite(got[k]).all(), k
    got = run_inorm(y, None, dout, 1, 1, gpu_device)
    assert torch.equal(got["out"][0, :, 3], torch.zeros(HW)) and torch.isfinite(got["dy"]).all()


def test_inorm_mean_100_std(gpu_device):
    """mean = 100 std: the forward stays within `bound` (a sum(x^2) / n - mean^2 variance is off by about 1e-3 here)."""
    _, _, dout = inorm_operands(2, 64 * 68, 32, False, seed=11)
    y = torch.randn(2, 64 * 68, 32, generator=torch.Generator().manual_seed(12)) + 100.0
    check_inorm("mean=100std", y, None, dout, 1, 1, gpu_device, forward_only=True)
    check_inorm("mean=100std norm only", y, None, dout, 1, 0, gpu_device)


def test_inorm_no_leak_between_images(gpu_device):
    """One image all zeros beside a normal one: each image's results are, bit for bit, those of the N = 1 call on it."""
    HW, Cn = T + 300, 96
    y, res, dout = inorm_operands(2, HW, Cn, True, seed=13)
    y[0] = 0
    both = run_inorm(y, res, dout, 1, 1, gpu_device)
    for n in (0, 1):
        one = run_inorm(y[n:n + 1], res[n:n + 1], dout[n:n + 1], 1, 1, gpu_device)
        for k in both:
            assert torch.equal(both[k][n:n + 1].view(torch.int32), one[k].view(torch.int32)), (n, k)
    assert torch.equal(both["mean"][0], torch.zeros(Cn))


def test_inorm_two_pixels(gpu_device):
    """HW = 2, the smallest map torch accepts: xhat = +-1 up to eps."""
    y = torch.tensor([[[1.0, -2.0, 3.0, 0.5, 4, 5, 6, 7], [3.0, -2.5, 3.0, 1.5, 0, 1, 2, 9]]])
    got = check_inorm("HW=2", y, None, torch.ones_like(y), 1, 0, gpu_device)
    assert float(got["out"][0, 0, 0]) == pytest.approx(-1.0, abs=1e-4) and float(got["out"][0, 0, 2]) == 0.0


# ---- 3: upflow8 alone ---------------------------------------------------------------------------------------------------------
def run_upflow(flow, dout, nchw, dev):
    from deep_visual_slam_amd import raft
    f = flow.to(dev)
    f = (f.contiguous() if nchw else f.contiguous(memory_format=CL)).requires_grad_(True)
    if not nchw and f.shape[2] * f.shape[3] > 1:
        assert not f.is_contiguous()
    up = raft.upflow8(f)
    assert up.is_contiguous()
    g, = torch.autograd.grad(up, f, dout.to(dev))
    torch.cuda.synchronize()
    return up.detach().cpu(), g.cpu()


UP_CASES = [(h, w, N, nchw) for (h, w) in ((1, 1), (1, 5), (2, 2), (5, 7), (16, 17)) for N in (1, 3) for nchw in (1, 0)]


@pytest.mark.parametrize("h,w,N,nchw", UP_CASES, ids=["%dx%d_n%d_%s" % (h, w, N, "nchw" if p else "nhwc") for h, w, N, p in UP_CASES])
def test_upflow8_against_fp64(gpu_device, h, w, N, nchw):
    """Forward and backward against F.interpolate in fp64 under `bound` (fp32 side: F.interpolate in fp32 on the CPU); the adjoint
    identity <up(f), g> = <f, up^T(g)> accumulated in fp64 from the kernel outputs within the sum of the two bounds (each bound
    times the l1 norm of the vector it is paired with); two runs agree bit for bit, backward included."""
    gen = torch.Generator().manual_seed(1000 * h + 10 * w + N)
    flow, dout = 3.0 * torch.randn(N, 2, h, w, generator=gen), torch.randn(N, 2, 8 * h, 8 * w, generator=gen)
    up, g = run_upflow(flow, dout, nchw, gpu_device)
    up2, g2 = run_upflow(flow, dout, nchw, gpu_device)
    assert torch.equal(up.view(torch.int32), up2.view(torch.int32)) and torch.equal(g.view(torch.int32), g2.view(torch.int32))
    ref = {}
    for dt in (torch.float64, torch.float32):
        f = flow.to(dt).requires_grad_(True)
        u = R.upflow8(f)
        ref[dt] = (u.detach(), torch.autograd.grad(u, f, dout.to(dt))[0])
    bounds = []
    for k, name, have in ((0, "up", up), (1, "dflow", g)):
        r64, r32 = ref[torch.float64][k], ref[torch.float32][k]
        assert have.shape == r64.shape and torch.isfinite(have).all()
        err, b = float((have.double() - r64).abs().max()), R.bound(r64, r32)
        print("%dx%d N%d nchw%d %s: max |err| %.3e, bound %.3e" % (h, w, N, nchw, name, err, b))
        assert err <= b, (name, err, b)
        bounds.append(b)
    lhs, rhs = float((up.double() * dout.double()).sum()), float((flow.double() * g.double()).sum())
    slack = bounds[0] * float(dout.double().abs().sum()) + bounds[1] * float(flow.double().abs().sum())
    print("adjoint: %.12e vs %.12e, slack %.3e" % (lhs, rhs, slack))
    assert abs(lhs - rhs) <= slack


# ---- 4: SmallEncoder forward ---------------------------------------------------------------------------------------------------
def make_encoder(norm, weights, dev, output_dim=128):
    from deep_visual_slam_amd import raft_encoder
    enc = raft_encoder.SmallEncoder(output_dim, norm)
    enc.load_state_dict(weights)
    return enc.to(dev)


@pytest.fixture(scope="module")
def encoder_weights():
    return R.make_encoder_weights(128, 21)


@pytest.mark.parametrize("size", [(40, 56), (128, 136)], ids=["40x56", "128x136"])
@pytest.mark.parametrize("norm", ["instance", "none"])
def test_encoder_forward(gpu_device, encoder_weights, norm, size):
    """2 images, as a list of two batches of one and as one tensor: the output within OUT_TOL (2e-5 of the max) of fp64."""
    gen = torch.Generator().manual_seed(size[0])
    x = torch.rand(2, 3, *size, generator=gen) * 2 - 1
    with torch.no_grad():
        want = R.small_encoder({k: v.double() for k, v in encoder_weights.items()}, x.double(), norm)
        enc = make_encoder(norm, encoder_weights, gpu_device)
        xd = x.to(gpu_device)
        one = enc(xd)
        a, b = enc([xd[:1], xd[1:]])
    torch.cuda.synchronize()
    assert tuple(a.shape) == (1, 128, size[0] // 8, size[1] // 8)
    R.U.check_rel("%s tensor" % norm, one, want)
    R.U.check_rel("%s list" % norm, torch.cat([a, b], 0), want)


# ---- 5: SmallEncoder gradients, element-wise, where that is well posed ---------------------------------------------------------
# seeds: tests/golden/make_golden_raft.py --search (the first seed per case that meets the margin condition checked below)
G5_SEEDS = {((16, 24), "instance"): 19, ((16, 24), "none"): 1, ((24, 40), "instance"): 2424, ((24, 40), "none"): 35}
# The conv biases in front of an instance norm: their gradients are mathematically zero (fp64 gives ~1e-17, fp32 rounding noise).
# The issue lists 20 of them; conv1.bias feeds the first instance norm and is the 21st of the same kind, so it is judged alike.
ZERO_GRADIENT_BIASES = ["conv1.bias"] + ["layer%d.%d.conv%d.bias" % (i, j, k) for i in (1, 2, 3) for j in (0, 1) for k in (1, 2, 3)] \
    + ["layer2.0.downsample.0.bias", "layer3.0.downsample.0.bias"]


def check_zero_bias(tag, key, got, ref32, weight_grad64):
    b = max(3.0 * float(ref32.abs().max()), R.ulp_floor(float(weight_grad64.abs().max())))
    err = float(got.detach().double().cpu().abs().max())
    print("%s %s (zero-gradient bias): max |value| %.3e, bound %.3e" % (tag, key, err, b))
    assert err <= b, (tag, key, err, b)


@pytest.mark.parametrize("size,norm", R.G5_CASES, ids=["%dx%d_%s" % (s + (n,)) for s, n in R.G5_CASES])
def test_encoder_gradients_elementwise(gpu_device, size, norm):
    """2 images whose features are 2x3 / 3x5, random cotangent: the gradients of the image and of every parameter within
    max(GRAD_TOL * max |ref|, bound).  Well posed only when no ReLU mask can flip: the test first checks that the fp64 run's
    smallest relative ReLU margin is at least 16 x the largest relative pre-activation difference between the restatement's fp32
    and fp64 runs."""
    w, x, cot = R.g5_case(size, norm, G5_SEEDS[(size, norm)])
    margin, diff = R.encoder_margins(w, x, norm)
    print("margin %.3e, fp32-vs-fp64 pre-activation difference %.3e" % (margin, diff))
    assert margin >= 16 * diff, "seed does not qualify: run tests/golden/make_golden_raft.py --search"
    r64, r32 = R.run_encoder(w, x, cot, norm, torch.float64), R.run_encoder(w, x, cot, norm, torch.float32)
    enc = make_encoder(norm, w, gpu_device)
    xd = x.to(gpu_device).requires_grad_(True)
    out = enc(xd)
    grads = torch.autograd.grad(out, [xd] + list(enc.parameters()), cot.to(gpu_device))
    torch.cuda.synchronize()
    R.U.check_rel("out", out, r64["out"], extra=R.bound(r64["out"], r32["out"]))
    names = ["x"] + [k for k, _ in enc.named_parameters()]
    assert names[1:] == list(w)
    for k, g in zip(names, grads):
        if norm == "instance" and k in ZERO_GRADIENT_BIASES:
            check_zero_bias(norm, k, g, r32["d/" + k], r64["d/" + k.replace(".bias", ".weight")])
        else:
            R.U.check_rel("d/" + k, g, r64["d/" + k], extra=R.bound(r64["d/" + k], r32["d/" + k]))


# ---- 6: SmallRAFT end to end ------------------------------------------------------------------------------------------------------
def make_raft(weights, dev, alternate):
    from deep_visual_slam_amd import raft
    model = raft.SmallRAFT(SimpleNamespace(alternate_corr=alternate))
    model.load_state_dict(weights, strict=True)
    return model.to(dev)


def run_gpu_raft(model, im1, im2, cot, iters, init, dev):
    for p in model.parameters():
        p.grad = None
    flows = model(im1.to(dev), im2.to(dev), iters=iters, flow_init=init.to(dev) if init is not None else None)
    low = model.flow_low
    loss = sum((f * c.to(dev)).sum() for f, c in zip(flows, cot))
    grads = torch.autograd.grad(loss, list(model.parameters()))
    torch.cuda.synchronize()
    res = {"d/" + k: g.cpu() for (k, _), g in zip(model.named_parameters(), grads)}
    for k in range(iters):
        res["low%d" % k], res["flow%d" % k] = low[k].cpu(), flows[k].detach().cpu()
    return res


@pytest.fixture(scope="module")
def raft_refs():
    """case -> (inputs, fp64 run, fp32 run) of the restatement: computed once, never modified."""
    out = {}
    for case in ("noinit", "init"):
        w, im1, im2, cot, init = R.g6_case(case)
        it = R.G6["iters"]
        out[case] = ((w, im1, im2, cot, init), R.run_raft(w, im1, im2, cot, torch.float64, it, init),
                     R.run_raft(w, im1, im2, cot, torch.float32, it, init))
    return out


def check_flows(tag, got, r64, r32, iters):
    for k in range(iters):
        for name in ("low%d" % k, "flow%d" % k):
            R.U.check_rel(tag + " " + name, got[name], r64[name], extra=R.bound(r64[name], r32[name]))


@pytest.mark.parametrize("alternate", [False, True], ids=["corr", "altcorr"])
@pytest.mark.parametrize("case", ["noinit", "init"])
def test_small_raft_end_to_end(gpu_device, raft_refs, case, alternate):
    """B=2, 128x136 (features 16x17), iters=3.  Forward: every flow, low and full resolution, within max(OUT_TOL * max, bound);
    last_only=True equals the last element bit for bit.  Gradients: this size has millions of ReLU inputs, so per parameter tensor
    the relative L2 error is held to max(GRAD_TOL, 3 e32) + sqrt(K) f with e32, K, f from the fixture (make_golden_raft.py); the
    zero-gradient biases of fnet follow their own rule."""
    rec = load_golden(FIXTURE)
    assert [int(v) for v in rec["g6/config"]] == [R.G6[k] for k in ("image_seed", "weight_seed", "cot_seed", "init_seed")]
    (w, im1, im2, cot, init), r64, r32 = raft_refs[case]
    it = R.G6["iters"]
    model = make_raft(w, gpu_device, alternate)
    got = run_gpu_raft(model, im1, im2, cot, it, init, gpu_device)
    check_flows(case, got, r64, r32, it)
    # two forward passes are compared, so the convolutions run in the deterministic mode (no split-K atomics) for them
    from deep_visual_slam_amd import _lib
    was = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        with torch.no_grad():
            args = (im1.to(gpu_device), im2.to(gpu_device))
            kw = dict(iters=it, flow_init=init.to(gpu_device) if init is not None else None)
            last = model(*args, last_only=True, **kw)
            every = model(*args, **kw)
    finally:
        _lib.set_deterministic(was)
    assert len(last) == 1 and len(every) == it
    assert torch.equal(last[0].view(torch.int32), every[-1].view(torch.int32))
    K, f = int(rec["g6/%s/K" % case]), float(rec["g6/%s/f" % case])
    keys = [str(k) for k in rec["meta/keys"]]
    zero = R.zero_gradient_biases("fnet.")
    print("K %d, f %.3e" % (K, f))
    for key, e32 in zip(keys, rec["g6/%s/e32" % case]):
        if key in zero:
            check_zero_bias(case, key, got["d/" + key], torch.tensor(float(rec["g6/%s/zb32" % case][zero.index(key)])),
                            r64["d/" + key.replace(".bias", ".weight")])
            continue
        err, b = R.rel_l2(got["d/" + key], r64["d/" + key]), max(R.GRAD_TOL, 3.0 * float(e32)) + np.sqrt(K) * f
        print("%s d/%s: relative L2 error %.3e, bound %.3e (e32 %.3e)" % (case, key, err, b, float(e32)))
        assert err <= b, (key, err, b)


# ---- 7: the fixture the reference produced -----------------------------------------------------------------------------------
def test_reference_fixture_through_the_gpu_model(gpu_device):
    """The reference's recorded fp32 flows (B=1, 128x136, iters=2) with the fixture's weights: within max(OUT_TOL * max, 3 x the
    recorded reference-fp32-vs-restatement-fp64 error)."""
    rec = load_golden(FIXTURE)
    B, H, W, iters, seed = (int(v) for v in rec["meta/config"])
    w = R.make_weights(seed)
    for k, v in w.items():
        assert np.allclose(R.checksum(v), rec["w/cs/" + k], rtol=1e-12, atol=0), "make_weights changed: " + k
    im1, im2 = (torch.from_numpy(rec["in/image%d" % i]).float() / 255 for i in (1, 2))
    model = make_raft(w, gpu_device, False)
    with torch.no_grad():
        flows = model(im1.to(gpu_device), im2.to(gpu_device), iters=iters)
    for k in range(iters):
        for name, have in (("low%d" % k, model.flow_low[k]), ("flow%d" % k, flows[k])):
            R.U.check_rel("fixture " + name, have, torch.from_numpy(rec["ref32/" + name]).double(),
                          extra=max(3.0 * float(rec["err/" + name]), R.ulp_floor(float(np.abs(rec["ref32/" + name]).max()))))


# ---- 8: the hoist ----------------------------------------------------------------------------------------------------------------
def test_context_convolution_runs_once_per_forward(gpu_device, raft_refs):
    (w, im1, im2, cot, init), _, _ = raft_refs["noinit"]
    model = make_raft(w, gpu_device, False)
    calls = []
    inner = model.update_block._context_conv
    model.update_block._context_conv = lambda *a: calls.append(1) or inner(*a)
    flows = model(im1.to(gpu_device), im2.to(gpu_device), iters=3)
    assert len(flows) == 3 and len(calls) == 1
    with torch.no_grad():
        model(im1.to(gpu_device), im2.to(gpu_device), iters=3)
    assert len(calls) == 2
