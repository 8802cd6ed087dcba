"""Full-size RAFT, restated (model/raft/core/raft.py:122-244, extractor.py:6-56 and 118-192, update.py:33-60 and 79-136) as functions
over a dict of weights keyed by the state-dict names, on tests/raft_ref.py's helpers.

Plain torch on the CPU (or any device), one function for every precision: fp64 tensors give the truth, fp32 tensors the error that
fp32 arithmetic of this formulation makes on the same inputs.  The update block is the CONCATENATED form -- F.conv2d with the full
(1,5) / (5,1) filters over cat[h, inp, motion] -- so it shares nothing with the split, shift-stacked implementation under test;
`sep_conv_gru_split` restates that implementation's algebra for the CPU test that compares the two in fp64.  The convex upsampling
is written from its index map (a gather of nine shifted copies), not with F.unfold.  BatchNorm is written out, so that the fp64
run also yields the running statistics a train-mode forward leaves behind.
"""
import math

import torch
import torch.nn.functional as F

import corr_ref
import raft_ref as S
from raft_ref import GRAD_TOL, OUT_TOL, Relus, bound, checksum, coords_grid, rel_l2, sub, ulp_floor  # noqa: F401  (the same rules)

HIDDEN, CONTEXT, LEVELS, RADIUS = 128, 128, 4, 4
PLANES = LEVELS * (2 * RADIUS + 1) ** 2          # 324
EPS, MOMENTUM = 1e-5, 0.1
LAYERS = ((64, 1), (96, 2), (128, 2))
MASK_SCALE = 0.25
BN_FIELDS = (("weight", None), ("bias", None), ("running_mean", None), ("running_var", None), ("num_batches_tracked", ()))


def _relus(r):
    return r if r is not None else Relus()


def _relu(r, x, name):
    """Relus.relu on contiguous memory (a convolution may hand back another layout, and Relus forces a mask through a flat view)."""
    return r.relu(x.contiguous(), name)


# ---- the new kernels' functions -------------------------------------------------------------------------------------------------
def shift_stack(x, axis):
    """[B,5C,H,W]: channel t*C + c is x[:, c] read at offset t - 2 along W (axis 0) or H (axis 1), 0 outside.  By indexing."""
    B, C, H, W = x.shape
    out = x.new_zeros(B, 5, C, H, W)
    for t in range(5):
        d = t - 2
        if axis == 0:
            lo, hi = max(0, -d), min(W, W - d)
            if lo < hi:
                out[:, t, :, :, lo:hi] = x[:, :, :, lo + d:hi + d]
        else:
            lo, hi = max(0, -d), min(H, H - d)
            if lo < hi:
                out[:, t, :, lo:hi, :] = x[:, :, lo + d:hi + d, :]
    return out.reshape(B, 5 * C, H, W)


def stacked_filter(weight):
    """[Cout, 5*Cin, 1, 1] over shift_stack of a [Cout,Cin,1,5] (axis 0) or [Cout,Cin,5,1] (axis 1) filter."""
    co, ci, kh, kw = weight.shape
    taps = weight.reshape(co, ci, 5)                   # one of kh, kw is 1
    return taps.permute(0, 2, 1).reshape(co, 5 * ci, 1, 1)


def upsample_flow(flow, mask, mask_scale=1.0):
    """out[n,ch,8y+i,8x+j] = sum_k softmax_k(mask_scale * mask[n, k*64+i*8+j, y, x]) * 8 * flow[n,ch,y+ky-1,x+kx-1], zeros outside."""
    N, _, h, w = flow.shape
    p = torch.softmax(mask_scale * mask.reshape(N, 9, 8, 8, h, w), dim=1)
    padded = F.pad(8 * flow, (1, 1, 1, 1))
    taps = torch.stack([padded[:, :, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 2)       # [N,2,9,h,w]
    up = (p[:, None] * taps[:, :, :, None, None]).sum(2)                                                   # [N,2,8,8,h,w]
    return up.permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * h, 8 * w)


# ---- BatchNorm, written out -------------------------------------------------------------------------------------------------------
def batch_norm(y, w, prefix, train, new_stats=None):
    """nn.BatchNorm2d(C) with the tensors w[prefix + ...]; train: batch statistics (biased variance), and new_stats (a dict)
    receives the running statistics one forward call leaves: (1 - m) * old + m * (mean, unbiased variance), count + 1."""
    g, b = w[prefix + "weight"], w[prefix + "bias"]
    if train:
        mean = y.mean((0, 2, 3))
        var = ((y - mean[None, :, None, None]) ** 2).mean((0, 2, 3))
        if new_stats is not None:
            n = y.numel() // y.shape[1]
            with torch.no_grad():
                new_stats[prefix + "running_mean"] = (1 - MOMENTUM) * w[prefix + "running_mean"].to(y.dtype) + MOMENTUM * mean
                new_stats[prefix + "running_var"] = (1 - MOMENTUM) * w[prefix + "running_var"].to(y.dtype) + MOMENTUM * var * n / (n - 1)
                new_stats[prefix + "num_batches_tracked"] = w[prefix + "num_batches_tracked"] + 1
    else:
        mean, var = w[prefix + "running_mean"].to(y.dtype), w[prefix + "running_var"].to(y.dtype)
    xhat = (y - mean[None, :, None, None]) / torch.sqrt(var + EPS)[None, :, None, None]
    return xhat * g[None, :, None, None] + b[None, :, None, None]


# ---- the encoder ------------------------------------------------------------------------------------------------------------------
def encoder_keys(output_dim, norm):
    """[(key, shape)] of BasicEncoder's state dict in the reference's order: norm1, conv1, per block conv1, conv2, norm1, norm2,
    [norm3, downsample.0, downsample.1 (norm3 again)], conv2.  Only 'batch' norms have entries."""
    bn = lambda p, c: [(p + f, (c,) if s is None else s) for f, s in BN_FIELDS] if norm == "batch" else []
    conv = lambda p, co, ci, k: [(p + "weight", (co, ci, k, k)), (p + "bias", (co,))]
    out = bn("norm1.", 64) + conv("conv1.", 64, 3, 7)
    planes = 64
    for i, (dim, stride) in enumerate(LAYERS, 1):
        for j, cin in enumerate((planes, dim)):
            p = "layer%d.%d." % (i, j)
            out += conv(p + "conv1.", dim, cin, 3) + conv(p + "conv2.", dim, dim, 3) + bn(p + "norm1.", dim) + bn(p + "norm2.", dim)
            if j == 0 and stride != 1:
                out += bn(p + "norm3.", dim) + conv(p + "downsample.0.", dim, cin, 1) + bn(p + "downsample.1.", dim)
        planes = dim
    return out + conv("conv2.", output_dim, 128, 1)


def make_encoder_weights(output_dim, norm, seed):
    """He-scaled conv weights, N(0, 0.1^2) biases; BatchNorm: gamma 1 + 0.1 N, beta 0.1 N, running_mean 0.2 N, running_var in
    0.5 .. 1.5, num_batches_tracked 3 -- non-trivial, so that eval mode and the running-statistics update are really tested.
    downsample.1 is norm3 (one module under two names): equal tensors."""
    gen = torch.Generator().manual_seed(seed)
    w = {}
    for key, shape in encoder_keys(output_dim, norm):
        field = key.rsplit(".", 1)[1]
        if ".downsample.1." in key:
            w[key] = w[key.replace(".downsample.1.", ".norm3.")].clone()
        elif len(shape) == 4:
            w[key] = torch.randn(*shape, generator=gen) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif field == "num_batches_tracked":
            w[key] = torch.tensor(3, dtype=torch.int64)
        elif field == "running_var":
            w[key] = 0.5 + torch.rand(*shape, generator=gen)
        elif field == "running_mean":
            w[key] = 0.2 * torch.randn(*shape, generator=gen)
        elif field == "weight":                                     # a BatchNorm's gamma (conv weights are 4-d)
            w[key] = 1.0 + 0.1 * torch.randn(*shape, generator=gen)
        else:
            w[key] = 0.1 * torch.randn(*shape, generator=gen)
    return w


def is_float_key(key):
    return not key.endswith("num_batches_tracked")


def cast(w, dtype):
    return {k: (v.to(dtype) if is_float_key(k) else v) for k, v in w.items()}


def basic_encoder(w, x, norm, train=False, relus=None, new_stats=None):
    """extractor.py:168-192 on a tensor or a list of two; norm is 'instance', 'batch' or 'none'; `train` matters to 'batch' only."""
    r = _relus(relus)
    assert norm in ("instance", "batch", "none"), norm
    is_list = isinstance(x, (tuple, list))
    if is_list:
        batch_dim = x[0].shape[0]
        x = torch.cat(list(x), 0)
    conv = lambda name, t, stride=1, pad=0: F.conv2d(t, w[name + ".weight"], w[name + ".bias"], stride=stride, padding=pad)

    def normed(y, name):
        if norm == "instance":
            return S.instance_norm(y)
        if norm == "batch":
            return batch_norm(y, w, name + ".", train, new_stats)
        return y
    x = _relu(r, normed(conv("conv1", x, 2, 3), "norm1"), "conv1")
    for i, (dim, stride) in enumerate(LAYERS, 1):
        for j in (0, 1):
            p = "layer%d.%d." % (i, j)
            s = stride if j == 0 else 1
            y = _relu(r, normed(conv(p + "conv1", x, s, 1), p + "norm1"), p + "conv1")
            y = _relu(r, normed(conv(p + "conv2", y, 1, 1), p + "norm2"), p + "conv2")
            if s != 1:
                x = normed(conv(p + "downsample.0", x, s), p + "norm3")
            x = _relu(r, x + y, p + "add")
    x = conv("conv2", x)
    if is_list:
        return torch.split(x, [batch_dim, batch_dim], dim=0)
    return x


# ---- the update block -------------------------------------------------------------------------------------------------------------
def update_layout():
    """[(state-dict prefix, Cout, Cin, (kh, kw))] in the reference's registration order."""
    gin = HIDDEN + CONTEXT + 128
    return ([("encoder.convc1", 256, PLANES, (1, 1)), ("encoder.convc2", 192, 256, (3, 3)), ("encoder.convf1", 128, 2, (7, 7)),
             ("encoder.convf2", 64, 128, (3, 3)), ("encoder.conv", 126, 256, (3, 3))]
            + [("gru.conv%s1" % g, HIDDEN, gin, (1, 5)) for g in "zrq"] + [("gru.conv%s2" % g, HIDDEN, gin, (5, 1)) for g in "zrq"]
            + [("flow_head.conv1", 256, HIDDEN, (3, 3)), ("flow_head.conv2", 2, 256, (3, 3)),
               ("mask.0", 256, 128, (3, 3)), ("mask.2", 576, 256, (1, 1))])


def update_keys():
    out = []
    for name, co, ci, (kh, kw) in update_layout():
        out += [(name + ".weight", (co, ci, kh, kw)), (name + ".bias", (co,))]
    return out


def make_update_weights(seed):
    gen = torch.Generator().manual_seed(seed)
    w = {}
    for name, co, ci, (kh, kw) in update_layout():
        w[name + ".weight"] = torch.randn(co, ci, kh, kw, generator=gen) * math.sqrt(2.0 / (ci * kh * kw))
        w[name + ".bias"] = 0.1 * torch.randn(co, generator=gen)
    return w


def motion_encoder(w, flow, corr, relus=None):
    r = _relus(relus)
    conv = lambda name, x, pad: F.conv2d(x, w[name + ".weight"], w[name + ".bias"], padding=pad)
    cor = _relu(r, conv("encoder.convc1", corr, 0), "update.convc1")
    cor = _relu(r, conv("encoder.convc2", cor, 1), "update.convc2")
    flo = _relu(r, conv("encoder.convf1", flow, 3), "update.convf1")
    flo = _relu(r, conv("encoder.convf2", flo, 1), "update.convf2")
    out = _relu(r, conv("encoder.conv", torch.cat([cor, flo], 1), 1), "update.conv")
    return torch.cat([out, flow], 1)


def sep_conv_gru(w, h, x):
    """update.py:45-60, the concatenated form."""
    for s, pad in (("1", (0, 2)), ("2", (2, 0))):
        conv = lambda g, t: F.conv2d(t, w["gru.conv%s%s.weight" % (g, s)], w["gru.conv%s%s.bias" % (g, s)], padding=pad)
        hx = torch.cat([h, x], 1)
        z = torch.sigmoid(conv("z", hx))
        rr = torch.sigmoid(conv("r", hx))
        q = torch.tanh(conv("q", torch.cat([rr * h, x], 1)))
        h = (1 - z) * h + z * q
    return h


def sep_conv_gru_split(w, h, inp, motion):
    """The same function by the implementation's algebra: per pass, the three filters cut by input block and stacked by gate, each
    contraction a 1x1 convolution over shift_stack(., axis), the context term c computed on its own."""
    hd = h.shape[1]
    for axis, s in ((0, "1"), (1, "2")):
        stack = torch.cat([w["gru.conv%s%s.weight" % (g, s)] for g in "zrq"], 0)
        bias = torch.cat([w["gru.conv%s%s.bias" % (g, s)] for g in "zrq"])
        cut = lambda t: stacked_filter(t)
        gh, gq = cut(stack[:2 * hd, :hd]), cut(stack[2 * hd:, :hd])
        gc, gx = cut(stack[:, hd:hd + inp.shape[1]]), cut(stack[:, hd + inp.shape[1]:])
        c = F.conv2d(shift_stack(inp, axis), gc, bias)
        a_x = F.conv2d(shift_stack(motion, axis), gx)
        a_h = F.conv2d(shift_stack(h, axis), gh)
        z = torch.sigmoid((a_h[:, :hd] + a_x[:, :hd]) + c[:, :hd])
        rr = torch.sigmoid((a_h[:, hd:] + a_x[:, hd:2 * hd]) + c[:, hd:2 * hd])
        a_q = F.conv2d(shift_stack(rr * h, axis), gq)
        q = torch.tanh((a_q + a_x[:, 2 * hd:]) + c[:, 2 * hd:])
        h = (1 - z) * h + z * q
    return h


def update_block(w, net, inp, corr, flow, relus=None):
    """(net, raw mask, delta_flow) of update.py:127-136; the reference's 0.25 is upsample_flow's mask_scale here."""
    r = _relus(relus)
    conv = lambda name, x, pad: F.conv2d(x, w[name + ".weight"], w[name + ".bias"], padding=pad)
    motion = motion_encoder(w, flow, corr, r)
    net = sep_conv_gru(w, net, torch.cat([inp, motion], 1))
    delta = conv("flow_head.conv2", _relu(r, conv("flow_head.conv1", net, 1), "update.flow_head"), 1)
    mask = conv("mask.2", _relu(r, conv("mask.0", net, 1), "update.mask"), 0)
    return net, mask, delta


UPDATE_INPUTS = ("net", "inp", "corr", "flow")


def make_update_case(B, H, W, seed):
    """(inputs dict, cotangents (d net, d mask, d delta_flow)): unit-normal inputs, flow of a few pixels."""
    gen = torch.Generator().manual_seed(seed)
    x = {"net": torch.tanh(torch.randn(B, HIDDEN, H, W, generator=gen)), "inp": torch.relu(torch.randn(B, CONTEXT, H, W, generator=gen)),
         "corr": torch.randn(B, PLANES, H, W, generator=gen), "flow": 2.0 * torch.randn(B, 2, H, W, generator=gen)}
    cot = (torch.randn(B, HIDDEN, H, W, generator=gen), torch.randn(B, 576, H, W, generator=gen), torch.randn(B, 2, H, W, generator=gen))
    return x, cot


def run_update(w, x, cot, dtype):
    """{"net", "mask", "delta", "d/<input>", "d/<parameter key>"} of one call for the loss <net, dn> + <mask, dm> + <delta, dd>."""
    w = {k: v.detach().to(dtype).requires_grad_(True) for k, v in w.items()}
    x = {k: v.detach().to(dtype).requires_grad_(True) for k, v in x.items()}
    net, mask, delta = update_block(w, *(x[k] for k in UPDATE_INPUTS))
    loss = sum((o * c.to(dtype)).sum() for o, c in zip((net, mask, delta), cot))
    names = list(UPDATE_INPUTS) + list(w)
    grads = torch.autograd.grad(loss, [x[k] for k in UPDATE_INPUTS] + list(w.values()))
    res = {"d/" + n: g.detach() for n, g in zip(names, grads)}
    res.update(net=net.detach(), mask=mask.detach(), delta=delta.detach())
    return res


# ---- the model --------------------------------------------------------------------------------------------------------------------
def state_keys():
    """[(key, shape)] of RAFT's state dict, in order."""
    return ([("fnet." + k, s) for k, s in encoder_keys(256, "instance")] + [("cnet." + k, s) for k, s in encoder_keys(HIDDEN + CONTEXT, "batch")]
            + [("update_block." + k, s) for k, s in update_keys()])


def make_weights(seed):
    w = {"fnet." + k: v for k, v in make_encoder_weights(256, "instance", seed).items()}
    w.update({"cnet." + k: v for k, v in make_encoder_weights(HIDDEN + CONTEXT, "batch", seed + 1).items()})
    w.update({"update_block." + k: v for k, v in make_update_weights(seed + 2).items()})
    return w


def parameter_keys(w):
    """The keys of `w` that are parameters (not BatchNorm buffers, and not downsample.1's second name for norm3)."""
    return [k for k in w if not any(f in k for f in ("running_mean", "running_var", "num_batches_tracked"))]


def basic_raft(w, image1, image2, iters=12, flow_init=None, train=False, relus=None, new_stats=None):
    """(low-resolution flows, full-resolution flows) of raft.py:184-244, every iteration upsampled.  downsample.1.* are norm3's
    tensors under a second name: the forward reads norm3.* only."""
    image1 = 2 * image1 - 1.0
    image2 = 2 * image2 - 1.0
    fmap1, fmap2 = basic_encoder(sub(w, "fnet."), [image1, image2], "instance", relus=relus)
    levels = corr_ref.pyramid(fmap1, fmap2, LEVELS)
    stats = {} if new_stats is not None else None
    cnet = basic_encoder(sub(w, "cnet."), image1, "batch", train, relus, stats)
    if new_stats is not None:
        new_stats.update({"cnet." + k: v for k, v in stats.items()})
    net, inp = torch.split(cnet, [HIDDEN, CONTEXT], dim=1)
    net, inp = torch.tanh(net), _relus(relus).relu(inp.contiguous(), "inp")     # (contiguous: Relus can then force one of its masks)
    B, _, H, W = image1.shape
    coords0 = coords_grid(B, H // 8, W // 8, image1.dtype)
    coords1 = coords0 if flow_init is None else coords0 + flow_init
    wu = sub(w, "update_block.")
    low, full = [], []
    for _ in range(iters):
        coords1 = coords1.detach()
        corr = corr_ref.lookup(levels, coords1, RADIUS)
        net, mask, delta = update_block(wu, net, inp, corr, coords1 - coords0, relus)
        coords1 = coords1 + delta
        low.append(coords1 - coords0)
        full.append(upsample_flow(coords1 - coords0, mask, MASK_SCALE))
    return low, full


def run_raft(w, image1, image2, cot, dtype, iters, flow_init=None, train=False, relus=None):
    """{"low<k>", "flow<k>", "d/<parameter key>", "stats/<buffer key>"}: the loss is sum_k <flow_k, cot_k>.  downsample.1's
    weight and bias are norm3's: the gradient is reported under norm3 only."""
    pk = [k for k in parameter_keys(w) if ".downsample.1." not in k]
    w = {k: (v.detach().to(dtype).requires_grad_(k in pk) if is_float_key(k) else v) for k, v in w.items()}
    fi = flow_init.to(dtype) if flow_init is not None else None
    stats = {}
    low, full = basic_raft(w, image1.to(dtype), image2.to(dtype), iters, fi, train, relus, stats)
    loss = sum((f * c.to(dtype)).sum() for f, c in zip(full, cot))
    grads = torch.autograd.grad(loss, [w[k] for k in pk], allow_unused=True)
    res = {"d/" + k: (g.detach() if g is not None else torch.zeros_like(w[k])) for k, g in zip(pk, grads)}
    res.update({"stats/" + k: v.detach() for k, v in stats.items()})
    for k in range(iters):
        res["low%d" % k], res["flow%d" % k] = low[k].detach(), full[k].detach()
    return res


def run_encoder(w, x, cot, norm, dtype, train=False, relus=None):
    """{"out", "d/x", "d/<parameter key>", "stats/<buffer key>"} of basic_encoder on one tensor x for the loss <out, cot>."""
    pk = [k for k in parameter_keys(w) if ".downsample.1." not in k]
    w = {k: (v.detach().to(dtype).requires_grad_(k in pk) if is_float_key(k) else v) for k, v in w.items()}
    x = x.detach().to(dtype).requires_grad_(True)
    stats = {}
    out = basic_encoder(w, x, norm, train, relus, stats)
    grads = torch.autograd.grad((out * cot.to(dtype)).sum(), [x] + [w[k] for k in pk], allow_unused=True)
    res = {"d/" + k: (g.detach() if g is not None else torch.zeros_like(w[k] if k != "x" else x)) for k, g in zip(["x"] + pk, grads)}
    res.update({"stats/" + k: v.detach() for k, v in stats.items()})
    res["out"] = out.detach()
    return res


def encoder_margins(w, x, norm, train):
    """raft_ref.encoder_margins for basic_encoder: (relative ReLU margin of the fp64 run, relative pre-activation difference of
    the fp32 and fp64 runs) for the ReLU tensor where margin / difference is smallest."""
    r64, r32 = Relus(keep=True), Relus(keep=True)
    with torch.no_grad():
        basic_encoder(cast(w, torch.float64), x.double(), norm, train, r64)
        basic_encoder(cast(w, torch.float32), x.float(), norm, train, r32)
    pairs = [(c[1], float((a.double() - b).abs().max() / b.abs().max())) for c, a, b in zip(r64.calls, r32.pre, r64.pre)]
    return min(pairs, key=lambda p: p[0] / max(p[1], 1e-300))


def zero_gradient_biases(norm, train):
    """The conv biases in front of a norm that removes the mean (instance norm; BatchNorm on batch statistics): their gradients
    are mathematically zero.  Every bias but conv2's."""
    if norm == "none" or (norm == "batch" and not train):
        return []
    return [k for k, s in encoder_keys(256, "none") if k.endswith(".bias") and k != "conv2.bias"]


# ---- the seeded cases the fixture generator and the GPU tests share -------------------------------------------------------------
ENC_MODES = (("instance", False), ("batch", True), ("batch", False), ("none", False))         # (norm_fn, train)
ENC_SIZES = ((16, 24), (24, 40))
G6 = dict(B=2, H=128, W=136, iters=2, image_seed=71, weight_seed=72, cot_seed=73, init_seed=74)


def enc_case(size, norm, seed):
    """(weights, x [2,3,h,w], cotangent) of one element-wise gradient case."""
    gen = torch.Generator().manual_seed(seed)
    w = make_encoder_weights(128, norm, seed)
    x = torch.rand(2, 3, *size, generator=gen) * 2 - 1
    cot = torch.randn(2, 128, size[0] // 8, size[1] // 8, generator=gen)
    return w, x, cot


def g6_case(case):
    """(weights, image1, image2, cotangents, flow_init) of the end-to-end GPU test."""
    c = G6
    w = make_weights(c["weight_seed"])
    im1, im2 = S.make_images(c["B"], c["H"], c["W"], c["image_seed"])
    gen = torch.Generator().manual_seed(c["cot_seed"])
    cot = [torch.randn(c["B"], 2, c["H"], c["W"], generator=gen) for _ in range(c["iters"])]
    init = None
    if case == "init":
        init = 2.0 * torch.randn(c["B"], 2, c["H"] // 8, c["W"] // 8, generator=torch.Generator().manual_seed(c["init_seed"]))
    return w, im1, im2, cot, init


def convex_case(N, h, w, seed):
    """(flow, mask, cotangent) of one convex-upsampling case: flow of a few pixels, mask logits of a few units."""
    gen = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn(N, 2, h, w, generator=gen), 4.0 * torch.randn(N, 576, h, w, generator=gen),
            torch.randn(N, 2, 8 * h, 8 * w, generator=gen))


CONVEX_SHAPES = ((1, 1), (1, 5), (3, 2), (5, 7), (16, 17))
CONVEX_CASES = [(h, w, N, s) for (h, w) in CONVEX_SHAPES for N in (1, 3) for s in (1.0, 0.25)]


def convex_seed(h, w, N):
    return 1000 * h + 10 * w + N


def run_convex(flow, mask, cot, scale, dtype):
    """(out, dflow, dmask) of upsample_flow in `dtype` for the loss <out, cot>."""
    f, m = flow.to(dtype).requires_grad_(True), mask.to(dtype).requires_grad_(True)
    out = upsample_flow(f, m, scale)
    df, dm = torch.autograd.grad(out, [f, m], cot.to(dtype))
    return out.detach(), df, dm
