"""SmallRAFT, restated (model/raft/core/raft.py:23-119, extractor.py:60-116 and 195-267, utils/utils.py:74-82) as functions over a
dict of weights keyed by the state-dict names.

Plain torch on the CPU (or any device), one function for every precision: fp64 tensors give the truth, fp32 tensors the error
that fp32 arithmetic of this formulation makes on the same inputs.  The correlation block is corr_ref's, the update block
raft_update_ref's with its ReLUs routed through the helper below.  The reference's own SmallRAFT cannot run in fp64 (corr.py casts with .float(), coords_grid is fp32), which is
why the truth comes from here and the reference contributes an fp32 fixture (tests/golden/make_golden_raft.py).

Every ReLU of the model (encoders, context split, update block) goes through `Relus.relu`: it can record the smallest
|pre-activation| / max |pre-activation| of each tensor it sees, exact zeros aside (the margin a perturbation must cross to flip a
mask), every pre-activation, and it can force the mask of one element the other way.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import corr_ref
import raft_update_ref as U
from raft_update_ref import GRAD_TOL, OUT_TOL, bound, checksum, ulp_floor  # noqa: F401  (the same rules)

HIDDEN, CONTEXT, LEVELS, RADIUS = 96, 64, 4, 3
PLANES = LEVELS * (2 * RADIUS + 1) ** 2
EPS = 1e-5
LAYERS = ((32, 1), (64, 2), (96, 2))


# ---- the ReLU helper ------------------------------------------------------------------------------------------------------------
class Relus:
    """relu(x) = x * [x > 0] with the mask exposed.  record: keep (name, relative margin, flat index of the closest element,
    number of elements, number of elements whose relative margin is below `count_below`) per call, and the detached
    pre-activations when keep=True.  force = (call index, flat element index): that one mask is inverted."""

    def __init__(self, keep=False, force=None, count_below=None):
        self.keep, self.force, self.count_below = keep, force, count_below
        self.calls, self.pre = [], []

    def relu(self, x, name=""):
        mask = x > 0
        k = len(self.calls)
        with torch.no_grad():
            a = x.detach().abs()
            top = float(a.max())
            flat = a.reshape(-1)
            # an exact zero is no risk: it is relu(.) + relu(.) of two negative pre-activations, which a perturbation leaves at 0
            live = torch.where(flat > 0, flat, torch.full_like(flat, float("inf")))
            i = int(live.argmin())
            rel = float(live[i]) / top if top > 0 and bool(torch.isfinite(live[i])) else float("inf")
            below = int((live < self.count_below * top).sum()) if self.count_below is not None else 0
            self.calls.append((name, rel, i, flat.numel(), below))
            if self.keep:
                self.pre.append(x.detach().clone())
        if self.force is not None and self.force[0] == k:
            mask = mask.clone()
            mask.view(-1)[self.force[1]] = ~mask.view(-1)[self.force[1]]
        return x * mask.to(x.dtype)

    def smallest_margin(self):
        return min(c[1] for c in self.calls)

    def most_at_risk(self):
        k = min(range(len(self.calls)), key=lambda j: self.calls[j][1])
        return k, self.calls[k][2]

    def inputs(self):
        return sum(c[3] for c in self.calls)

    def below(self):
        return sum(c[4] for c in self.calls)


def _relus(r):
    return r if r is not None else Relus()


# ---- the kernels' functions -----------------------------------------------------------------------------------------------------
def instance_norm(y):
    """nn.InstanceNorm2d(C) as the reference constructs it: no affine, no running statistics, biased variance, eps 1e-5."""
    return F.instance_norm(y, eps=EPS)


def instance_norm_act(y, norm=True, relu=True, residual=None, relus=None, name=""):
    r = _relus(relus)
    z = instance_norm(y) if norm else y
    if relu:
        z = r.relu(z, name + ".relu")
    if residual is not None:
        z = r.relu(residual + z, name + ".add")
    return z


def upflow8(flow):
    h, w = flow.shape[-2:]
    return 8 * F.interpolate(flow, size=(8 * h, 8 * w), mode="bilinear", align_corners=True)


def coords_grid(batch, ht, wd, dtype):
    ys, xs = torch.meshgrid(torch.arange(ht), torch.arange(wd), indexing="ij")
    return torch.stack([xs, ys], dim=0).to(dtype)[None].repeat(batch, 1, 1, 1)


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
def encoder_layout(output_dim):
    """[(state-dict prefix, Cout, Cin, k)] in the reference's registration order."""
    out = [("conv1", 32, 3, 7)]
    planes = 32
    for i, (dim, stride) in enumerate(LAYERS, 1):
        for j, cin in enumerate((planes, dim)):
            p = "layer%d.%d." % (i, j)
            out += [(p + "conv1", dim // 4, cin, 1), (p + "conv2", dim // 4, dim // 4, 3), (p + "conv3", dim, dim // 4, 1)]
            if j == 0 and stride != 1:
                out.append((p + "downsample.0", dim, cin, 1))
        planes = dim
    return out + [("conv2", output_dim, 96, 1)]


def encoder_keys(output_dim):
    out = []
    for name, co, ci, k in encoder_layout(output_dim):
        out += [(name + ".weight", (co, ci, k, k)), (name + ".bias", (co,))]
    return out


def state_keys():
    """[(key, shape)] of SmallRAFT's state dict, in order."""
    return ([("fnet." + k, s) for k, s in encoder_keys(128)] + [("cnet." + k, s) for k, s in encoder_keys(HIDDEN + CONTEXT)]
            + [("update_block." + k, s) for k, s in U.state_keys(HIDDEN, PLANES)])


def make_encoder_weights(output_dim, seed):
    gen = torch.Generator().manual_seed(seed)
    w = {}
    for name, co, ci, k in encoder_layout(output_dim):
        w[name + ".weight"] = torch.randn(co, ci, k, k, generator=gen) * math.sqrt(2.0 / (ci * k * k))
        w[name + ".bias"] = 0.1 * torch.randn(co, generator=gen)
    return w


def make_weights(seed):
    """He-scaled fp32 weights (std sqrt(2 / fan_in)) and N(0, 0.1^2) biases for every key of state_keys()."""
    w = {"fnet." + k: v for k, v in make_encoder_weights(128, seed).items()}
    w.update({"cnet." + k: v for k, v in make_encoder_weights(HIDDEN + CONTEXT, seed + 1).items()})
    w.update({"update_block." + k: v for k, v in U.make_weights(HIDDEN, PLANES, seed + 2).items()})
    return w


def sub(w, prefix):
    return {k[len(prefix):]: v for k, v in w.items() if k.startswith(prefix)}


def small_encoder(w, x, norm, relus=None):
    """extractor.py:244-267 on a tensor or a list of two; norm is 'instance' or 'none'."""
    r = _relus(relus)
    inst = norm == "instance"
    assert inst or norm == "none", norm
    is_list = isinstance(x, (tuple, list))
    if is_list:
        batch_dim = x[0].shape[0]
        x = torch.cat(list(x), 0)
    conv = lambda name, t, stride=1, pad=0: F.conv2d(t, w[name + ".weight"], w[name + ".bias"], stride=stride, padding=pad)
    x = instance_norm_act(conv("conv1", x, 2, 3), inst, True, None, r, "conv1")
    for i, (dim, stride) in enumerate(LAYERS, 1):
        for j in (0, 1):
            p = "layer%d.%d." % (i, j)
            s = stride if j == 0 else 1
            y = instance_norm_act(conv(p + "conv1", x), inst, True, None, r, p + "conv1")
            y = instance_norm_act(conv(p + "conv2", y, s, 1), inst, True, None, r, p + "conv2")
            if s != 1:
                x = instance_norm_act(conv(p + "downsample.0", x, s), inst, False)
            x = instance_norm_act(conv(p + "conv3", y), inst, True, x, r, p + "conv3")
    x = conv("conv2", x)
    if is_list:
        return torch.split(x, [batch_dim, batch_dim], dim=0)
    return x


# ---- the model ------------------------------------------------------------------------------------------------------------------
def update_block(w, net, inp, corr, flow, relus=None):
    """raft_update_ref.update_block (update.py:106-112), the same torch calls, with its five ReLUs through the helper."""
    r = _relus(relus)
    conv = lambda name, x, pad: F.conv2d(x, w[name + ".weight"], w[name + ".bias"], padding=pad)
    cor = r.relu(conv("encoder.convc1", corr, 0), "update.convc1")
    flo = r.relu(conv("encoder.convf1", flow, 3), "update.convf1")
    flo = r.relu(conv("encoder.convf2", flo, 1), "update.convf2")
    out = r.relu(conv("encoder.conv", torch.cat([cor, flo], 1), 1), "update.conv")
    x = torch.cat([inp, out, flow], 1)
    hx = torch.cat([net, x], 1)
    z = torch.sigmoid(conv("gru.convz", hx, 1))
    rr = torch.sigmoid(conv("gru.convr", hx, 1))
    q = torch.tanh(conv("gru.convq", torch.cat([rr * net, x], 1), 1))
    net = (1 - z) * net + z * q
    return net, conv("flow_head.conv2", r.relu(conv("flow_head.conv1", net, 1), "update.flow_head"), 1)


def small_raft(w, image1, image2, iters=12, flow_init=None, relus=None):
    """(low-resolution flows, full-resolution flows) of raft.py:66-119."""
    image1 = 2 * image1 - 1.0
    image2 = 2 * image2 - 1.0
    fmap1, fmap2 = small_encoder(sub(w, "fnet."), [image1, image2], "instance", relus)
    levels = corr_ref.pyramid(fmap1, fmap2, LEVELS)
    cnet = small_encoder(sub(w, "cnet."), image1, "none", relus)
    net, inp = torch.split(cnet, [HIDDEN, CONTEXT], dim=1)
    net, inp = torch.tanh(net), _relus(relus).relu(inp, "inp")
    B, _, H, W = image1.shape
    coords0 = coords_grid(B, H // 8, W // 8, image1.dtype)
    coords1 = coords0 if flow_init is None else coords0 + flow_init
    wu = sub(w, "update_block.")
    low, full = [], []
    for _ in range(iters):
        coords1 = coords1.detach()
        corr = corr_ref.lookup(levels, coords1, RADIUS)
        net, delta = update_block(wu, net, inp, corr, coords1 - coords0, relus)
        coords1 = coords1 + delta
        low.append(coords1 - coords0)
        full.append(upflow8(coords1 - coords0))
    return low, full


def make_images(B, H, W, seed):
    """Two smooth-ish images in 0 .. 1 (the second the first moved by a few pixels, plus noise) and nothing else."""
    gen = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(B, 3, H // 4 + 2, W // 4 + 2, generator=gen), size=(H + 8, W + 8), mode="bilinear", align_corners=True)
    base = (base + 0.25 * torch.rand(B, 3, H + 8, W + 8, generator=gen)) / 1.25
    im1 = base[:, :, 4:4 + H, 4:4 + W].contiguous()
    im2 = (base[:, :, 2:2 + H, 6:6 + W] + 0.02 * torch.randn(B, 3, H, W, generator=gen)).clamp(0, 1).contiguous()
    return im1, im2


def run_raft(w, image1, image2, cot, dtype, iters, flow_init=None, relus=None):
    """{"low<k>", "flow<k>", "d/<key>"}: the loss is sum_k <flow_k, cot_k>."""
    w = {k: v.detach().to(dtype).requires_grad_(True) for k, v in w.items()}
    fi = flow_init.to(dtype) if flow_init is not None else None
    low, full = small_raft(w, image1.to(dtype), image2.to(dtype), iters, fi, relus)
    loss = sum((f * c.to(dtype)).sum() for f, c in zip(full, cot))
    grads = torch.autograd.grad(loss, list(w.values()))
    res = {"d/" + k: g.detach() for k, g in zip(w, grads)}
    for k in range(iters):
        res["low%d" % k], res["flow%d" % k] = low[k].detach(), full[k].detach()
    return res


def run_encoder(w, x, cot, norm, dtype, relus=None):
    """{"out", "d/x", "d/<key>"} of small_encoder on one tensor x for the loss <out, cot>."""
    w = {k: v.detach().to(dtype).requires_grad_(True) for k, v in w.items()}
    x = x.detach().to(dtype).requires_grad_(True)
    out = small_encoder(w, x, norm, relus)
    grads = torch.autograd.grad((out * cot.to(dtype)).sum(), [x] + list(w.values()))
    res = {"d/" + k: g.detach() for k, g in zip(["x"] + list(w), grads)}
    res["out"] = out.detach()
    return res


def zero_gradient_biases(prefix="", own_output=True):
    """The conv biases in front of an instance norm: their gradients are mathematically zero (the norm removes the mean).  Every
    bias of an 'instance' encoder but conv2's; own_output=False also leaves conv1.bias out (the issue's list of 20)."""
    names = [n for n, _, _, _ in encoder_layout(128) if n != "conv2" and (own_output or n != "conv1")]
    return [prefix + n + ".bias" for n in names]


def rel_l2(got, ref):
    ref = ref.double()
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def encoder_margins(w, x, norm):
    """Per ReLU tensor of the encoder: (relative margin of the fp64 run, relative pre-activation difference between the fp32 and
    fp64 runs), both relative to that tensor's max.  Returned for the tensor where margin / difference is smallest."""
    r64, r32 = Relus(keep=True), Relus(keep=True)
    with torch.no_grad():
        small_encoder({k: v.double() for k, v in w.items()}, x.double(), norm, r64)
        small_encoder({k: v.float() for k, v in w.items()}, x.float(), norm, r32)
    pairs = [(c[1], float((a.double() - b).abs().max() / b.abs().max())) for c, a, b in zip(r64.calls, r32.pre, r64.pre)]
    return min(pairs, key=lambda p: p[0] / max(p[1], 1e-300))


# ---- the seeded cases the fixture generator and the GPU tests share ---------------------------------------------------------
G6 = dict(B=2, H=128, W=136, iters=3, image_seed=61, weight_seed=62, cot_seed=63, init_seed=64)
G5_CASES = [((16, 24), "instance"), ((16, 24), "none"), ((24, 40), "instance"), ((24, 40), "none")]


def g6_case(case):
    """(weights, image1, image2, cotangents, flow_init) of the end-to-end GPU test."""
    c = G6
    w = make_weights(c["weight_seed"])
    im1, im2 = make_images(c["B"], c["H"], c["W"], c["image_seed"])
    gen = torch.Generator().manual_seed(c["cot_seed"])
    cot = [torch.randn(c["B"], 2, c["H"], c["W"], generator=gen) for _ in range(c["iters"])]
    init = None
    if case == "init":
        init = 2.0 * torch.randn(c["B"], 2, c["H"] // 8, c["W"] // 8, generator=torch.Generator().manual_seed(c["init_seed"]))
    return w, im1, im2, cot, init


def g5_case(size, norm, seed):
    """(weights, x [2,3,h,w], cotangent) of one element-wise gradient case."""
    gen = torch.Generator().manual_seed(seed)
    w = make_encoder_weights(128, seed)
    x = torch.rand(2, 3, *size, generator=gen) * 2 - 1
    cot = torch.randn(2, 128, size[0] // 8, size[1] // 8, generator=gen)
    return w, x, cot
