"""FlowPoseNet, restated (model/posenet_single.py:91-147) as functions over a dict of weights keyed by the state-dict names: SmallRAFT
is raft_ref's, the regressor (three strided convolutions, global average pooling, Linear, * 0.01) is plain torch.

One function for every precision: fp64 tensors give the truth, fp32 tensors the error that fp32 arithmetic of this formulation
makes on the same inputs.  Every ReLU goes through raft_ref.Relus, the regressor's three included.
"""
import math

import torch
import torch.nn.functional as F

import raft_ref as R
from raft_ref import GRAD_TOL, OUT_TOL, bound, checksum, rel_l2, ulp_floor  # noqa: F401  (the same rules)

POSE_SCALE = 0.01
ITERS = 12                                                  # the reference's SmallRAFT default, which its FlowPoseNet uses
REGRESSOR = (("pose_cnn.0", 32, 2, 7, 2, 3), ("pose_cnn.2", 64, 32, 5, 2, 2), ("pose_cnn.4", 128, 64, 3, 2, 1))     # name, Cout, Cin, k, stride, pad
PARAMETERS = 1119224


def regressor_keys():
    out = []
    for name, co, ci, k, _, _ in REGRESSOR:
        out += [(name + ".weight", (co, ci, k, k)), (name + ".bias", (co,))]
    return out + [("fc.weight", (6, 128)), ("fc.bias", (6,))]


def state_keys():
    """[(key, shape)] of FlowPoseNet's state dict, in order."""
    return [("flow_net." + k, s) for k, s in R.state_keys()] + regressor_keys()


def make_regressor_weights(seed):
    """He-scaled fp32 weights (std sqrt(2 / fan_in)) and N(0, 0.1^2) biases from a seeded CPU generator."""
    gen = torch.Generator().manual_seed(seed)
    w = {}
    for name, co, ci, k, _, _ in REGRESSOR:
        w[name + ".weight"] = torch.randn(co, ci, k, k, generator=gen) * math.sqrt(2.0 / (ci * k * k))
        w[name + ".bias"] = 0.1 * torch.randn(co, generator=gen)
    w["fc.weight"] = torch.randn(6, 128, generator=gen) * math.sqrt(2.0 / 128)
    w["fc.bias"] = 0.1 * torch.randn(6, generator=gen)
    return w


def make_weights(seed):
    """raft_ref.make_weights(seed) under flow_net., plus the seeded regressor."""
    w = {"flow_net." + k: v for k, v in R.make_weights(seed).items()}
    w.update(make_regressor_weights(seed + 3))
    return w


def regressor(w, flow, relus=None):
    """[B,6]: pose_cnn, the flatten, fc and the scale (posenet_single.py:137-142) of a [B,2,H,W] flow."""
    r = R._relus(relus)
    x = flow
    for name, _, _, _, stride, pad in REGRESSOR:
        x = r.relu(F.conv2d(x, w[name + ".weight"], w[name + ".bias"], stride=stride, padding=pad), name)
    feat = x.mean(dim=(2, 3))                               # AdaptiveAvgPool2d(1) and the view
    return F.linear(feat, w["fc.weight"], w["fc.bias"]) * POSE_SCALE


def flow_posenet(w, images, iters=ITERS, relus=None):
    """(axis-angle, translation), two [B,1,1,3] views, of [B,6,H,W] images in 0 .. 1."""
    _, full = R.small_raft(R.sub(w, "flow_net."), images[:, :3], images[:, 3:], iters, None, relus)
    pose6 = regressor(w, full[-1], relus).view(-1, 1, 1, 6)
    return pose6[..., :3], pose6[..., 3:]


def run_net(w, images, cot, dtype, iters, relus=None):
    """{"aa", "t", "d/<key>"}: the loss is <aa, cot[0]> + <t, cot[1]>."""
    w = {k: v.detach().to(dtype).requires_grad_(True) for k, v in w.items()}
    aa, t = flow_posenet(w, images.to(dtype), iters, relus)
    loss = (aa * cot[0].to(dtype)).sum() + (t * cot[1].to(dtype)).sum()
    grads = torch.autograd.grad(loss, list(w.values()))
    res = {"d/" + k: g.detach() for k, g in zip(w, grads)}
    res["aa"], res["t"] = aa.detach(), t.detach()
    return res


def run_regressor(w, flow, cot, dtype, relus=None):
    """{"out", "d/flow", "d/<key>"} of the regressor alone for the loss <out, cot>."""
    w = {k: v.detach().to(dtype).requires_grad_(True) for k, v in w.items()}
    flow = flow.detach().to(dtype).requires_grad_(True)
    out = regressor(w, flow, relus)
    grads = torch.autograd.grad((out * cot.to(dtype)).sum(), [flow] + list(w.values()))
    res = {"d/" + k: g.detach() for k, g in zip(["flow"] + list(w), grads)}
    res["out"] = out.detach()
    return res


def regressor_margins(w, flow):
    """raft_ref.encoder_margins for the regressor: (relative margin of the fp64 run, relative pre-activation difference between the
    fp32 and fp64 runs) of the ReLU tensor where margin / difference is smallest."""
    r64, r32 = R.Relus(keep=True), R.Relus(keep=True)
    with torch.no_grad():
        regressor({k: v.double() for k, v in w.items()}, flow.double(), r64)
        regressor({k: v.float() for k, v in w.items()}, flow.float(), r32)
    pairs = [(c[1], float((a.double() - b).abs().max() / b.abs().max())) for c, a, b in zip(r64.calls, r32.pre, r64.pre)]
    return min(pairs, key=lambda p: p[0] / max(p[1], 1e-300))


def pool_fc(y, W, b, relu, scale):
    """The issue's forward formulas of the pooling head on y [N,P,C]: (out [N,J], mean [N,C])."""
    mean = (F.relu(y) if relu else y).mean(1)               # F.relu: the gradient at y == 0 is 0
    out = mean @ W.t()
    if b is not None:
        out = out + b
    return scale * out, mean


# ---- the seeded cases the fixture generator and the GPU tests share ---------------------------------------------------------
G4 = dict(B=2, H=128, W=136, iters=3, image_seed=71, weight_seed=72, cot_seed=73)
G3_SIZES = [(16, 24), (24, 40)]


def g4_case():
    """(weights, images [B,6,H,W], cotangents (d aa, d t)) of the end-to-end GPU test."""
    c = G4
    w = make_weights(c["weight_seed"])
    im1, im2 = R.make_images(c["B"], c["H"], c["W"], c["image_seed"])
    gen = torch.Generator().manual_seed(c["cot_seed"])
    cot = (torch.randn(c["B"], 1, 1, 3, generator=gen), torch.randn(c["B"], 1, 1, 3, generator=gen))
    return w, torch.cat([im1, im2], 1), cot


def g3_case(size, seed):
    """(regressor weights, flow [2,2,h,w] of a few pixels, cotangent [2,6]) of one element-wise gradient case."""
    gen = torch.Generator().manual_seed(seed)
    w = make_regressor_weights(seed)
    flow = 2.0 * torch.randn(2, 2, *size, generator=gen)
    return w, flow, torch.randn(2, 6, generator=gen)
