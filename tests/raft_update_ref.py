"""SmallRAFT's update block, restated (model/raft/core/update.py:62-112) as a function over a dict of weights keyed by the
state-dict names.

Plain torch on the CPU (or any device), one function for every precision: fp64 tensors give the truth, fp32 tensors the error
that fp32 arithmetic of this formulation makes on the same inputs.  It is the CONCATENATED form -- F.conv2d over cat[h, inp,
motion, flow] with the full 242-channel filters -- so it shares nothing with the split, hoisted implementation under test.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

CTX_DIM = 64
INPUTS = ("net", "inp", "corr", "flow")


def layout(hidden, cor_planes):
    """[(state-dict prefix, Cout, Cin, k)] in the reference's registration order."""
    gin = hidden + CTX_DIM + 82
    return [("encoder.convc1", 96, cor_planes, 1), ("encoder.convf1", 64, 2, 7), ("encoder.convf2", 32, 64, 3),
            ("encoder.conv", 80, 128, 3), ("gru.convz", hidden, gin, 3), ("gru.convr", hidden, gin, 3),
            ("gru.convq", hidden, gin, 3), ("flow_head.conv1", 128, hidden, 3), ("flow_head.conv2", 2, 128, 3)]


def state_keys(hidden, cor_planes):
    """[(key, shape)] of the block's state dict."""
    out = []
    for name, co, ci, k in layout(hidden, cor_planes):
        out += [(name + ".weight", (co, ci, k, k)), (name + ".bias", (co,))]
    return out


def make_weights(hidden, cor_planes, seed):
    """He-scaled fp32 weights (std sqrt(2 / fan_in)) and N(0, 0.1^2) biases from a seeded CPU generator."""
    gen = torch.Generator().manual_seed(seed)
    w = {}
    for name, co, ci, k in layout(hidden, cor_planes):
        w[name + ".weight"] = torch.randn(co, ci, k, k, generator=gen) * math.sqrt(2.0 / (ci * k * k))
        w[name + ".bias"] = 0.1 * torch.randn(co, generator=gen)
    return w


def make_case(hidden, cor_planes, B, H, W, seed, steps=1):
    """(inputs dict, cotangents [(d net, d delta_flow)] per step): unit-normal inputs, flow of a few pixels."""
    gen = torch.Generator().manual_seed(seed)
    x = {"net": torch.tanh(torch.randn(B, hidden, H, W, generator=gen)), "inp": torch.relu(torch.randn(B, CTX_DIM, H, W, generator=gen)),
         "corr": torch.randn(B, cor_planes, H, W, generator=gen), "flow": 2.0 * torch.randn(B, 2, H, W, generator=gen)}
    cot = [(torch.randn(B, hidden, H, W, generator=gen), torch.randn(B, 2, H, W, generator=gen)) for _ in range(steps)]
    return x, cot


def update_block(w, net, inp, corr, flow):
    """(net, delta_flow) of one call (update.py:106-112)."""
    conv = lambda name, x, pad: F.conv2d(x, w[name + ".weight"], w[name + ".bias"], padding=pad)
    cor = F.relu(conv("encoder.convc1", corr, 0))
    flo = F.relu(conv("encoder.convf1", flow, 3))
    flo = F.relu(conv("encoder.convf2", flo, 1))
    out = F.relu(conv("encoder.conv", torch.cat([cor, flo], 1), 1))
    x = torch.cat([inp, out, flow], 1)
    hx = torch.cat([net, x], 1)
    z = torch.sigmoid(conv("gru.convz", hx, 1))
    r = torch.sigmoid(conv("gru.convr", hx, 1))
    q = torch.tanh(conv("gru.convq", torch.cat([r * net, x], 1), 1))
    net = (1 - z) * net + z * q
    return net, conv("flow_head.conv2", F.relu(conv("flow_head.conv1", net, 1)), 1)


def chain(step, net, inp, corr, flow, cot):
    """len(cot) calls of step(net, inp, corr, flow) -> (net, delta_flow) the way raft.py:100-117 chains them, minus the lookup:
    the hidden state is carried, the flow moves by delta_flow and is detached before the next call (raft.py:101), corr and inp
    stay.  Returns (outputs [(net_k, delta_k)], loss = sum_k <net_k, dn_k> + <delta_k, dd_k>)."""
    outs, loss = [], 0
    for dn, dd in cot:
        net, delta = step(net, inp, corr, flow)
        outs.append((net, delta))
        loss = loss + (net * dn.to(net.dtype)).sum() + (delta * dd.to(delta.dtype)).sum()
        flow = (flow + delta).detach()
    return outs, loss


def run(w, x, cot, dtype, device="cpu"):
    """The restatement on (w, x) cast to dtype: {"net<k>", "delta<k>", "d/net", .., "d/<parameter key>"} detached on the CPU."""
    w = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in w.items()}
    x = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in x.items()}
    cot = [(a.to(device), b.to(device)) for a, b in cot]
    outs, loss = chain(lambda *a: update_block(w, *a), x["net"], x["inp"], x["corr"], x["flow"], cot)
    names = list(INPUTS) + list(w)
    grads = torch.autograd.grad(loss, [x[k] for k in INPUTS] + list(w.values()))
    res = {"d/" + n: g.detach().cpu() for n, g in zip(names, grads)}
    for k, (n, d) in enumerate(outs):
        res["net%d" % k], res["delta%d" % k] = n.detach().cpu(), d.detach().cpu()
    return res


def reference(w, x, cot):
    return {dt: run(w, x, cot, dt) for dt in (torch.float64, torch.float32)}


def checksum(t):
    """(sum, sum of |.|) in fp64."""
    t = torch.as_tensor(t).double()
    return np.array([float(t.sum()), float(t.abs().sum())])


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def ulp_floor(top):
    return 2.0 * float(np.spacing(np.float32(top)))


def bound(ref64, ref32):
    """corr_ref.bound's rule: 3 x the fp32 restatement's own error, floor 2 ulp of the tensor's max."""
    return max(3.0 * float((ref32.double() - ref64).abs().max()), ulp_floor(float(ref64.abs().max())))


OUT_TOL, GRAD_TOL = 2e-5, 1e-4      # of the tensor's max: tests/test_conv_gpu.py, restated in test_conv_sequences_gpu.py:12-13


def conv_tol(name):
    return GRAD_TOL if name.startswith("d/") else OUT_TOL


def check_rel(name, got, ref64, extra=0.0):
    """Every element within max(conv_tol(name) * max |ref|, extra)."""
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    top = float(ref64.abs().max())
    err, b = float((got - ref64.double()).abs().max()), max(conv_tol(name) * top, extra)
    print("%s: max |err| %.3e, bound %.3e (max |ref| %.3e)" % (name, err, b, top))
    assert err <= b, (name, err, b)
