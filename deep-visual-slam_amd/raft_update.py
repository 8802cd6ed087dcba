"""SmallRAFT's update block on the device: motion encoder, ConvGRU, flow head (model/raft/core/update.py:62-112).

    raft.update_block = raft_update.SmallUpdateBlock.from_module(raft.update_block)
    net, _, delta_flow = raft.update_block(net, inp, corr, flow)                    # raft.py:104-105

The reference's ConvGRU convolves ONE 242-channel concatenation hx = cat[h(hd), inp(64), motion(80), flow(2)] three times
(update.py:23-31).  242 is not a multiple of 4, so none of this package's kernels can gather it -- and they do not have to: a
convolution is linear in its input channels, conv(W, cat[a, b]) = conv(W[:, A], a) + conv(W[:, B], b).  The block therefore runs

    c   = conv(inp,        cat[Wz, Wr, Wq][:, hd:hd+64]) + cat[bz, br, bq]    once per context (raft.py:95 makes inp once, :100-117
                                                                              call the block 12 times with it): 26 % of the flops
    a_x = conv(motion(84), cat[Wz, Wr, Wq][:, hd+64:])                        the 82 motion channels zero-padded to 84
    a_h = conv(h,          cat[Wz, Wr][:, :hd])
    z, r, rh = gates(a_h, a_x, c, h)                                          csrc/gru.hip
    a_q = conv(rh,         Wq[:, :hd])
    h'  = blend(a_q, a_x, c, z, h)                                            csrc/gru.hip

with every convolution on conv.conv2d / conv.head_conv2d (the route plan picks the kernels, the process-wide precision mode applies)
and the gate arithmetic on four kernels of its own.  Weights are sliced, concatenated and zero-padded by differentiable torch ops
once per context, so gradients land on the original parameters, whose names and shapes are the reference's: a raft-small.pth
sub-dictionary loads with load_state_dict.  GPU and fp32 only; no host synchronisation in forward or backward.

BasicUpdateBlock (update.py:114-136) is the same split, twice: SepConvGRU's (1,5) and (5,1) convolutions are 1x1 convolutions
over shift_stack(x, axis), the five shifted copies of x side by side along the channels (csrc/shiftstack.hip), with the filter
re-laid by stacked_filter; the gate kernels are the same four.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, conv
from ._lib import DvsError, check
from ._raft_host import CL, DerivedOperands, aligned, gpu_arg

CTX_DIM = 64            # channels of `inp` (SmallRAFT's context_dim, raft.py:34)
MOTION_DIM = 82         # SmallMotionEncoder's 80 + the 2 flow channels (update.py:77)

_ENCODER = (("convc1", 96, None, 1), ("convf1", 64, 2, 7), ("convf2", 32, 64, 3), ("conv", 80, 128, 3))


def _rows(t):
    """(P, channels) of a [B,C,H,W] tensor in channels_last memory: the [P][C] matrix the gate kernels see."""
    B, Cn, H, W = t.shape
    return B * H * W, Cn


def _as_map(m, like, channels):
    """A [B,H,W,channels] matrix buffer as the [B,channels,H,W] channels_last tensor autograd expects."""
    B, _, H, W = like.shape
    return m.view(B, H, W, channels).permute(0, 3, 1, 2)


def _empty_map(like, channels):
    B, _, H, W = like.shape
    return torch.empty((B, H, W, channels), device=like.device, dtype=torch.float32)


def _gates_raw(a_h, a_x, c, h):
    P, hd = _rows(h)
    z, r, rh = (_as_map(_empty_map(h, hd), h, hd) for _ in range(3))
    check(_lib.lib().dvs_gru_gates_fwd(a_h.data_ptr(), a_x.data_ptr(), c.data_ptr(), h.data_ptr(), z.data_ptr(), r.data_ptr(),
                                       rh.data_ptr(), P, hd, _lib.stream()), "dvs_gru_gates_fwd")
    return z, r, rh


def _blend_raw(a_q, a_x, c, z, h):
    P, hd = _rows(h)
    q, h_new = (_as_map(_empty_map(h, hd), h, hd) for _ in range(2))
    check(_lib.lib().dvs_gru_blend_fwd(a_q.data_ptr(), a_x.data_ptr(), c.data_ptr(), z.data_ptr(), h.data_ptr(), q.data_ptr(),
                                       h_new.data_ptr(), P, hd, _lib.stream()), "dvs_gru_blend_fwd")
    return q, h_new


class _Link:
    """What the blend node's backward leaves for the gates node's of the same step: dpre [P][3hd] and dah [P][2hd] with the z
    (and q) columns written, and dh_a.  The gates node consumes z, which the blend node reads, so autograd always runs the blend
    node's backward first; the gates node then fills the r columns and hands the finished matrices on.  That way dpre is written
    once and is the gradient of a_x and of c without a sum of two half-empty tensors, and dh = dh_a + d_rh * r costs no
    accumulation pass."""
    __slots__ = ("dpre", "dah", "dh_a")

    def __init__(self):
        self.dpre = self.dah = self.dh_a = None


class _Gates(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a_h, a_x, c, h, link):
        ctx.set_materialize_grads(False)
        a_h, a_x, c, h = (aligned(t.detach(), CL) for t in (a_h, a_x, c, h))
        z, r, rh = _gates_raw(a_h, a_x, c, h)
        ctx.save_for_backward(r, h)
        ctx.link = link
        return z, r, rh

    @staticmethod
    def backward(ctx, dz, dr, d_rh):
        if dz is not None or dr is not None:
            raise DvsError("raft_update: z and r are internal to the update block; their gradients come through the blend node")
        link = ctx.link
        dpre, dah, dh_a = link.dpre, link.dah, link.dh_a
        link.dpre = link.dah = link.dh_a = None
        if dpre is None:
            if d_rh is not None:
                raise DvsError("raft_update: the gates node's backward ran before the blend node's of the same step (no dpre in "
                               "the link): z must reach the blend node through this node's output")
            return None, None, None, None, None
        r, h = ctx.saved_tensors
        P, hd = _rows(h)
        # a conv_q that hands no gradient back for r * h: the z and q columns the blend node wrote still count
        d_rh = torch.zeros_like(h) if d_rh is None else aligned(d_rh, CL)
        dh = _empty_map(h, hd)
        check(_lib.lib().dvs_gru_gates_bwd(d_rh.data_ptr(), h.data_ptr(), r.data_ptr(), dh_a.data_ptr(), dpre.data_ptr(),
                                           dah.data_ptr(), dh.data_ptr(), P, hd, _lib.stream()), "dvs_gru_gates_bwd")
        need = ctx.needs_input_grad
        dpre = _as_map(dpre, h, 3 * hd)
        return (_as_map(dah, h, 2 * hd) if need[0] else None, dpre if need[1] else None, dpre if need[2] else None,
                _as_map(dh, h, hd) if need[3] else None, None)


class _Blend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a_q, a_x, c, z, h, link):
        a_q, a_x, c, z, h = (aligned(t.detach(), CL) for t in (a_q, a_x, c, z, h))
        q, h_new = _blend_raw(a_q, a_x, c, z, h)
        ctx.save_for_backward(z, q, h)
        ctx.link = link
        return h_new

    @staticmethod
    def backward(ctx, g):
        z, q, h = ctx.saved_tensors
        P, hd = _rows(h)
        g = aligned(g, CL)
        dpre, dah, dq, dh_a = _empty_map(h, 3 * hd), _empty_map(h, 2 * hd), _empty_map(h, hd), _empty_map(h, hd)
        check(_lib.lib().dvs_gru_blend_bwd(g.data_ptr(), z.data_ptr(), q.data_ptr(), h.data_ptr(), dpre.data_ptr(), dah.data_ptr(),
                                           dq.data_ptr(), dh_a.data_ptr(), P, hd, _lib.stream()), "dvs_gru_blend_bwd")
        link = ctx.link
        link.dpre, link.dah, link.dh_a = dpre, dah, dh_a
        # a_x, c, z and h take their gradients from the gates node (see _Link)
        return _as_map(dq, h, hd) if ctx.needs_input_grad[0] else None, None, None, None, None, None


def conv_gru(a_h, a_x, c, h, conv_q):
    """h' of the split ConvGRU from the three pre-activation parts; conv_q(r * h) is the caller's convolution of the reset
    hidden state.  Differentiable in a_h, a_x, c, h and whatever conv_q closes over."""
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in (a_h, a_x, c, h)):
        a_h, a_x, c, h = (aligned(t, CL) for t in (a_h, a_x, c, h))
        z, _, rh = _gates_raw(a_h, a_x, c, h)
        a_q = conv_q(rh)
        if not a_q.requires_grad:
            return _blend_raw(aligned(a_q, CL), a_x, c, z, h)[1]
        return _Blend.apply(a_q, a_x, c, z, h, _Link())
    link = _Link()
    z, _, rh = _Gates.apply(a_h, a_x, c, h, link)
    return _Blend.apply(conv_q(rh), a_x, c, z, h, link)


class _Weights:
    """The kernels' view of the eighteen parameters: channels_last, the GRU's three filters stacked and cut by input block.
    cor and flo are the motion encoder's two chains of (filter, bias), m its closing convolution."""
    __slots__ = ("cor", "flo", "m", "gh", "gq", "gx", "gc", "h1", "h2")


def _cl(t):
    return t.contiguous(memory_format=CL)


def _pad_in(t, n):
    """A filter with n zero input channels behind its own."""
    return F.pad(t, (0, 0, 0, 0, 0, n))


def _flow4(flow):
    """flow as a NHWC tensor with two zero channels behind its own: 4 channels for convf1."""
    return F.pad(flow.permute(0, 2, 3, 1), (0, 2)).contiguous().permute(0, 3, 1, 2)


def _chain(x, layers):
    """relu(conv(.)) through `layers` of (filter, bias), each padded to keep the map's size."""
    for wt, b in layers:
        x = conv.conv2d(x, wt, b, padding=wt.shape[2] // 2, act="relu")
    return x


class _UpdateBlock(DerivedOperands, nn.Module):
    """One update step (update.py:99-136) up to what differs between the two blocks.  Here: the parameter holders under the
    reference's names, the cache of the derived operands and of the hoisted context terms (_raft_host.DerivedOperands), the input
    checks, the motion encoder and the flow head.  A subclass sets CTX (channels of `inp`) and GATE (the gate convolution whose
    width is hidden_dim) and provides _layout(hidden, planes), _operands(), _context_terms(inp, w) and its GRU in forward."""
    CTX = GATE = None

    def __init__(self, hidden_dim, corr_levels, corr_radius):
        super().__init__()
        self._setup(int(hidden_dim), int(corr_levels) * (2 * int(corr_radius) + 1) ** 2, None)

    @classmethod
    def from_module(cls, block):
        """Wrap a block of the reference's shape (duck typing: .encoder / .gru / .flow_head [/ .mask] with the class's
        convolutions), sharing its Parameter objects."""
        try:
            hidden, planes = getattr(block.gru, cls.GATE).weight.shape[0], block.encoder.convc1.weight.shape[1]
        except AttributeError as e:
            raise DvsError("%s.from_module: not a %s (%s)" % (cls.__name__, cls.__name__, e))
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._setup(int(hidden), int(planes), block)
        return self

    def _setup(self, hidden, planes, source):
        """self._layout's {group: [(name, Cout, Cin, k, padding)]}, k an int or (kh, kw): nn.Conv2d holders with the reference's
        init, or, with `source`, holders that share the Parameter objects of a block of the reference's shape."""
        who = type(self).__name__
        layout = self._layout(hidden, planes)               # refuses a hidden_dim the block cannot run
        if planes <= 0 or planes % 4:
            raise DvsError("%s: corr_levels * (2 * corr_radius + 1)^2 = %d correlation planes must be a multiple of 4 (the "
                           "reference's settings give 196 and 324)" % (who, planes))
        self.hidden_dim, self.cor_planes = hidden, planes
        for group, convs in layout.items():
            holder = nn.Module()
            for name, co, ci, k, pad in convs:
                kh, kw = (k, k) if isinstance(k, int) else k
                if source is None:
                    layer = nn.Conv2d(ci, co, (kh, kw), padding=pad)        # holds the parameters (and the reference's init) only
                else:
                    theirs = getattr(getattr(source, group, None), name, None)
                    w, b = getattr(theirs, "weight", None), getattr(theirs, "bias", None)
                    if not isinstance(w, nn.Parameter) or not isinstance(b, nn.Parameter):
                        raise DvsError("%s.from_module: %s.%s has no weight / bias parameters" % (who, group, name))
                    if tuple(w.shape) != (co, ci, kh, kw) or tuple(b.shape) != (co,):
                        raise DvsError("%s.from_module: %s.%s is %s / %s, expected %s / %s"
                                       % (who, group, name, tuple(w.shape), tuple(b.shape), (co, ci, kh, kw), (co,)))
                    layer = nn.Module()
                    layer.weight, layer.bias = w, b
                setattr(holder, name, layer)
            setattr(self, group, holder)
        self._drop()

    def _check(self, net, inp, corr, flow):
        who = type(self).__name__
        want = (("net", net, self.hidden_dim), ("inp", inp, self.CTX), ("corr", corr, self.cor_planes), ("flow", flow, 2))
        for name, t, _ in want:
            gpu_arg("%s: %s" % (who, name), t, "[B,C,H,W] expected")
        B, _, H, W = net.shape
        for name, t, ch in want:
            if tuple(t.shape) != (B, ch, H, W):
                raise DvsError("%s: %s must be [%d,%d,%d,%d], got %s" % (who, name, B, ch, H, W, tuple(t.shape)))
            if t.device != net.device:
                raise DvsError("%s: %s on %s, net on %s" % (who, name, t.device, net.device))
        for p in self.parameters():
            if p.device != net.device or p.dtype != torch.float32:
                raise DvsError("%s: parameters on %s / %s, inputs on %s / fp32; move the block with .to()"
                               % (who, p.device, p.dtype, net.device))

    def _enter(self, net, inp, corr, flow):
        """What a step does before its GRU: (operands, hoisted terms, net in NHWC memory, the motion encoder's output
        (update.py:71-77, 89-97) without the flow, the 4-channel flow)."""
        self._check(net, inp, corr, flow)
        w = self._derive()
        c = self._hoisted(inp, w)                           # reused while `inp` is the same tensor object and the weights stand
        net = conv._nhwc(net)
        flow4 = _flow4(flow)
        cor, flo = _chain(corr, w.cor), _chain(flow4, w.flo)
        return w, c, net, conv.conv2d(torch.cat([cor, flo], 1), *w.m, padding=1, act="relu"), flow4

    @staticmethod
    def _flow_head(w, net):
        """update.py:13-14."""
        return conv.head_conv2d(conv.conv2d(net, *w.h1, padding=1, act="relu"), *w.h2, 1, 0, None)


class SmallUpdateBlock(_UpdateBlock):
    """update.py:99-112 with the reference's parameter names: encoder.{convc1,convf1,convf2,conv}, gru.{convz,convr,convq},
    flow_head.{conv1,conv2}, each .weight / .bias."""
    CTX, GATE = CTX_DIM, "convz"

    def __init__(self, hidden_dim=96, corr_levels=4, corr_radius=3):
        super().__init__(hidden_dim, corr_levels, corr_radius)

    def _layout(self, hidden, planes):
        if hidden <= 0 or hidden % 4:
            raise DvsError("SmallUpdateBlock: hidden_dim=%d must be a positive multiple of 4 (16-byte channel groups)" % hidden)
        gin = hidden + CTX_DIM + MOTION_DIM
        return {"encoder": [(n, co, ci if ci is not None else planes, k, k // 2) for n, co, ci, k in _ENCODER],
                "gru": [(n, hidden, gin, 3, 1) for n in ("convz", "convr", "convq")],
                "flow_head": [("conv1", 128, hidden, 3, 1), ("conv2", 2, 128, 3, 1)]}

    def _operands(self):
        hd = self.hidden_dim
        e, g, f = self.encoder, self.gru, self.flow_head
        stack = torch.cat([g.convz.weight, g.convr.weight, g.convq.weight], 0)  # [3hd, hd + 64 + 82, 3, 3]
        w = _Weights()
        w.cor = ((_cl(e.convc1.weight), e.convc1.bias),)
        w.flo = ((_cl(_pad_in(e.convf1.weight, 2)), e.convf1.bias), (_cl(e.convf2.weight), e.convf2.bias))   # flow's 2 channels -> 4
        w.m = (_cl(e.conv.weight), e.conv.bias)
        w.gh = _cl(stack[:2 * hd, :hd])
        w.gq = _cl(stack[2 * hd:, :hd])
        w.gc = (_cl(stack[:, hd:hd + CTX_DIM]), torch.cat([g.convz.bias, g.convr.bias, g.convq.bias]))
        w.gx = _cl(_pad_in(stack[:, hd + CTX_DIM:], 2))                         # motion's 82 channels -> 84
        w.h1 = (_cl(f.conv1.weight), f.conv1.bias)
        w.h2 = (_cl(f.conv2.weight), f.conv2.bias)
        return w, [p[0] for p in w.cor + w.flo + (w.m, w.h1, w.h2)] + [w.gh, w.gq, w.gc[0], w.gc[1], w.gx]

    def _context_conv(self, inp, weight, bias):
        """The hoisted convolution itself (tests count its calls)."""
        return conv.conv2d(inp, weight, bias, padding=1)

    def _context_terms(self, inp, w):
        """c = conv(inp) + biases of the three gates, [B, 3hd, H, W]."""
        return self._context_conv(inp, *w.gc)

    def forward(self, net, inp, corr, flow):
        w, c, net, out, flow4 = self._enter(net, inp, corr, flow)
        motion = torch.cat([out, flow4], 1)                 # the flow's two zero channels close the 80 + 2 motion channels to 84
        # ConvGRU (update.py:23-31), split by input block
        a_x = conv.conv2d(motion, w.gx, None, padding=1)
        a_h = conv.conv2d(net, w.gh, None, padding=1)
        net = conv_gru(a_h, a_x, c, net, lambda rh: conv.conv2d(rh, w.gq, None, padding=1))
        return net, None, self._flow_head(w, net)


# ---- the full-size block -------------------------------------------------------------------------------------------------------
class _ShiftStack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, axis):
        x = aligned(x.detach(), CL)
        B, Cn, H, W = x.shape
        out = torch.empty((B, H, W, 5 * Cn), device=x.device, dtype=torch.float32)
        check(_lib.lib().dvs_shift_stack_fwd(x.data_ptr(), out.data_ptr(), B, H, W, Cn, axis, _lib.stream()), "dvs_shift_stack_fwd")
        ctx.geometry = (B, Cn, H, W, axis)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        B, Cn, H, W, axis = ctx.geometry
        g = aligned(g, CL)
        dx = torch.empty((B, H, W, Cn), device=g.device, dtype=torch.float32)
        check(_lib.lib().dvs_shift_stack_bwd(g.data_ptr(), dx.data_ptr(), B, H, W, Cn, axis, _lib.stream()), "dvs_shift_stack_bwd")
        return dx.permute(0, 3, 1, 2), None


def shift_stack(x, axis):
    """[B,5C,H,W] (channels_last memory) with channel t*C + c = x[:, c] moved by t - 2 along W (axis 0) or H (axis 1), zeros
    outside: a (1,5) / (5,1) convolution of x, padding (0,2) / (2,0), is the 1x1 convolution of this tensor with
    stacked_filter(weight).  fp32 GPU tensors, C % 4 == 0; differentiable."""
    gpu_arg("shift_stack", x, "[B,C,H,W] with C % 4 == 0 expected", ok=lambda s: s[1] % 4 == 0 and min(s) >= 1)
    if axis not in (0, 1):
        raise DvsError("shift_stack: axis=%r must be 0 (taps along W) or 1 (taps along H)" % (axis,))
    return _ShiftStack.apply(x, int(axis))


def stacked_filter(weight):
    """The [Cout, 5*Cin, 1, 1] filter over shift_stack(x, axis) of a [Cout,Cin,1,5] (axis 0) or [Cout,Cin,5,1] (axis 1) filter:
    input channel t*Cin + c is tap t of channel c.  A differentiable re-layout."""
    co, ci, kh, kw = weight.shape
    if (kh, kw) == (1, 5):
        return weight.permute(0, 3, 2, 1).reshape(co, 5 * ci, 1, 1)
    if (kh, kw) == (5, 1):
        return weight.permute(0, 2, 3, 1).reshape(co, 5 * ci, 1, 1)
    raise DvsError("stacked_filter: a (1,5) or (5,1) filter expected, got %s" % (tuple(weight.shape),))


def split_gru_filters(wz, wr, wq, bz, br, bq, hidden, ctx):
    """The SepConvGRU pass's three filters over cat[h(hidden), inp(ctx), motion] cut by input block and stacked by gate, each as
    the stacked 1x1 filter: (gh [2hd] on stack(h), gq [hd] on stack(r*h), gc [3hd] on stack(inp), bias [3hd], gx [3hd] on
    stack(motion))."""
    stack = torch.cat([wz, wr, wq], 0)
    cut = lambda t: _cl(stacked_filter(t))
    return (cut(stack[:2 * hidden, :hidden]), cut(stack[2 * hidden:, :hidden]), cut(stack[:, hidden:hidden + ctx]),
            torch.cat([bz, br, bq]), cut(stack[:, hidden + ctx:]))


class _BasicWeights:
    """The kernels' view of BasicUpdateBlock's parameters; gru[axis] = split_gru_filters of that pass."""
    __slots__ = ("cor", "flo", "m", "gru", "h1", "h2", "m1", "m2")


class BasicUpdateBlock(_UpdateBlock):
    """update.py:114-136 with the reference's parameter names: encoder.{convc1,convc2,convf1,convf2,conv},
    gru.{convz1,convr1,convq1,convz2,convr2,convq2}, flow_head.{conv1,conv2}, mask.{0,2}, each .weight / .bias.

    SepConvGRU is the split of the module docstring, twice: a horizontal pass whose (1,5) filters act on shift_stack(., 0) and a
    vertical pass whose (5,1) filters act on shift_stack(., 1), every contraction a 1x1 convolution with K = 5 * 128 on
    conv.conv2d.  Both passes' context terms are hoisted.  forward returns (net, mask, delta_flow); mask is the RAW output of the
    mask head, [B,576,H,W] in channels_last memory: the reference's 0.25 is raft.upsample_flow's mask_scale."""
    CTX, GATE = 128, "convz1"
    MASK_SCALE = 0.25       # update.py:135

    def __init__(self, hidden_dim=128, corr_levels=4, corr_radius=4):
        super().__init__(hidden_dim, corr_levels, corr_radius)

    def _layout(self, hidden, planes):
        if hidden != 128:
            raise DvsError("BasicUpdateBlock: hidden_dim=%d: the motion encoder's 128 channels and FlowHead(128, 256) fix it at 128 "
                           "(raft.py:134)" % hidden)
        gin = hidden + self.CTX + 128
        return {"encoder": [("convc1", 256, planes, 1, 0), ("convc2", 192, 256, 3, 1), ("convf1", 128, 2, 7, 3),
                            ("convf2", 64, 128, 3, 1), ("conv", 126, 256, 3, 1)],
                "gru": [(n + "1", hidden, gin, (1, 5), (0, 2)) for n in ("convz", "convr", "convq")]
                       + [(n + "2", hidden, gin, (5, 1), (2, 0)) for n in ("convz", "convr", "convq")],
                "flow_head": [("conv1", 256, hidden, 3, 1), ("conv2", 2, 256, 3, 1)],
                "mask": [("0", 256, 128, 3, 1), ("2", 576, 256, 1, 0)]}

    def _operands(self):
        e, g, f = self.encoder, self.gru, self.flow_head
        m0, m2 = getattr(self.mask, "0"), getattr(self.mask, "2")
        w = _BasicWeights()
        w.cor = ((_cl(e.convc1.weight), e.convc1.bias), (_cl(e.convc2.weight), e.convc2.bias))
        w.flo = ((_cl(_pad_in(e.convf1.weight, 2)), e.convf1.bias), (_cl(e.convf2.weight), e.convf2.bias))   # flow's 2 channels -> 4
        # 126 outputs -> 128: two zero filters (and zero biases) whose relu(0) = 0 channels make room for the flow
        w.m = (_cl(F.pad(e.conv.weight, (0, 0, 0, 0, 0, 0, 0, 2))), F.pad(e.conv.bias, (0, 2)))
        w.gru = tuple(split_gru_filters(*(getattr(g, n + s).weight for n in ("convz", "convr", "convq")),
                                        *(getattr(g, n + s).bias for n in ("convz", "convr", "convq")), self.hidden_dim, self.CTX)
                      for s in ("1", "2"))
        w.h1 = (_cl(f.conv1.weight), f.conv1.bias)
        w.h2 = (_cl(f.conv2.weight), f.conv2.bias)
        w.m1 = (_cl(m0.weight), m0.bias)
        w.m2 = (_cl(m2.weight), m2.bias)
        return w, [p[0] for p in w.cor + w.flo + (w.m, w.h1, w.h2, w.m1, w.m2)] + [w.m[1], *w.gru[0], *w.gru[1]]

    def _context_conv(self, stacked_inp, weight, bias):
        """One pass's hoisted convolution itself (tests count its calls)."""
        return conv.conv2d(stacked_inp, weight, bias)

    def _context_terms(self, inp, w):
        """(c of the horizontal pass, c of the vertical pass), each conv(stack(inp)) + the three biases, [B, 3hd, H, W]."""
        return tuple(self._context_conv(shift_stack(inp, axis), w.gru[axis][2], w.gru[axis][3]) for axis in (0, 1))

    def forward(self, net, inp, corr, flow, upsample=True):
        w, c, net, out, flow4 = self._enter(net, inp, corr, flow)
        motion = torch.cat([out[:, :126], flow4[:, :2]], 1)     # `out` has 128 channels, the last two zero: the flow takes their place
        # SepConvGRU (update.py:45-60): horizontal, then vertical
        for axis in (0, 1):
            gh, gq, _, _, gx = w.gru[axis]
            a_x = conv.conv2d(shift_stack(motion, axis), gx, None)
            a_h = conv.conv2d(shift_stack(net, axis), gh, None)
            net = conv_gru(a_h, a_x, c[axis], net, lambda rh: conv.conv2d(shift_stack(rh, axis), gq, None))
        delta_flow = self._flow_head(w, net)
        mask = conv.conv2d(conv.conv2d(net, *w.m1, padding=1, act="relu"), *w.m2) if upsample else None
        return net, mask, delta_flow
