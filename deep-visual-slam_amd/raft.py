"""SmallRAFT end to end on the device (model/raft/core/raft.py:23-119): the two encoders (raft_encoder), the correlation block
(raft_corr), the update block (raft_update) and upflow8 (csrc/upflow.hip).

    raft = SmallRAFT(); raft.load_state_dict(torch.load("raft-small.pth")); raft = raft.cuda()
    flows = raft(image1, image2, iters=12)              # list of 12 [B,2,H,W] flows, images in 0 .. 1
    flow = raft(image1, image2, last_only=True)[-1]     # only the final flow is upsampled (an extension)

Submodules are fnet, cnet and update_block with the reference's parameter names, so a raft-small.pth state dict loads with
load_state_dict(strict=True).  `inp` is made once and handed to the update block as the same tensor object in every iteration, so
its hoisted context convolution runs once per forward.  All `iters` low-resolution flows are upsampled by ONE upflow8 launch
(N = iters * B), and their gradients by one.  GPU and fp32 only; no host synchronisation in forward or backward.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import _lib, conv
from ._lib import DvsError, check
from .raft_corr import AlternateCorrBlock, CorrBlock
from .raft_encoder import SmallEncoder
from .raft_update import SmallUpdateBlock

CL = torch.channels_last


def _flow_layout(t):
    """(tensor whose memory the kernels read in place, planar flag) of a [N,2,h,w] tensor."""
    if t.is_contiguous():
        return t, 1
    if not t.is_contiguous(memory_format=CL):
        t = t.contiguous(memory_format=CL)
    return t, 0


class _Upflow8(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow):
        flow, nchw = _flow_layout(flow.detach())
        N, _, h, w = flow.shape
        out = torch.empty((N, 2, 8 * h, 8 * w), device=flow.device, dtype=torch.float32)
        check(_lib.lib().dvs_upflow8_fwd(flow.data_ptr(), out.data_ptr(), N, h, w, nchw, _lib.stream()), "dvs_upflow8_fwd")
        ctx.geometry = (N, h, w, nchw)
        return out

    @staticmethod
    def backward(ctx, dout):
        N, h, w, nchw = ctx.geometry
        dout = dout.contiguous()
        if nchw:
            dflow = torch.empty((N, 2, h, w), device=dout.device, dtype=torch.float32)
        else:
            dflow = torch.empty((N, h, w, 2), device=dout.device, dtype=torch.float32)
        check(_lib.lib().dvs_upflow8_bwd(dout.data_ptr(), dflow.data_ptr(), N, h, w, nchw, _lib.stream()), "dvs_upflow8_bwd")
        return dflow if nchw else dflow.permute(0, 3, 1, 2)


def upflow8(flow):
    """8 * F.interpolate(flow, 8x, mode='bilinear', align_corners=True) of a [N,2,h,w] fp32 GPU tensor in planar or channels_last
    memory (utils/utils.py:80-82); planar [N,2,8h,8w] out.  Differentiable; both directions repeat bit for bit."""
    if not torch.is_tensor(flow) or not flow.is_cuda:
        raise DvsError("upflow8: GPU tensors only (got %s); this package has no CPU path" % (getattr(flow, "device", type(flow)),))
    if flow.dtype != torch.float32:
        raise DvsError("upflow8: fp32 only, got %s" % flow.dtype)
    if flow.dim() != 4 or flow.shape[1] != 2 or flow.shape[0] < 1 or flow.shape[2] < 1 or flow.shape[3] < 1:
        raise DvsError("upflow8: [N,2,h,w] expected, got %s" % (tuple(flow.shape),))
    return _Upflow8.apply(flow)


def coords_grid(batch, ht, wd, device):
    """utils/utils.py:74-77: [batch, 2, ht, wd], channel 0 the x coordinate."""
    ys, xs = torch.meshgrid(torch.arange(ht, device=device), torch.arange(wd, device=device), indexing="ij")
    return torch.stack([xs, ys], dim=0).float()[None].repeat(batch, 1, 1, 1)


def _option(args, name, default):
    if args is None:
        return default
    if isinstance(args, dict):
        return args.get(name, default)
    return getattr(args, name, default)


class RAFT(nn.Module):
    """The full-size model (raft.py:122-244) is not built: BasicEncoder, SepConvGRU and the convex-upsampling mask head are missing."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("RAFT (BasicEncoder, SepConvGRU, mask head) is not built in this package; SmallRAFT is")


class SmallRAFT(nn.Module):
    def __init__(self, args=None):
        super().__init__()
        self.args = args if args is not None else SimpleNamespace()
        self.hidden_dim, self.context_dim = 96, 64
        self.corr_levels, self.corr_radius = 4, 3
        self.alternate_corr = bool(_option(args, "alternate_corr", False))
        self.fnet = SmallEncoder(output_dim=128, norm_fn="instance", dropout=0.0)
        self.cnet = SmallEncoder(output_dim=self.hidden_dim + self.context_dim, norm_fn="none", dropout=0.0)
        self.update_block = SmallUpdateBlock(hidden_dim=self.hidden_dim, corr_levels=self.corr_levels, corr_radius=self.corr_radius)

    def freeze_bn(self):
        """raft.py:38-41; there is no BatchNorm in SmallRAFT."""

    def _check(self, image1, image2, iters, flow_init):
        for name, t in (("image1", image1), ("image2", image2)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise DvsError("SmallRAFT: %s: GPU tensors only (got %s); this package has no CPU path"
                               % (name, getattr(t, "device", type(t))))
            if t.dtype != torch.float32:
                raise DvsError("SmallRAFT: %s: fp32 only, got %s" % (name, t.dtype))
            if t.dim() != 4 or t.shape[1] != 3:
                raise DvsError("SmallRAFT: %s: [B,3,H,W] expected, got %s" % (name, tuple(t.shape)))
        if image1.shape != image2.shape or image1.device != image2.device:
            raise DvsError("SmallRAFT: image1 %s on %s, image2 %s on %s"
                           % (tuple(image1.shape), image1.device, tuple(image2.shape), image2.device))
        B, _, H, W = image1.shape
        if H % 8 or W % 8 or H < 128 or W < 128:
            raise DvsError("SmallRAFT: images must be multiples of 8 and at least 128x128 (the 4-level correlation pyramid needs "
                           "16x16 features), got %dx%d" % (H, W))
        if int(iters) < 1:
            raise DvsError("SmallRAFT: iters=%r must be at least 1" % (iters,))
        if flow_init is not None:
            if (not torch.is_tensor(flow_init) or flow_init.device != image1.device or flow_init.dtype != torch.float32
                    or tuple(flow_init.shape) != (B, 2, H // 8, W // 8)):
                raise DvsError("SmallRAFT: flow_init must be a fp32 [%d,2,%d,%d] tensor on %s" % (B, H // 8, W // 8, image1.device))

    def forward(self, image1, image2, iters=12, flow_init=None, last_only=False):
        self._check(image1, image2, iters, flow_init)
        image1 = 2 * image1 - 1.0
        image2 = 2 * image2 - 1.0
        hdim, cdim = self.hidden_dim, self.context_dim
        fmap1, fmap2 = self.fnet([image1, image2])
        block = AlternateCorrBlock if self.alternate_corr else CorrBlock
        corr_fn = block(fmap1, fmap2, num_levels=self.corr_levels, radius=self.corr_radius)
        cnet = self.cnet(image1)
        net, inp = torch.split(cnet, [hdim, cdim], dim=1)
        net = conv._nhwc(torch.tanh(net))
        inp = conv._nhwc(torch.relu(inp))                   # made once: the update block's hoisted term is keyed on this object
        B, _, H, W = image1.shape
        coords0 = coords_grid(B, H // 8, W // 8, image1.device)
        coords1 = coords0
        if flow_init is not None:
            coords1 = coords1 + flow_init
        flows = []
        for _ in range(int(iters)):
            coords1 = coords1.detach()
            corr = corr_fn(coords1, memory_format=CL)
            flow = coords1 - coords0
            net, _, delta_flow = self.update_block(net, inp, corr, flow)
            coords1 = coords1 + delta_flow
            flows.append(coords1 - coords0)
        self.flow_low = [f.detach() for f in flows]         # the 1/8-resolution flows of the last call (RAFT's test_mode output)
        if last_only:
            return [upflow8(flows[-1])]
        return list(torch.split(upflow8(torch.cat(flows, 0)), B, dim=0))
