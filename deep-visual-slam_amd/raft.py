"""SmallRAFT and RAFT end to end on the device (model/raft/core/raft.py:23-119 and 122-244): the two encoders (raft_encoder), the
correlation block (raft_corr), the update block (raft_update), upflow8 (csrc/upflow.hip) and, for the full-size model, the convex
upsampling upsample_flow (csrc/convexup.hip); RAFT's own usage is in its docstring.

    raft = SmallRAFT(); raft.load_state_dict(torch.load("raft-small.pth")); raft = raft.cuda()
    flows = raft(image1, image2, iters=12)              # list of 12 [B,2,H,W] flows, images in 0 .. 1
    flow = raft(image1, image2, last_only=True)[-1]     # only the final flow is upsampled (an extension)
    feat = raft.encode_frame(image4)                    # one frame's (fmap, net, inp); image4 is dvs_frame_ingest's output
    flows = raft.refine(feat1, feat2, iters=12)         # forward's result for the pair, each frame encoded once (raft_video.FlowStream)
    flows = raft.refine_pair(feat1, feat2, iters=12)    # both directions as one loop at batch 2N: rows [0:N] forward, [N:2N] backward

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
from ._raft_host import CL, aligned, gpu_arg
from .raft_corr import AlternateCorrBlock, CorrBlock
from .raft_encoder import BasicEncoder, SmallEncoder
from .raft_update import BasicUpdateBlock, SmallUpdateBlock


def _flow_layout(t):
    """(tensor whose memory the kernels read in place, planar flag) of a [N,2,h,w] tensor."""
    if t.is_contiguous():
        return aligned(t), 1
    return aligned(t, CL), 0


def _is_flow(shape):
    return shape[1] == 2 and min(shape) >= 1


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
        dout = aligned(dout)
        if nchw:
            dflow = torch.empty((N, 2, h, w), device=dout.device, dtype=torch.float32)
        else:
            dflow = torch.empty((N, h, w, 2), device=dout.device, dtype=torch.float32)
        check(_lib.lib().dvs_upflow8_bwd(dout.data_ptr(), dflow.data_ptr(), N, h, w, nchw, _lib.stream()), "dvs_upflow8_bwd")
        return dflow if nchw else dflow.permute(0, 3, 1, 2)


def upflow8(flow):
    """8 * F.interpolate(flow, 8x, mode='bilinear', align_corners=True) of a [N,2,h,w] fp32 GPU tensor in planar or channels_last
    memory (utils/utils.py:80-82); planar [N,2,8h,8w] out.  Differentiable; both directions repeat bit for bit."""
    gpu_arg("upflow8", flow, "[N,2,h,w] expected", ok=_is_flow)
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


class _ConvexUp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, mask, mask_scale):
        flow, mask = aligned(flow.detach()), aligned(mask.detach(), CL)
        N, _, h, w = flow.shape
        out = torch.empty((N, 2, 8 * h, 8 * w), device=flow.device, dtype=torch.float32)
        check(_lib.lib().dvs_convex_up_fwd(flow.data_ptr(), mask.data_ptr(), out.data_ptr(), N, h, w, mask_scale, _lib.stream()),
              "dvs_convex_up_fwd")
        ctx.save_for_backward(flow, mask)
        ctx.mask_scale = mask_scale
        return out

    @staticmethod
    def backward(ctx, dout):
        flow, mask = ctx.saved_tensors
        N, _, h, w = flow.shape
        need_flow, need_mask = ctx.needs_input_grad[:2]
        if not (need_flow or need_mask):
            return None, None, None
        dout = aligned(dout)
        dflow = ws = dmask = None
        nbytes = 0
        if need_flow:                                       # the workspace and the gather kernel serve dflow alone
            dflow = torch.empty_like(flow)
            nbytes = int(_lib.lib().dvs_convex_up_workspace(N, h, w))
            ws = torch.empty(nbytes, device=flow.device, dtype=torch.uint8)
        if need_mask:
            dmask = torch.empty((N, h, w, 576), device=flow.device, dtype=torch.float32)
        p = lambda t: t.data_ptr() if t is not None else None
        check(_lib.lib().dvs_convex_up_bwd(dout.data_ptr(), flow.data_ptr(), mask.data_ptr(), p(dflow), p(dmask), p(ws), nbytes, N, h, w,
                                           ctx.mask_scale, _lib.stream()), "dvs_convex_up_bwd")
        return dflow, dmask.permute(0, 3, 1, 2) if need_mask else None, None


def upsample_flow(flow, mask, mask_scale=1.0):
    """RAFT.upsample_flow (raft.py:170-181): the convex combination of the 3x3 neighbourhood of 8 * flow, [N,2,h,w], under
    softmax(mask_scale * mask) over the nine taps of mask [N,576,h,w] (channels_last memory is read in place); planar [N,2,8h,8w]
    out.  The reference hands in 0.25 * mask; here the raw mask head output and mask_scale=0.25 save that pass.  Differentiable in
    flow and mask; both directions repeat bit for bit."""
    gpu_arg("upsample_flow: flow", flow, "[N,2,h,w] expected", ok=_is_flow)
    gpu_arg("upsample_flow: mask", mask)
    N, _, h, w = flow.shape
    if tuple(mask.shape) != (N, 576, h, w) or mask.device != flow.device:
        raise DvsError("upsample_flow: mask must be [%d,576,%d,%d] on %s, got %s on %s"
                       % (N, h, w, flow.device, tuple(mask.shape), mask.device))
    return _ConvexUp.apply(flow, mask, float(mask_scale))


class NoRaftArgs(DvsError, NotImplementedError):
    """RAFT(None): a DvsError like every input error of this package, and a NotImplementedError because that is what the name
    RAFT raised while the full-size model was not built (the precedent of raft_corr.NoCpuPath)."""


class _RaftBase(nn.Module):
    """What SmallRAFT and RAFT share: the input checks, the forward loop and the one upsampling launch behind it."""

    def _check(self, image1, image2, iters, flow_init):
        who = type(self).__name__
        for name, t in (("image1", image1), ("image2", image2)):
            gpu_arg("%s: %s" % (who, name), t, "[B,3,H,W] expected", ok=lambda shape: shape[1] == 3)
        if image1.shape != image2.shape or image1.device != image2.device:
            raise DvsError("%s: image1 %s on %s, image2 %s on %s"
                           % (who, tuple(image1.shape), image1.device, tuple(image2.shape), image2.device))
        B, _, H, W = image1.shape
        self._check_size(who, H, W)
        self._check_rest(who, B, H, W, image1.device, iters, flow_init)

    @staticmethod
    def _check_size(who, H, W):
        if H % 8 or W % 8 or H < 128 or W < 128:
            raise DvsError("%s: images must be multiples of 8 and at least 128x128 (the 4-level correlation pyramid needs "
                           "16x16 features), got %dx%d" % (who, H, W))

    @staticmethod
    def _check_rest(who, B, H, W, device, iters, flow_init):
        if int(iters) < 1:
            raise DvsError("%s: iters=%r must be at least 1" % (who, iters))
        if flow_init is not None:
            if (not torch.is_tensor(flow_init) or flow_init.device != device or flow_init.dtype != torch.float32
                    or tuple(flow_init.shape) != (B, 2, H // 8, W // 8)):
                raise DvsError("%s: flow_init must be a fp32 [%d,2,%d,%d] tensor on %s" % (who, B, H // 8, W // 8, device))

    def _iterate(self, image1, image2, iters, flow_init, want_mask=None):
        """raft.py:76-117 and 183-239 up to the upsampling: (the 1/8-resolution flow of every iteration, the update block's mask
        of every iteration).  want_mask(it, iters) decides whether iteration `it` runs the block's mask head; None is for a
        block without one."""
        self._check(image1, image2, iters, flow_init)
        image1 = 2 * image1 - 1.0
        image2 = 2 * image2 - 1.0
        fmap1, fmap2 = self.fnet([image1, image2])
        return self._loop(fmap1, fmap2, lambda: self._context(self.cnet(image1)), iters, flow_init, want_mask)

    def _context(self, c):
        """(net, inp) of the context encoder's output, in the memory the update block takes."""
        net, inp = torch.split(c, [self.hidden_dim, self.context_dim], dim=1)
        net = conv._nhwc(torch.tanh(net))
        inp = conv._nhwc(torch.relu(inp))                   # made once: the update block's hoisted terms are keyed on this object
        return net, inp

    def _loop(self, fmap1, fmap2, context, iters, flow_init, want_mask):
        """The correlation block on (fmap1, fmap2), then context() -> (net, inp), then `iters` update steps."""
        iters = int(iters)
        block = AlternateCorrBlock if self.alternate_corr else CorrBlock
        corr_fn = block(fmap1, fmap2, num_levels=self.corr_levels, radius=self.corr_radius)
        net, inp = context()
        B, _, h, w = fmap1.shape
        coords0 = coords_grid(B, h, w, fmap1.device)
        coords1 = coords0
        if flow_init is not None:
            coords1 = coords1 + flow_init
        flows, masks = [], []
        for it in range(iters):
            coords1 = coords1.detach()
            corr = corr_fn(coords1, memory_format=CL)
            flow = coords1 - coords0
            options = {} if want_mask is None else {"upsample": want_mask(it, iters)}
            net, mask, delta_flow = self.update_block(net, inp, corr, flow, **options)
            coords1 = coords1 + delta_flow
            flows.append(coords1 - coords0)
            masks.append(mask)
        self.flow_low = [f.detach() for f in flows]         # the 1/8-resolution flows of the last call (RAFT's test_mode output)
        return flows, masks

    # ---- one frame at a time: a sequence encodes every frame once (raft_video.FlowStream) ----------------------------------------
    def encode_frame(self, image4):
        """The features of ONE frame batch: a namespace (fmap = fnet(frame); net, inp = the tanh / relu halves of cnet(frame), in
        the memory the update block takes).  image4 is conv1's own operand, [N,4,H,W] in NHWC memory: the frame as 2 * x - 1 with a
        zero fourth channel, which dvs_frame_ingest writes.  fnet's instance norm is per image and cnet has no norm (SmallRAFT) or
        a BatchNorm on its running statistics in eval() (RAFT), so the features of a frame do not depend on its partner."""
        who = type(self).__name__
        gpu_arg("%s.encode_frame: image4" % who, image4, "[N,4,H,W] expected", ok=lambda shape: shape[1] == 4)
        self._check_size(who + ".encode_frame", *image4.shape[2:])
        fmap = self.fnet(image4, _image4_operand=True)
        net, inp = self._context(self.cnet(image4, _image4_operand=True))
        return SimpleNamespace(fmap=fmap, net=net, inp=inp)

    def _check_feats(self, who, feat1, feat2, context_of):
        """The checks of refine / refine_pair: both frames' three tensors on the GPU, equal fmap shapes, and net / inp of every
        frame in `context_of` belonging to its fmap.  Returns the fmap shape."""
        for name, f in (("feat1", feat1), ("feat2", feat2)):
            for field in ("fmap", "net", "inp"):
                gpu_arg("%s: %s.%s" % (who, name, field), getattr(f, field, None), "[N,C,h,w] expected")
        f1, f2 = feat1.fmap, feat2.fmap
        if f1.shape != f2.shape or f1.device != f2.device:
            raise DvsError("%s: feat1.fmap %s on %s, feat2.fmap %s on %s" % (who, tuple(f1.shape), f1.device, tuple(f2.shape), f2.device))
        B, _, h, w = f1.shape
        for name, f in context_of:
            if (tuple(f.net.shape) != (B, self.hidden_dim, h, w) or tuple(f.inp.shape) != (B, self.context_dim, h, w)
                    or f.net.device != f1.device or f.inp.device != f1.device):
                raise DvsError("%s: %s.net %s / %s.inp %s do not belong to %s.fmap %s (encode_frame makes all three)"
                               % (who, name, tuple(f.net.shape), name, tuple(f.inp.shape), name, tuple(f1.shape)))
        return B, h, w

    def _refine(self, feat1, feat2, iters, flow_init, want_mask=None):
        who = type(self).__name__ + ".refine"
        B, h, w = self._check_feats(who, feat1, feat2, (("feat1", feat1),))
        f1, f2 = feat1.fmap, feat2.fmap
        self._check_rest(who, B, 8 * h, 8 * w, f1.device, iters, flow_init)
        return self._loop(f1, f2, lambda: (feat1.net, feat1.inp), iters, flow_init, want_mask)

    def _refine_pair(self, feat1, feat2, iters, flow_init, want_mask=None):
        """Both directions as ONE loop at batch 2N: rows 0 .. N-1 are (feat1 -> feat2), rows N .. 2N-1 are (feat2 -> feat1).  The
        concatenated `inp` is one tensor object for the whole call, so the update block hoists its context terms once; a new call
        makes a new object, which the block's cache (keyed on the object and its _version) sees as new, also under graph capture."""
        who = type(self).__name__ + ".refine_pair"
        B, h, w = self._check_feats(who, feat1, feat2, (("feat1", feat1), ("feat2", feat2)))
        f1, f2 = feat1.fmap, feat2.fmap
        self._check_rest(who, 2 * B, 8 * h, 8 * w, f1.device, iters, flow_init)
        net, inp = torch.cat((feat1.net, feat2.net), 0), torch.cat((feat1.inp, feat2.inp), 0)
        return self._loop(torch.cat((f1, f2), 0), torch.cat((f2, f1), 0), lambda: (net, inp), iters, flow_init, want_mask)

    def _upsampled(self, flows, masks, only_last):
        """The list of full-resolution flows, of the last iteration alone or of all of them by ONE launch (N = iters * B): upflow8
        (utils/utils.py:80-82) without masks, the update block's convex upsampling with them."""
        pick = (lambda ts: ts[-1]) if only_last else (lambda ts: torch.cat(ts, 0))
        if masks is None:
            up = upflow8(pick(flows))
        else:
            up = upsample_flow(pick(flows), pick(masks), self.update_block.MASK_SCALE)
        return [up] if only_last else list(torch.split(up, flows[0].shape[0], dim=0))


class RAFT(_RaftBase):
    """The full-size model (raft.py:122-244): BasicEncoder('instance') and BasicEncoder('batch'), the radius-4 correlation block,
    BasicUpdateBlock and the convex upsampling (csrc/convexup.hip).

        raft = RAFT({"small": False}); raft.load_state_dict(torch.load("raft-things.pth")); raft = raft.cuda().eval()
        flow_low, flow_up = raft(image1, image2, iters=20, test_mode=True)      # images in 0 .. 1
        flows = raft(image1, image2, iters=12)                                  # every iteration's flow, upsampled in one launch

    `args` is a namespace or a dict (small, alternate_corr, mixed_precision, dropout).  test_mode and last_only (an extension) run
    the mask head and the upsampling at the last iteration only.  GPU and fp32 only."""

    def __init__(self, args):
        if args is None:
            raise NoRaftArgs("RAFT: args are required (a namespace or a dict: small=False, alternate_corr, ...), as the reference "
                             "requires them; RAFT({'small': False}) builds the full-size model")
        if _option(args, "small", False):
            raise DvsError("RAFT: small=True is SmallRAFT in this package: use raft.SmallRAFT(args)")
        if _option(args, "mixed_precision", False):
            raise DvsError("RAFT: mixed_precision=True is not built: the kernels are fp32; use _lib.set_precision('bf16') for bf16 "
                           "matrix-core convolutions")
        dropout = _option(args, "dropout", 0) or 0
        if dropout > 0:
            raise DvsError("RAFT: dropout=%r is not built: use dropout=0 (the released checkpoints were trained without)" % (dropout,))
        super().__init__()
        self.args = args
        self.hidden_dim, self.context_dim = 128, 128
        self.corr_levels, self.corr_radius = 4, 4
        self.alternate_corr = bool(_option(args, "alternate_corr", False))
        self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=0.0)
        self.cnet = BasicEncoder(output_dim=self.hidden_dim + self.context_dim, norm_fn="batch", dropout=0.0)
        self.update_block = BasicUpdateBlock(hidden_dim=self.hidden_dim, corr_levels=self.corr_levels, corr_radius=self.corr_radius)

    def freeze_bn(self):
        """raft.py:156-159: every BatchNorm2d (the context encoder's) uses its running statistics from here on."""
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    def _outputs(self, iterate, upsample, test_mode, last_only):
        only_last = bool(test_mode or last_only)
        flows, masks = iterate(lambda it, n: bool(upsample) and (not only_last or it == n - 1))
        # upsample=False is the block's: no mask, bilinear upflow8 as raft.py:234-235
        up = self._upsampled(flows, masks if upsample else None, only_last)
        if test_mode:
            return flows[-1], up[-1]
        return up

    def forward(self, image1, image2, iters=12, flow_init=None, upsample=True, test_mode=False, last_only=False):
        return self._outputs(lambda want_mask: self._iterate(image1, image2, iters, flow_init, want_mask), upsample, test_mode, last_only)

    def refine(self, feat1, feat2, iters=12, flow_init=None, upsample=True, test_mode=False, last_only=False):
        """What forward returns for the pair whose frames encode_frame made feat1 and feat2 of: the correlation block on their
        fmaps, the loop on feat1.net / feat1.inp, the upsampling."""
        return self._outputs(lambda want_mask: self._refine(feat1, feat2, iters, flow_init, want_mask), upsample, test_mode, last_only)

    def refine_pair(self, feat1, feat2, iters=12, flow_init=None, upsample=True, test_mode=False, last_only=False):
        """Both directions of the pair by ONE loop at batch 2N: what refine returns at batch 2N, rows 0 .. N-1 = refine(feat1,
        feat2), rows N .. 2N-1 = refine(feat2, feat1); flow_init is [2N,2,h,w] in that order or None.  Equal to the two refine
        calls mathematically, not bit for bit: a convolution's route may differ with the batch."""
        return self._outputs(lambda want_mask: self._refine_pair(feat1, feat2, iters, flow_init, want_mask), upsample, test_mode, last_only)


class SmallRAFT(_RaftBase):
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

    def forward(self, image1, image2, iters=12, flow_init=None, last_only=False):
        flows, _ = self._iterate(image1, image2, iters, flow_init)
        return self._upsampled(flows, None, last_only)

    def refine(self, feat1, feat2, iters=12, flow_init=None, last_only=False):
        """What forward returns for the pair whose frames encode_frame made feat1 and feat2 of."""
        flows, _ = self._refine(feat1, feat2, iters, flow_init)
        return self._upsampled(flows, None, last_only)

    def refine_pair(self, feat1, feat2, iters=12, flow_init=None, last_only=False):
        """Both directions of the pair by ONE loop at batch 2N: what refine returns at batch 2N, rows 0 .. N-1 = refine(feat1,
        feat2), rows N .. 2N-1 = refine(feat2, feat1); flow_init is [2N,2,h,w] in that order or None.  Equal to the two refine
        calls mathematically, not bit for bit: a convolution's route may differ with the batch."""
        flows, _ = self._refine_pair(feat1, feat2, iters, flow_init)
        return self._upsampled(flows, None, last_only)
