"""RAFT on video, on the device: what the reference's flow demo and RAFT's video protocol do around a forward.

    forward_interpolate(flow)      utils/utils.py:26-54: the previous pair's 1/8-resolution flow pushed forward = the next flow_init
    flow_to_image(flow, ...)       utils/flow_viz.py:109-132: the colour-wheel picture of a flow, uint8
    InputPadder(dims, mode)        utils/utils.py:7-24: replicate padding to multiples of 8, and the view that undoes it
    FlowPredictor(model, ...)      pad -> model(test_mode) -> warm start -> un-pad -> colour, one call per frame pair

    pred = FlowPredictor(raft.RAFT({"small": False}).cuda().eval(), iters=12)
    for frame1, frame2 in pairs:                       # [B,3,H,W] fp32 in 0 .. 1 on the GPU, any H, W the padded model accepts
        r = pred(frame1, frame2)                       # r.flow_up [B,2,H,W] (a view), r.flow_low, r.image [B,H,W,3] uint8
    pred.reset()                                       # a new sequence: drop the kept flow

forward_interpolate and flow_to_image are csrc/flowstage.hip (include/dvslam.h states their arithmetic); nothing here copies to
the host or synchronises.  Padding is F.pad and a slice: not hot, it stays ATen.  GPU and fp32 only.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import DvsError, check
from ._raft_host import gpu_arg
from .raft import RAFT, SmallRAFT

MAX_POINTS = 65536          # dvs_forward_interp is a brute-force search: h * w sources per image at the most


def _flow_arg(who, flow, what):
    """A [2,h,w] or [N,2,h,w] fp32 GPU tensor as ([N,2,h,w] view, had a batch dimension)."""
    gpu_arg(who, flow, what + " expected", rank=(3, 4), ok=lambda shape: shape[-3] == 2 and min(shape) >= 1)
    batched = flow.dim() == 4
    return (flow if batched else flow[None]).detach(), batched


def forward_interpolate(flow):
    """utils/utils.py:26-54 on the device.  flow [2,h,w] (the reference's form) or [N,2,h,w], fp32, h * w <= 65536; the result has
    the same shape and stays on the device.  Every grid pixel takes the flow of the nearest source pixel after the sources moved
    by their own flow (fp64 distances, sources that leave the image dropped); of equally near sources the one with the lowest
    row-major index wins, where the reference's KD-tree defines no answer; an image none of whose sources stays inside returns
    zeros, where the reference has no flow to give (griddata on zero points: NaN under SciPy 1.15)."""
    f, batched = _flow_arg("forward_interpolate", flow, "[2,h,w] or [N,2,h,w]")
    N, _, h, w = f.shape
    if h * w > MAX_POINTS:
        raise DvsError("forward_interpolate: h * w = %d exceeds %d (a brute-force search; it is meant for the 1/8-resolution flow)"
                       % (h * w, MAX_POINTS))
    f = f.contiguous()
    out = torch.empty_like(f)
    check(_lib.lib().dvs_forward_interp(f.data_ptr(), out.data_ptr(), N, h, w, _lib.stream()), "dvs_forward_interp")
    return out if batched else out[0]


def _strided(f):
    """(tensor, plane stride, row stride) with which dvs_flow_to_image reads `f` [N,2,H,W]: `f` itself if it has unit stride along
    W, rows and planes that do not overlap and images two planes apart (every slice of a contiguous flow has), else a copy."""
    N, _, H, W = f.shape
    s0, s1, s2, s3 = f.stride()
    row = s2 if H > 1 else W
    if ((s3 == 1 or W == 1) and row >= W and s1 >= (H - 1) * row + W and (N == 1 or s0 == 2 * s1) and f.data_ptr() % 4 == 0):
        return f, s1, row
    f = f.contiguous()
    return f, H * W, W


def flow_to_image(flow, clip_flow=None, convert_to_bgr=False):
    """utils/flow_viz.py:109-132 on the device.  flow [2,H,W] or [N,2,H,W] fp32 (the model's layout; a view such as
    InputPadder.unpad's is read in place); uint8 [H,W,3] or [N,H,W,3] out, every image normalised by its own largest radius."""
    f, batched = _flow_arg("flow_to_image", flow, "[2,H,W] or [N,2,H,W]")
    clip = -1.0
    if clip_flow is not None:
        clip = float(clip_flow)
        if not clip >= 0.0:
            raise DvsError("flow_to_image: clip_flow=%r must be None or at least 0 (the flow is clipped to 0 .. clip_flow)" % (clip_flow,))
    f, plane, row = _strided(f)
    N, _, H, W = f.shape
    radmax = torch.empty((N,), device=f.device, dtype=torch.float32)
    out = torch.empty((N, H, W, 3), device=f.device, dtype=torch.uint8)
    lib, st = _lib.lib(), _lib.stream()
    check(lib.dvs_flow_radmax(f.data_ptr(), plane, row, N, H, W, clip, radmax.data_ptr(), st), "dvs_flow_radmax")
    check(lib.dvs_flow_to_image(f.data_ptr(), plane, row, radmax.data_ptr(), out.data_ptr(), N, H, W, clip, int(bool(convert_to_bgr)), st),
          "dvs_flow_to_image")
    return out if batched else out[0]


class InputPadder:
    """utils/utils.py:7-24: pads images so that both sides are multiples of 8 -- 'sintel': split between both ends of each side;
    any other mode (the reference's 'kitti'): split along the width, all at the bottom along the height."""

    def __init__(self, dims, mode="sintel"):
        self.ht, self.wd = (int(d) for d in dims[-2:])
        pad_ht = (((self.ht // 8) + 1) * 8 - self.ht) % 8
        pad_wd = (((self.wd // 8) + 1) * 8 - self.wd) % 8
        if mode == "sintel":
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]
        else:
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]

    def pad(self, *inputs):
        return [F.pad(x, self._pad, mode="replicate") for x in inputs]

    def unpad(self, x):
        """The window of `x` [..., Hp, Wp] that the padding surrounds: a view."""
        ht, wd = x.shape[-2:]
        left, right, top, bottom = self._pad
        return x[..., top:ht - bottom, left:wd - right]


class FlowPredictor:
    """One call per frame pair around SmallRAFT or RAFT in eval mode: replicate-pad, run the model under no_grad in test mode,
    keep forward_interpolate(flow_low) as the next call's flow_init (warm_start), un-pad, colour (image).

    __call__ / pred(image1, image2) returns a namespace: flow_low [B,2,Hp/8,Wp/8] at the padded size, flow_up [B,2,H,W] (a view of
    the padded flow), image uint8 [B,H,W,3] or None.  reset() starts a new sequence; a change of input shape without it raises."""

    def __init__(self, model, iters=20, warm_start=True, pad_mode="sintel", image=True, convert_to_bgr=False):
        if not isinstance(model, (RAFT, SmallRAFT)):
            raise DvsError("FlowPredictor: model must be a raft.RAFT or a raft.SmallRAFT, got %s" % type(model).__name__)
        if int(iters) < 1:
            raise DvsError("FlowPredictor: iters=%r must be at least 1" % (iters,))
        self.model, self.iters, self.warm_start, self.pad_mode = model, int(iters), bool(warm_start), pad_mode
        self.image, self.convert_to_bgr = bool(image), bool(convert_to_bgr)
        self.flow_init, self._shape = None, None

    def reset(self):
        self.flow_init, self._shape = None, None

    def _run(self, image1, image2):
        """(flow_low, flow_up) of the padded pair: RAFT has a test mode; SmallRAFT's counterpart is last_only and its flow_low."""
        if isinstance(self.model, RAFT):
            return self.model(image1, image2, iters=self.iters, flow_init=self.flow_init, test_mode=True)
        up = self.model(image1, image2, iters=self.iters, flow_init=self.flow_init, last_only=True)[-1]
        return self.model.flow_low[-1], up

    @torch.no_grad()
    def pred(self, image1, image2):
        if self.model.training:
            raise DvsError("FlowPredictor: the model is in train() mode; call model.eval() (inference runs BatchNorm on its running "
                           "statistics and keeps no graph)")
        for name, t in (("image1", image1), ("image2", image2)):
            gpu_arg("FlowPredictor: " + name, t, "[B,3,H,W] expected", ok=lambda shape: shape[1] == 3)
        if image1.shape != image2.shape or image1.device != image2.device:
            raise DvsError("FlowPredictor: image1 %s on %s, image2 %s on %s"
                           % (tuple(image1.shape), image1.device, tuple(image2.shape), image2.device))
        shape = (tuple(image1.shape), image1.device)
        if self._shape is not None and shape != self._shape:
            raise DvsError("FlowPredictor: input changed from %s on %s to %s on %s inside a sequence; call reset() first"
                           % (self._shape + shape))
        padder = InputPadder(image1.shape, self.pad_mode)
        a, b = padder.pad(image1, image2)
        flow_low, flow_pad = self._run(a, b)                # a padded size the model refuses: the model's own error
        self._shape = shape
        if self.warm_start:
            self.flow_init = forward_interpolate(flow_low)
        flow_up = padder.unpad(flow_pad)
        image = flow_to_image(flow_up, convert_to_bgr=self.convert_to_bgr) if self.image else None
        return SimpleNamespace(flow_low=flow_low, flow_up=flow_up, image=image)

    __call__ = pred
