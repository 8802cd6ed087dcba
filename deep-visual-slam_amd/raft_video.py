"""RAFT on video, on the device: what the reference's flow demo and RAFT's video protocol do around a forward.

    forward_interpolate(flow)      utils/utils.py:26-54: the previous pair's 1/8-resolution flow pushed forward = the next flow_init
    flow_to_image(flow, ...)       utils/flow_viz.py:109-132: the colour-wheel picture of a flow, uint8
    InputPadder(dims, mode)        utils/utils.py:7-24: replicate padding to multiples of 8, and the view that undoes it
    FlowPredictor(model, ...)      pad -> model(test_mode) -> warm start -> un-pad -> colour, one call per frame pair
    frame_ingest(frame, pad)       csrc/ingest.hip: a uint8 frame as the encoders' first operand (/255, replicate pad, 2x - 1, NHWC)
    FlowStream(model, ...)         one push per uint8 frame: ingest -> encode once -> refine(previous, current) -> warm start -> colour;
                                   graph=True replays it as one HIP graph, host=True adds pinned host copies, bidirectional=True
                                   runs both directions as one loop at batch 2N and adds the two consistency masks
    flow_consistency(fw, bw, ...)  csrc/flowcons.hip: the forward-backward check of UnFlow, both validity masks by one launch
    rigid_flow(depth, T, K, ...)   csrc/rigidflow.hip: the flow a static scene shows under a depth map and a camera motion, and a
                                   static / moving label for a measured flow against it, by one launch
    RigidFlowStream(model, ...)    FlowStream whose push also takes depth, T, K, inv_K and adds rigid and motion to every pair
    fit_pose(depth, flow, K, ...)  csrc/posefit.hip: the camera motion that explains a measured flow under a depth map, by Gauss-Newton
                                   on SE(3) with Huber weights, two launches a step
    PoseFlowStream(model, ...)     RigidFlowStream that fits T to its own flow (two rounds: all pixels, then the static ones)

    pred = FlowPredictor(raft.RAFT({"small": False}).cuda().eval(), iters=12)
    for frame1, frame2 in pairs:                       # [B,3,H,W] fp32 in 0 .. 1 on the GPU, any H, W the padded model accepts
        r = pred(frame1, frame2)                       # r.flow_up [B,2,H,W] (a view), r.flow_low, r.image [B,H,W,3] uint8
    pred.reset()                                       # a new sequence: drop the kept flow

    stream = FlowStream(model, iters=12)               # graph=True by default: one HIP graph replay per frame
    for frame in frames:                               # uint8 [H,W,3] or [N,H,W,3], on the GPU or on the host
        r = stream.push(frame)                         # None for the first frame, then r.flow_up, r.flow_low, r.image (until the next push)

forward_interpolate and flow_to_image are csrc/flowstage.hip (include/dvslam.h states their arithmetic); nothing here synchronises
(host=True copies are asynchronous).  FlowPredictor's padding stays ATen: not hot.  GPU only; fp32 flows, uint8 frames and pictures.
"""
import copy
from functools import partial
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import _lib
from ._graph import CapturedStep, HostRing
from ._host import dense_view, gpu_arg, not_negative
from ._lib import DvsError, check
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


_rows = _planes = dense_view                # a flow [N,2,H,W]: image, plane and row stride; a depth [N,H,W]: image and row stride
_packed = partial(dense_view, inner=3)          # uint8 frames [N,H,W,3]: image and row stride in bytes


def _strided(f):
    """(tensor, plane stride, row stride) with which dvs_flow_to_image reads `f` [N,2,H,W]: the entry takes no image stride, so
    a batch whose images do not lie two planes apart is copied as well."""
    kept, image, plane, row = _rows(f)
    if f.shape[0] > 1 and image != 2 * plane:
        kept, image, plane, row = _rows(f.contiguous())
    return kept, plane, row


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


def flow_consistency(flow_fw, flow_bw, alpha=0.01, beta=0.5, excess=False):
    """The forward-backward check of UnFlow (Meister et al. 2018, eq. 2) on the device, both directions in ONE launch
    (dvs_flow_consistency; include/dvslam.h states the arithmetic).  flow_fw [2,H,W] or [N,2,H,W] fp32 on image 1's grid (image 1 ->
    image 2), flow_bw the same on image 2's grid (image 2 -> image 1).  Returns (valid_fw, valid_bw), uint8 [H,W] or [N,H,W]: 1 where

        |w + w'(x + w)|^2 <= alpha * (|w|^2 + |w'(x + w)|^2) + beta        w the pixel's own flow, w' the other flow, sampled bilinearly

    and x + w lies inside the image (closed border: a zero flow is valid everywhere), 0 where the pixel is occluded, leaves the
    image or holds a NaN.  excess=True: (valid_fw, valid_bw, excess_fw, excess_bw), the fp32 fields `left side - right side`
    (+inf where x + w is outside or the difference is NaN), so that a caller can apply a threshold of its own.  Views whose rows
    are dense (InputPadder.unpad's, a batch slice) are read in place through their strides; any other layout is copied once."""
    who = "flow_consistency"
    fw, batched = _flow_arg(who + ": flow_fw", flow_fw, "[2,H,W] or [N,2,H,W]")
    bw, _ = _flow_arg(who + ": flow_bw", flow_bw, "[2,H,W] or [N,2,H,W]")
    if fw.shape != bw.shape or fw.device != bw.device:
        raise DvsError("%s: flow_fw %s on %s, flow_bw %s on %s" % (who, tuple(fw.shape), fw.device, tuple(bw.shape), bw.device))
    alpha, beta = not_negative(who, alpha=alpha, beta=beta)
    fw, fw_image, fw_plane, fw_row = _rows(fw)
    bw, bw_image, bw_plane, bw_row = _rows(bw)
    N, _, H, W = fw.shape
    valid = torch.empty((2, N, H, W), device=fw.device, dtype=torch.uint8)
    over = torch.empty((2, N, H, W), device=fw.device, dtype=torch.float32) if excess else None
    p = lambda t, i: t[i].data_ptr() if t is not None else None
    check(_lib.lib().dvs_flow_consistency(fw.data_ptr(), fw_image, fw_plane, fw_row, bw.data_ptr(), bw_image, bw_plane, bw_row,
                                          p(valid, 0), p(valid, 1), p(over, 0), p(over, 1), N, H, W, alpha, beta, _lib.stream()),
          "dvs_flow_consistency")
    out = (valid[0], valid[1]) + ((over[0], over[1]) if excess else ())
    return out if batched else tuple(t[0] for t in out)


def _matrix_arg(who, m, N, single):
    """Refuse `m` unless it is an fp32 GPU [N,4,4] (or, with `single`, a [4,4] that stands for every image)."""
    want = "[%d,4,4]%s expected" % (N, " or [4,4]" if single else "")
    gpu_arg(who, m, want, rank=(2, 3) if single else 3, ok=lambda shape: tuple(shape) in ((N, 4, 4),) + (((4, 4),) if single else ()))


def _rigid_args(who, depth, T, K, inv_K, flow=None, valid=None, shape=None, T_name="T"):
    """The argument checks of rigid_flow, made on the tensors' descriptions alone (before any launch or copy); `shape`: the
    (N, H, W) the caller demands; T_name: what the caller calls T (None: it has none to check).  Returns (N, H, W)."""
    gpu_arg(who + ": depth", depth, "[N,1,H,W] or [N,H,W] expected", rank=(3, 4),
            ok=lambda s: min(s) >= 1 and (len(s) == 3 or s[1] == 1) and (shape is None or (s[0], s[-2], s[-1]) == tuple(shape)))
    N, H, W = depth.shape[0], depth.shape[-2], depth.shape[-1]
    if T_name is not None:
        _matrix_arg(who + ": " + T_name, T, N, False)
    _matrix_arg(who + ": K", K, N, True)
    if inv_K is not None:
        _matrix_arg(who + ": inv_K", inv_K, N, True)
    if flow is not None:
        gpu_arg(who + ": flow", flow, "[%d,2,%d,%d] expected" % (N, H, W), ok=lambda s: tuple(s) == (N, 2, H, W))
    if valid is not None:
        if not torch.is_tensor(valid) or not valid.is_cuda:
            raise DvsError("%s: valid: GPU tensors only (got %s); this package has no CPU path" % (who, getattr(valid, "device", type(valid))))
        if valid.dtype != torch.uint8 or tuple(valid.shape) != (N, H, W):
            raise DvsError("%s: valid: uint8 [%d,%d,%d] expected (the mask of flow_consistency), got %s %s"
                           % (who, N, H, W, valid.dtype, tuple(valid.shape)))
    for name, t in ((T_name, T), ("K", K), ("inv_K", inv_K), ("flow", flow), ("valid", valid)):
        if t is not None and t.device != depth.device:
            raise DvsError("%s: %s is on %s, depth on %s" % (who, name, t.device, depth.device))
    return N, H, W


def _geometry(N, depth, K, inv_K, flow, valid, pose, pose_first):
    """dvs_rigid_flow's and dvs_pose_fit's operands: depth view, dense [N,4,4] K, inv_K and pose, flow view, dense valid, pointer-or-None."""
    d = _planes(depth.detach() if depth.dim() == 3 else depth.detach()[:, 0])
    mat = lambda m: m.detach().expand(N, 4, 4).contiguous()
    pose, K = (mat(pose) if pose_first else pose), mat(K)       # before K or after inv_K: each caller's own order of copies, kept
    inv_K = mat(inv_K) if inv_K is not None else torch.linalg.inv(K).contiguous()
    if not pose_first:                                          # fit_pose: no guess is the identity
        pose = mat(pose) if pose is not None else torch.eye(4, device=d[0].device, dtype=torch.float32).repeat(N, 1, 1)
    f = _rows(flow.detach()) if flow is not None else (None, 0, 0, 0)
    return d, K, inv_K, pose, f, valid.contiguous() if valid is not None else None, lambda t: t.data_ptr() if t is not None else None


def rigid_flow(depth, T, K, inv_K=None, flow=None, valid=None, alpha=0.01, beta=0.5, eps=1e-7, excess=False):
    """The flow a STATIC scene shows under this depth and this camera motion, and where a measured flow disagrees with it, on the
    device in ONE launch (dvs_rigid_flow; include/dvslam.h states the arithmetic): the reference's BackprojectDepth and Project3D
    (vo/learner_func.py:106-159) in pixel coordinates, rigid = project(K T backproject(depth, inv_K)) - (x, y).

    depth [N,1,H,W] or [N,H,W] fp32, of the flow's SOURCE frame; T [N,4,4] maps points of that camera into the target camera;
    K and inv_K [4,4] or [N,4,4] (the reference's 4x4 intrinsics).  inv_K=None inverts K once with torch.linalg.inv on the device:
    the bit-for-bit contract of the entry holds for an inv_K that the caller passes.  Returns rigid fp32 [N,2,H,W].
    With flow [N,2,H,W] (and optionally valid uint8 [N,H,W], the mask of flow_consistency): (rigid, label), label uint8 [N,H,W] =
    0 not judged (the pixel projects outside the image or behind the camera, valid is 0, or a value is not finite), 1 static

        |flow - rigid|^2 <= alpha * (|flow|^2 + |rigid|^2) + beta

    2 moving (or wrong depth).  excess=True: (rigid, label, excess), the fp32 field `left side - right side` (+inf where label is
    0).  valid is read with a flow only.  Views whose rows are dense (InputPadder.unpad's, a batch slice) are read in place through
    their strides; any other layout is copied once."""
    who = "rigid_flow"
    N, H, W = _rigid_args(who, depth, T, K, inv_K, flow, valid)
    alpha, beta, eps = not_negative(who, alpha=alpha, beta=beta, eps=eps)
    if excess and flow is None:
        raise DvsError("%s: excess=True needs a flow" % who)
    (d, d_image, d_row), K, inv_K, T, (f, f_image, f_plane, f_row), valid, p = _geometry(N, depth, K, inv_K, flow, valid, T, True)
    rigid = torch.empty((N, 2, H, W), device=d.device, dtype=torch.float32)
    label = torch.empty((N, H, W), device=d.device, dtype=torch.uint8) if f is not None else None
    over = torch.empty((N, H, W), device=d.device, dtype=torch.float32) if excess else None
    check(_lib.lib().dvs_rigid_flow(d.data_ptr(), d_image, d_row, K.data_ptr(), inv_K.data_ptr(), T.data_ptr(), p(f), f_image, f_plane,
                                    f_row, p(valid), rigid.data_ptr(), p(over), p(label), N, H, W, alpha, beta, eps, _lib.stream()),
          "dvs_rigid_flow")
    if f is None:
        return rigid
    return (rigid, label, over) if excess else (rigid, label)


POSE_SUMS = 30              # dvs_pose_fit's sums per image: 21 of J^T J, 6 of J^T e, the cost, the weights, the judged count


def pose_fit_workspace(N, H, W, device):
    """The workspace of one fit_pose call at this shape: a uint8 tensor of dvs_pose_fit_workspace bytes."""
    return torch.empty((int(_lib.lib().dvs_pose_fit_workspace(N, H, W)),), device=device, dtype=torch.uint8)


def fit_pose(depth, flow, K, inv_K=None, T0=None, valid=None, iters=4, huber=1.0, damping=1e-6, eps=1e-7, normal=False,
             workspace=None):
    """The camera motion under which a STATIC scene of this depth shows this flow, on the device (dvs_pose_fit; include/dvslam.h
    states the arithmetic): `iters` Gauss-Newton steps on SE(3) over the reprojection error of every judged pixel, with Huber
    weights (huber=inf: plain least squares), two launches a step.  The inverse of rigid_flow, whose conventions it shares.

    depth [N,1,H,W] or [N,H,W] fp32, of the flow's SOURCE frame; flow [N,2,H,W] fp32; K and inv_K [4,4] or [N,4,4] (inv_K=None
    inverts K once with torch.linalg.inv on the device); T0 [N,4,4], the initial guess (None: the identity); valid uint8 [N,H,W]
    or None: the pixels that take part (flow_consistency's mask, or rigid_flow's label == 1).  Returns (T, status): T fp32 [N,4,4]
    maps points of the source camera into the target camera, status int32 [N] is 0 where every step was taken and 1 where one
    was skipped (fewer than 6 judged pixels, a singular or non-finite system: T then stays where it was).  normal=True:
    (T, status, normal), normal fp64 [N,30] = the sums at the final T (0 .. 20 the upper triangle of J^T W J, 21 .. 26 J^T W e, 27
    the cost, 28 the sum of the weights, 29 the judged count).  workspace: a tensor of pose_fit_workspace(N, H, W, device) to
    reuse; by default one is allocated.  Views whose rows are dense are read in place through their strides; any other layout
    is copied once."""
    who = "fit_pose"
    if flow is None:
        raise DvsError("%s: flow: a measured flow [N,2,H,W] is what the pose is fitted to" % who)
    N, H, W = _rigid_args(who, depth, T0, K, inv_K, flow, valid, T_name="T0" if T0 is not None else None)
    iters = int(iters)
    if not 0 <= iters <= 64:
        raise DvsError("%s: iters=%r must be in 0 .. 64" % (who, iters))
    huber = float(huber)
    if not huber > 0.0:
        raise DvsError("%s: huber=%r must be above 0 (inf: plain least squares)" % (who, huber))
    damping, eps = not_negative(who, damping=damping, eps=eps)
    (d, d_image, d_row), K, inv_K, T0, (f, f_image, f_plane, f_row), valid, p = _geometry(N, depth, K, inv_K, flow, valid, T0, False)
    lib = _lib.lib()
    need = int(lib.dvs_pose_fit_workspace(N, H, W))
    if workspace is None:
        workspace = torch.empty((need,), device=d.device, dtype=torch.uint8)
    elif workspace.device != d.device or workspace.numel() * workspace.element_size() < need or not workspace.is_contiguous():
        raise DvsError("%s: workspace must be a dense tensor of at least %d bytes on %s" % (who, need, d.device))
    T = torch.empty((N, 4, 4), device=d.device, dtype=torch.float32)
    status = torch.empty((N,), device=d.device, dtype=torch.int32)
    sums = torch.empty((N, POSE_SUMS), device=d.device, dtype=torch.float64) if normal else None
    check(lib.dvs_pose_fit(d.data_ptr(), d_image, d_row, K.data_ptr(), inv_K.data_ptr(), T0.data_ptr(), f.data_ptr(), f_image, f_plane,
                           f_row, p(valid), T.data_ptr(), status.data_ptr(), p(sums), workspace.data_ptr(),
                           workspace.numel() * workspace.element_size(), N, H, W, iters, huber, damping, eps, _lib.stream()),
          "dvs_pose_fit")
    return (T, status, sums) if normal else (T, status)


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


def _low_up(model, call, a, b, iters, flow_init):
    """(flow_low, flow_up at the padded size) of call(a, b), call being `model`, model.refine or model.refine_pair: RAFT has a test
    mode; SmallRAFT's counterpart is last_only and its flow_low."""
    if isinstance(model, RAFT):
        return call(a, b, iters=iters, flow_init=flow_init, test_mode=True)
    up = call(a, b, iters=iters, flow_init=flow_init, last_only=True)[-1]
    return model.flow_low[-1], up


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
        # a padded size the model refuses: the model's own error
        flow_low, flow_pad = _low_up(self.model, self.model, a, b, self.iters, self.flow_init)
        self._shape = shape
        if self.warm_start:
            self.flow_init = forward_interpolate(flow_low)
        flow_up = padder.unpad(flow_pad)
        image = flow_to_image(flow_up, convert_to_bgr=self.convert_to_bgr) if self.image else None
        return SimpleNamespace(flow_low=flow_low, flow_up=flow_up, image=image)

    __call__ = pred


# ---- one frame at a time ---------------------------------------------------------------------------------------------------------
def _frames_u8(who, frame):
    """A uint8 [H,W,3] or [N,H,W,3] tensor (host or device) as its [N,H,W,3] view."""
    if not torch.is_tensor(frame):
        raise DvsError("%s: a uint8 tensor [H,W,3] or [N,H,W,3] expected, got %s" % (who, type(frame).__name__))
    if frame.dtype != torch.uint8:
        raise DvsError("%s: uint8 only, got %s (the frame as the decoder delivers it; float pairs are FlowPredictor's)" % (who, frame.dtype))
    if frame.dim() not in (3, 4) or frame.shape[-1] != 3 or min(frame.shape) < 1:
        raise DvsError("%s: [H,W,3] or [N,H,W,3] expected, got %s" % (who, tuple(frame.shape)))
    return frame if frame.dim() == 4 else frame[None]


def frame_ingest(frame, pad=(0, 0, 0, 0), bgr=False):
    """dvs_frame_ingest (include/dvslam.h states the arithmetic): uint8 frames [H,W,3] or [N,H,W,3] on the GPU, RGB (BGR with
    bgr=True), to the RAFT encoders' first operand: 2 * (x / 255) - 1, replicate-padded by pad = (left, right, top, bottom) as
    InputPadder._pad orders them (0 .. 7 each), with a zero fourth channel, fp32 [N,4,Hp,Wp] in NHWC memory.  Bit for bit what
    the reference's .float() / 255.0, InputPadder.pad and 2 * image - 1.0 give on the CPU.  Frames whose pixels are three
    adjacent bytes are read in place through their strides; any other layout is copied once."""
    who = "frame_ingest"
    f = _frames_u8(who, frame)
    if not f.is_cuda:
        raise DvsError("%s: GPU tensors only (got %s); this package has no CPU path" % (who, f.device))
    pad = tuple(int(p) for p in pad)
    if len(pad) != 4 or min(pad) < 0 or max(pad) > 7:
        raise DvsError("%s: pad=%r must be (left, right, top, bottom), each in 0 .. 7" % (who, pad))
    f, image_stride, row_stride = _packed(f)
    N, H, W, _ = f.shape
    left, right, top, bottom = pad
    out = torch.empty((N, top + H + bottom, left + W + right, 4), device=f.device, dtype=torch.float32)
    check(_lib.lib().dvs_frame_ingest(f.data_ptr(), image_stride, row_stride, out.data_ptr(), N, H, W, left, right, top, bottom,
                                      int(bool(bgr)), _lib.stream()), "dvs_frame_ingest")
    return out.permute(0, 3, 1, 2)


class FlowFrame:
    """What FlowStream.push returns for a pair: flow_low [N,2,Hp/8,Wp/8] at the padded size, flow_up [N,2,H,W] (a view of the padded
    flow), image uint8 [N,H,W,3] or None, all on the device.  With host=True, image_host and flow_low_host are numpy views of
    pinned host memory that is filled asynchronously: reading one waits for this frame's copy event first (`wait()`), and the
    views stay valid until the push after next (two buffers).
    A bidirectional stream also fills flow_low_bw and flow_up_bw (the pair current -> previous, shaped like flow_low and flow_up),
    valid uint8 [N,H,W] on the previous frame's grid and valid_bw on the current frame's (flow_consistency of flow_up and
    flow_up_bw), and with host=True valid_host; they are None otherwise.  flow_low, flow_up and image are the forward pair's.
    A rigid stream (RigidFlowStream) also fills rigid fp32 [N,2,H,W] and motion uint8 [N,H,W] (rigid_flow's rigid and label for
    flow_up), and with host=True motion_host; they are None otherwise.
    A pose stream (PoseFlowStream) also fills T fp32 [N,4,4], the camera motion fitted to flow_up (previous -> current camera), and
    pose_status int32 [N] (fit_pose's status of the last round), and with host=True T_host; rigid and motion are then taken under
    that T.  They are None otherwise."""

    def __init__(self, flow_low, flow_up, image, slot=None, flow_low_bw=None, flow_up_bw=None, valid=None, valid_bw=None,
                 rigid=None, motion=None, T=None, pose_status=None):
        self.flow_low, self.flow_up, self.image, self._slot = flow_low, flow_up, image, slot
        self.flow_low_bw, self.flow_up_bw, self.valid, self.valid_bw = flow_low_bw, flow_up_bw, valid, valid_bw
        self.rigid, self.motion = rigid, motion
        self.T, self.pose_status = T, pose_status

    def wait(self):
        if self._slot is None:
            raise DvsError("FlowStream: host copies are made with host=True only")
        self._slot.wait()
        return self

    def _host(self, name):
        t = self.wait()._slot[name]
        return t.numpy() if t is not None else None

    flow_low_host = property(lambda self: self._host("flow_low"))
    image_host = property(lambda self: self._host("image"))
    valid_host = property(lambda self: self._host("valid"))
    motion_host = property(lambda self: self._host("motion"))
    T_host = property(lambda self: self._host("T") if "T" in self.wait()._slot else None)


class FlowStream:
    """RAFT on a stream of uint8 frames, one push per frame: every frame is ingested by ONE launch (dvs_frame_ingest: /255, the
    replicate padding, 2 * x - 1, conv1's 4-channel NHWC operand) and encoded ONCE (fnet and cnet over N images), its features
    are kept for the next push, and each pair is model.refine(previous, current) with forward_interpolate(flow_low) kept as the
    next flow_init, exactly as in FlowPredictor.

        stream = FlowStream(raft.RAFT({"small": False}).cuda().eval(), iters=12)
        for frame in frames:                    # uint8 [H,W,3] or [N,H,W,3], RGB (bgr=True: BGR); on the GPU, or on the host
            r = stream.push(frame)              # None for the first frame of a sequence, then a FlowFrame for (previous, this)
        stream.reset()                          # a new sequence

    A host frame is copied with one non_blocking H2D copy (pin it to make that asynchronous).  The copy then reads the caller's
    buffer after push has returned: do not write the next frame into it before `stream.frame_copied.synchronize()` (an event
    recorded behind the copy; None after a push of a device frame), or hand push a buffer of its own per frame in flight.  A device frame whose pixels are
    three adjacent bytes (dense, a batch slice, a crop of a larger frame) is read in place; any other layout is copied once.
    Frames are taken as they are: a caller who wants the demo's Image.resize((640, 480), BILINEAR) runs input_pipeline's PIL-exact
    uint8 resize first and pushes its output.

    graph=True (the default: measured faster than the eager stream for both models; graph=False issues the
    same launches eagerly and returns fresh tensors): everything after the copy of the frame into a static uint8 buffer, the kept
    flow and the hand-over of this frame's features included, is one HIP graph, captured on one stream at the first push of a shape
    and again when stale().  The returned tensors are then the graph's static outputs: consume (or clone) them before the
    next push.  A zeroed flow_init is the cold start, so reset() zeroes the buffer and marks the slot empty without a new capture.
    host=True: the picture and flow_low are also copied asynchronously into two alternating pinned host buffers (FlowFrame).
    bidirectional=True: each pair is model.refine_pair(previous, current), ONE loop at batch 2N (rows 0 .. N-1 previous -> current,
    rows N .. 2N-1 current -> previous; no further encoder pass), the kept flow is forward_interpolate of all 2N flow_low, and
    flow_consistency(flow_up, flow_up_bw, fb_alpha, fb_beta) on the un-padded views adds the two validity masks, inside the same
    graph.  The default changes nothing.  Measured: DESIGN.md section 23.  The rigid mode is RigidFlowStream, below."""

    def __init__(self, model, iters=12, warm_start=True, pad_mode="sintel", image=True, convert_to_bgr=False, bgr=False,
                 graph=True, host=False, warmup=2, bidirectional=False, fb_alpha=0.01, fb_beta=0.5):
        if not isinstance(model, (RAFT, SmallRAFT)):
            raise DvsError("FlowStream: model must be a raft.RAFT or a raft.SmallRAFT, got %s" % type(model).__name__)
        if int(iters) < 1:
            raise DvsError("FlowStream: iters=%r must be at least 1" % (iters,))
        self.model, self.iters, self.warm_start, self.pad_mode = model, int(iters), bool(warm_start), pad_mode
        self.image, self.convert_to_bgr, self.bgr = bool(image), bool(convert_to_bgr), bool(bgr)
        self.use_graph, self.host, self.warmup = bool(graph), bool(host), int(warmup)
        self.bidirectional = bool(bidirectional)
        self.fb_alpha, self.fb_beta = not_negative("FlowStream", fb_alpha=fb_alpha, fb_beta=fb_beta)
        self.flow_init = None               # eager: the kept flow or None; graph: the persistent buffer
        self._prev, self._shape = None, None  # the previous frame's features (graph: the slot, with _have_prev)
        self._have_prev = False
        self._captured, self._graph_shape = None, None
        self._ring = HostRing()
        self.frame_copied = None            # the event behind the last host frame's H2D copy
        self.rigid, self.rigid_alpha, self.rigid_beta = False, 0.01, 0.5      # RigidFlowStream's mode
        self._geo = None                    # graph mode: the static depth, T, K and inv_K the rigid-flow node reads

    graph = property(lambda self: self._captured and self._captured.graph)

    def reset(self):
        """A new sequence: the next push encodes its frame and returns None."""
        self._shape, self._have_prev = None, False
        if self.graph is None:
            self.flow_init, self._prev = None, None
        elif self.warm_start:
            self.flow_init.zero_()

    # ---- one step, eager or under capture --------------------------------------------------------------------------------------
    def _encode(self, frames, padder):
        return self.model.encode_frame(frame_ingest(frames, padder._pad, self.bgr))

    def _pair(self, prev, feat, flow_init, padder, geo=None):
        """(the pair's FlowFrame, without a slot; the next flow_init).  geo: a rigid stream's (depth, T, K, inv_K)."""
        refine = self.model.refine_pair if self.bidirectional else self.model.refine     # refine_pair: batch 2N, forward rows first
        flow_low, flow_pad = _low_up(self.model, refine, prev, feat, self.iters, flow_init)
        kept = forward_interpolate(flow_low) if self.warm_start else None
        flow_up = padder.unpad(flow_pad)
        frame = FlowFrame(flow_low, flow_up, None)
        if self.bidirectional:                              # the mask is taken on the un-padded views: the padding is not the image
            N = flow_up.shape[0] // 2
            frame.flow_low, frame.flow_up = flow_low[:N], flow_up[:N]
            frame.flow_low_bw, frame.flow_up_bw = flow_low[N:], flow_up[N:]
            frame.valid, frame.valid_bw = flow_consistency(frame.flow_up, frame.flow_up_bw, self.fb_alpha, self.fb_beta)
        if self.image:
            frame.image = flow_to_image(frame.flow_up, convert_to_bgr=self.convert_to_bgr)
        if self.rigid:                                      # on the same un-padded view, masked by the forward validity
            self._label(frame, geo)
        return frame, kept

    def _label(self, frame, geo):
        """A rigid stream's fields of the pair, from its (depth, T, K, inv_K)."""
        frame.rigid, frame.motion = rigid_flow(*geo, flow=frame.flow_up, valid=frame.valid, alpha=self.rigid_alpha, beta=self.rigid_beta)

    def _host_fields(self, frame):
        """What host=True copies besides flow_low, image, valid and motion: name -> tensor."""
        return {}

    def _graph_step(self):
        """What the graph holds: s_frame -> a FlowFrame, flow_init and the previous slot advanced in place."""
        feat = self._encode(self.s_frame, self._padder)
        frame, kept = self._pair(self._prev, feat, self.flow_init, self._padder, self._geo)
        if kept is not None:
            self.flow_init.copy_(kept)
        for name in ("fmap", "net", "inp"):                 # copy_ bumps inp's version: the update block's hoisted terms are re-made
            getattr(self._prev, name).copy_(getattr(feat, name))
        return frame

    # ---- capture -----------------------------------------------------------------------------------------------------------------
    def _derived(self):
        return [m._weights for m in (self.model.fnet, self.model.cnet, self.model.update_block)]

    def _state(self):
        return [self._prev.fmap, self._prev.net, self._prev.inp] + ([self.flow_init] if self.warm_start else [])

    def _allocate(self, frames, padder):
        """The first push of a shape: the static frame, the previous slot, the kept flow, a rigid stream's operands, a new graph."""
        self._captured = self._graph_shape = None
        self._padder = padder
        self.s_frame = torch.empty(tuple(frames.shape), device=frames.device, dtype=torch.uint8)
        self.s_frame.copy_(frames)
        feat = self._encode(self.s_frame, padder)           # a padded size the model refuses: the model's own error
        self._prev = SimpleNamespace(fmap=feat.fmap.clone(), net=feat.net.clone(), inp=feat.inp.clone())
        N, _, h, w = feat.fmap.shape
        pairs = 2 * N if self.bidirectional else N          # bidirectional: the kept flow of both directions, forward rows first
        self.flow_init = torch.zeros((pairs, 2, h, w), device=frames.device) if self.warm_start else None
        if self.rigid:                                      # filled before every replay, as s_frame is
            f32 = dict(device=frames.device, dtype=torch.float32)
            self._geo = (torch.ones((N,) + tuple(frames.shape[1:3]), **f32),) + tuple(
                torch.eye(4, **f32).repeat(N, 1, 1) for _ in range(3))
        self._captured = CapturedStep(self._graph_step, (self.model,), state=self._state, derived=self._derived)
        self._captured.capture(self.warmup)
        self._graph_shape = self._shape_of(frames)

    def stale(self):
        """True when the weights or BatchNorm buffers changed since the capture, or the operands derived from them were re-made."""
        return self._captured is not None and self._captured.stale()

    @staticmethod
    def _shape_of(frames):
        return (tuple(frames.shape), frames.device)

    # ---- push --------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def push(self, frame, depth=None, T=None, K=None, inv_K=None):
        if self.model.training:
            raise DvsError("FlowStream: the model is in train() mode; call model.eval() (inference runs BatchNorm on its running "
                           "statistics and keeps no graph)")
        frames = _frames_u8("FlowStream: frame", frame)
        device = next(self.model.parameters()).device
        if device.type != "cuda":
            raise DvsError("FlowStream: the model is on %s; GPU only, this package has no CPU path" % (device,))
        self.frame_copied = None
        if not frames.is_cuda:
            frames = frames.to(device, non_blocking=True)   # one H2D copy (asynchronous from pinned memory)
            self.frame_copied = torch.cuda.Event()
            self.frame_copied.record()
        shape = self._shape_of(frames)
        if self._shape is not None and shape != self._shape:
            raise DvsError("FlowStream: input changed from %s on %s to %s on %s inside a sequence; call reset() first"
                           % (self._shape + shape))
        geo = self._geo_args(frames, depth, T, K, inv_K)
        padder = InputPadder(frames.shape[1:3], self.pad_mode)
        if self.use_graph:
            out = self._push_graph(frames, padder, geo)
        else:
            out = self._push_eager(frames, padder, geo)
        self._shape = shape
        if out is None:
            return None
        if self.use_graph:                                  # `out` is the graph's own frame: every push hands out a fresh one
            out = copy.copy(out)
        if self.host:
            out._slot = self._ring.put(flow_low=out.flow_low, image=out.image, valid=out.valid, motion=out.motion,
                                       **self._host_fields(out))
        return out

    def _geo_args(self, frames, depth, T, K, inv_K):
        """A rigid stream's (depth, T, K, inv_K) for the pair this push completes, checked; None for the first frame of a
        sequence (no pair: the arguments are not read) and for a stream that is not rigid."""
        if not self.rigid:
            if not (depth is None and T is None and K is None and inv_K is None):
                raise DvsError("FlowStream: depth, T, K and inv_K are arguments of a rigid stream (RigidFlowStream)")
            return None
        if self._shape is None:
            return None
        for name, t in (("depth", depth), ("T", T), ("K", K)):
            if t is None:
                raise DvsError("FlowStream: a rigid stream needs %s with every frame after the first (depth: of the PREVIOUS frame, "
                               "T: previous -> current camera, K: the 4x4 intrinsics)" % name)
        N, H, W = frames.shape[:3]
        _rigid_args("FlowStream", depth, T, K, inv_K, shape=(N, H, W))
        if depth.device != frames.device:
            raise DvsError("FlowStream: depth is on %s, the frame on %s" % (depth.device, frames.device))
        depth = depth.detach() if depth.dim() == 3 else depth.detach()[:, 0]
        return depth, T, K, inv_K if inv_K is not None else torch.linalg.inv(K)

    def _push_eager(self, frames, padder, geo=None):
        feat = self._encode(frames, padder)                 # a padded size the model refuses: the model's own error
        prev, self._prev = self._prev, feat
        if prev is None:
            return None
        out, self.flow_init = self._pair(prev, feat, self.flow_init, padder, geo)
        return out

    def _push_graph(self, frames, padder, geo=None):
        if self._graph_shape != self._shape_of(frames):
            self._have_prev = False
            self._allocate(frames, padder)
        elif self._captured.stale():
            self._captured.capture(self.warmup)
        self.s_frame.copy_(frames, non_blocking=True)
        if geo is not None:
            for static, t in zip(self._geo, geo):           # a [4,4] K or inv_K is broadcast over the images
                static.copy_(t, non_blocking=True)
        self._captured.replay()
        if self._have_prev:
            return self._captured.out
        self._have_prev = True                              # the first frame of a sequence: only its features count
        if self.warm_start:
            self.flow_init.zero_()
        return None


class RigidFlowStream(FlowStream):
    """FlowStream in its rigid mode: every pair also gets the flow a static scene would show under the previous frame's depth and
    the camera motion, and a label per pixel that says where the measured flow disagrees with it (rigid_flow, dvs_rigid_flow).

        stream = RigidFlowStream(model, iters=12, bidirectional=True)       # every FlowStream argument, plus rigid_alpha, rigid_beta
        for frame in frames:
            r = stream.push(frame, depth=depth_prev, T=T, K=K, inv_K=inv_K) # depth of the PREVIOUS frame, T: previous -> current
            # r.rigid [N,2,H,W], r.motion uint8 [N,H,W]: 0 not judged, 1 static, 2 moving; host=True: r.motion_host

    depth [N,1,H,W] or [N,H,W] at the un-padded frame size, T [N,4,4], K and inv_K [4,4] or [N,4,4], fp32 on the frame's device;
    inv_K=None inverts K with torch.linalg.inv on every push.  The first frame of a sequence completes no pair and reads none of
    them; after it a missing or mis-shaped one is a DvsError that names it.  The kernel runs on the un-padded flow_up view, with
    `valid` as its mask in a bidirectional stream (an occluded pixel is not judged).  graph=True: the four tensors are copied into
    static buffers before the replay, as the frame is, and the kernel is a node of the same single-stream graph; reset(), stale()
    and the re-capture rules are FlowStream's.  rigid=False is a plain FlowStream.  Measured: DESIGN.md section 24."""

    def __init__(self, model, *args, rigid=True, rigid_alpha=0.01, rigid_beta=0.5, **kw):
        super().__init__(model, *args, **kw)
        self.rigid = bool(rigid)
        self.rigid_alpha, self.rigid_beta = not_negative("FlowStream", rigid_alpha=rigid_alpha, rigid_beta=rigid_beta)


class PoseFlowStream(RigidFlowStream):
    """RigidFlowStream that FITS the camera motion to the measured flow instead of being handed it: every pair needs only the
    previous frame's depth and the intrinsics, and its static / moving label is taken under the pose that the static pixels
    themselves agree on (fit_pose, dvs_pose_fit).

        stream = PoseFlowStream(model, iters=12, bidirectional=True)        # every RigidFlowStream argument, plus pose_iters,
        for frame in frames:                                                # pose_huber, pose_rounds
            r = stream.push(frame, depth=depth_prev, K=K, inv_K=inv_K)      # T=: an optional initial guess (PoseNet's); else identity
            # r.T [N,4,4] previous -> current camera, r.pose_status int32 [N], r.rigid and r.motion under r.T; host=True: r.T_host

    Round 1 fits over `valid` (every pixel in a one-directional stream), pose_iters Gauss-Newton steps with Huber weights of
    pose_huber pixels.  Every further round labels the flow with rigid_flow under the current pose and refits over the pixels
    labelled static (label == 1), starting from that pose: a moving object pulls a Huber fit, and leaves the second round
    altogether.  The frame's rigid and motion are rigid_flow under the final pose, with `valid` as the mask.
    graph=True: all of it is nodes of the same single-stream graph; the workspace and the static guess are allocated with the
    other static buffers, and the guess is refilled before every replay (with the identity when none is passed)."""

    def __init__(self, model, *args, pose_iters=4, pose_huber=1.0, pose_rounds=2, **kw):
        super().__init__(model, *args, **kw)
        self.pose_iters, self.pose_rounds, self.pose_huber = int(pose_iters), int(pose_rounds), float(pose_huber)
        if not 1 <= self.pose_iters <= 64 or self.pose_rounds < 1 or not self.pose_huber > 0.0:
            raise DvsError("FlowStream: pose_iters=%r must be in 1 .. 64, pose_rounds=%r at least 1, pose_huber=%r above 0"
                           % (pose_iters, pose_rounds, pose_huber))
        self._pose_ws, self._eye = None, None

    def push(self, frame, depth=None, K=None, inv_K=None, T=None):
        if T is None and self.rigid and torch.is_tensor(frame) and frame.dim() in (3, 4):
            N = frame.shape[0] if frame.dim() == 4 else 1
            device = next(self.model.parameters()).device
            if self._eye is None or self._eye.shape[0] != N or self._eye.device != device:
                self._eye = torch.eye(4, device=device, dtype=torch.float32).repeat(N, 1, 1)
            T = self._eye
        return super().push(frame, depth=depth, T=T, K=K, inv_K=inv_K)

    def _allocate(self, frames, padder):
        N, H, W = frames.shape[:3]
        self._pose_ws = pose_fit_workspace(N, H, W, frames.device) if self.rigid else None
        super()._allocate(frames, padder)

    def _label(self, frame, geo):
        depth, T, K, inv_K = geo
        ws = self._pose_ws if self.use_graph else None      # eager: fresh tensors, a workspace included
        mask = frame.valid
        for round_ in range(self.pose_rounds):
            if round_:                                      # the pixels that are static under the pose so far
                _, label = rigid_flow(depth, T, K, inv_K, flow=frame.flow_up, valid=frame.valid, alpha=self.rigid_alpha,
                                      beta=self.rigid_beta)
                mask = (label == 1).view(torch.uint8)
            T, frame.pose_status = fit_pose(depth, frame.flow_up, K, inv_K, T0=T, valid=mask, iters=self.pose_iters,
                                            huber=self.pose_huber, workspace=ws)
        frame.T = T
        super()._label(frame, (depth, T, K, inv_K))

    def _host_fields(self, frame):
        return {"T": frame.T} if self.rigid else {}
