"""Inference path of the networks (callers vo/predict.py:20-42,63-86, vo/eval_traj.py,
vo/eval_redwood.py:325-350 and the ROS2 node): `.eval()` + `torch.no_grad()`, batch 1, `("disp", 0)` and the 6-DoF pose.

Nothing has to change in those callers: in that mode `nn_ops.conv_bn_act` folds every BatchNorm into the convolution in
front of it and lets the conv epilogue add the identity and apply the ReLU (one kernel per conv, `dvs_conv_fusion.residual`).
This module adds the two optional extras a real-time loop wants:

  * `depth_net.inference_scales = (0,)`   skip the three coarse disparity heads nobody reads at inference;
  * `Graphed(net, example)`               capture `net(example)` into a HIP graph and replay it per frame;
  * `FramePredictor(depth, pose, ...)`    the whole per-frame work, PoseNet and DepthNet side by side on two streams (at batch 1
                                          neither fills the chip), by default as one graph with a fork / join;
  * `CloudPredictor(depth, pose, ...)`    FramePredictor + world pose chain and coloured point cloud on the device (pointcloud.py)
                                          inside the same graph, then one asynchronous copy into pinned host memory.
"""
import torch

from . import _lib
from ._graph import CapturedStep, HostRing


class Graphed:
    """net(x) for one fixed input shape, replayed from a captured HIP graph.

    The returned tensors are the graph's static outputs: consume (or clone) them before the next call.  The BatchNorm fold is part
    of the capture, which is made again by itself when the weights or buffers change (_graph.CapturedStep)."""

    def __init__(self, net, example, warmup=3):
        if net.training:
            raise _lib.DvsError("Graphed: put the network in eval() mode first (training steps are issued eagerly)")
        if not example.is_cuda:
            raise _lib.DvsError("Graphed: GPU tensors only; this package has no CPU path")
        self.net = net
        self.static_in = example.detach().clone()
        self.warmup = warmup
        self._captured = CapturedStep(self._step, (net,))
        self.refresh()

    def _step(self):
        return self.net(self.static_in)

    graph = property(lambda self: self._captured.graph)
    static_out = property(lambda self: self._captured.out)

    def refresh(self):
        self._captured.capture(self.warmup)

    def stale(self):
        """True when the weights or BatchNorm buffers changed since the capture (the fold is part of the graph)."""
        return self._captured.stale()

    def __call__(self, x):
        if x.shape != self.static_in.shape:
            raise _lib.DvsError("Graphed: captured for input %s, got %s" % (tuple(self.static_in.shape), tuple(x.shape)))
        if self.stale():
            self.refresh()                   # re-fold and re-capture: never replay pointers to a replaced fold
        self.static_in.copy_(x, non_blocking=True)
        self._captured.replay()
        return self.static_out


class FramePredictor:
    """The per-frame work of vo/predict.py:63-86 -- PoseNet on the frame pair + 4x4 pose matrix, DepthNet on the target
    frame + depth -- with the two networks on two HIP streams (they are independent, and at batch 1 neither fills the
    chip), optionally captured as ONE HIP graph with a fork / join.  Returns (T [B,4,4], depth [B,1,H,W], disp); with
    graph=True these are the graph's static outputs (consume or clone them before the next call)."""

    def __init__(self, depth_net, pose_net, target, pair, min_depth=0.1, max_depth=10.0, invert=False, graph=True,
                 warmup=3):
        if depth_net.training or pose_net.training:
            raise _lib.DvsError("FramePredictor: put both networks in eval() mode first")
        from .layers import disp_to_depth, transformation_from_parameters
        self._d2d, self._t = disp_to_depth, transformation_from_parameters
        self.depth_net, self.pose_net = depth_net, pose_net
        self.min_depth, self.max_depth, self.invert = min_depth, max_depth, invert
        self.side = torch.cuda.Stream(device=target.device)
        self._captured = None
        if graph:
            self.s_target, self.s_pair = target.detach().clone(), pair.detach().clone()
            self._captured = CapturedStep(self._step, (depth_net, pose_net), state=self._state)
            self._captured.capture(warmup)

    def _step(self):
        return self._run(self.s_target, self.s_pair)

    graph = property(lambda self: self._captured and self._captured.graph)
    static_out = property(lambda self: self._captured.out)

    def _state(self):                                           # the persistent tensors _run advances in place
        return []

    def stale(self):
        return self._captured is not None and self._captured.stale()

    def _run(self, target, pair):
        main = torch.cuda.current_stream()
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            aa, t = self.pose_net(pair)
            T = self._t(aa[:, 0], t[:, 0], invert=self.invert)
        disp = self.depth_net(target)[("disp", 0)]
        _, depth = self._d2d(disp, self.min_depth, self.max_depth)
        main.wait_stream(self.side)
        return T, depth, disp

    def __call__(self, target, pair):
        if self._captured is None:
            with torch.no_grad():
                return self._run(target, pair)
        if self._captured.stale():
            self._captured.capture(1)                           # one eager step refolds (fills the cache), then the re-capture
        self.s_target.copy_(target, non_blocking=True)
        self.s_pair.copy_(pair, non_blocking=True)
        self._captured.replay()
        return self._captured.out


class Frame:
    """One frame of CloudPredictor.  T / depth / disp are device tensors as FramePredictor returns them.  records, count,
    world_pose and tq live in pinned host memory that is filled asynchronously: reading one of them waits for this frame's
    copy event first (`wait()`), so a caller can do host work between the call and the first read.  The host views stay
    valid until the call after next (two buffers)."""

    def __init__(self, T, depth, disp, slot, batch):
        self.T, self.depth, self.disp = T, depth, disp
        self._slot, self._batch = slot, batch

    def wait(self):
        self._slot.wait()
        return self

    def _host(name, doc):
        return property(lambda self: self._slot.wait()[name].numpy(), doc=doc)

    count = _host("count", "Records per image, numpy int32 [B].")
    world_pose = _host("world", "World pose after this frame, numpy [4,4] (after the last image of the batch).")
    tq = _host("tq", "(tx, ty, tz, qx, qy, qz, qw) of the world pose after each image, numpy [B,7].")

    @property
    def records(self):
        """pointcloud.as_records view: a RECORD_DTYPE array for batch 1, a list of them otherwise."""
        from . import pointcloud
        r = pointcloud.as_records(self._slot.wait()["records"], self.count)
        return r[0] if self._batch == 1 else r


class CloudPredictor(FramePredictor):
    """FramePredictor + world pose + coloured point cloud, ready to publish: what visualizer_node.py:128-191 and
    vo/predict.py:69-98 do on the host after the two networks.  Same fork / join: the pose chain (pointcloud.PoseChain,
    world <- world @ T) follows the pose matrix on the pose stream, the cloud kernel follows the join and reads ("disp", 0)
    directly; with graph=True all of it is one captured graph.  The records (+ count, tq, world pose) are then copied
    asynchronously into pinned, double-buffered host memory, one event per buffer.

    K: [B,4,4] or [B,3,3] intrinsics (device tensor, copied).  frame: "world" (points through left @ world) or "camera"
    (the ROS2 node's cloud; the pose chain still runs and `left` only shapes nothing then).  stride / z_range as
    pointcloud.depth_to_cloud (z_range switches compact mode on).  d2h (compact mode only): "full" copies the whole
    capacity and slices on the host after the event; "count" copies `count` first, waits for it inside the call, then copies
    count[b] records per image.  init: start pose.  A capture puts `chain.world` back: the pose advances exactly once per call."""

    def __init__(self, depth_net, pose_net, target, pair, K, *, frame="world", left=None, init=None, stride=1, z_range=None,
                 min_depth=0.1, max_depth=10.0, invert=False, graph=True, d2h="full", warmup=3):
        from . import pointcloud
        if frame not in ("world", "camera"):
            raise _lib.DvsError("CloudPredictor: frame must be 'world' or 'camera'")
        if d2h not in ("full", "count"):
            raise _lib.DvsError("CloudPredictor: d2h must be 'full' or 'count'")
        if not K.is_cuda:
            raise _lib.DvsError("CloudPredictor: GPU tensors only; this package has no CPU path")
        self._pc = pointcloud
        dev = target.device
        B, _, H, W = target.shape
        self.frame, self.stride, self.z_range, self.d2h = frame, stride, z_range, d2h
        self.K = K.detach().float().contiguous().clone()
        self.chain = pointcloud.PoseChain(dev, left=left, init=init)
        cfg = pointcloud.make_cfg(B, H, W, stride, (min_depth, max_depth), z_range, self.K.shape[1])
        n_max = pointcloud.capacity(cfg)
        f32 = dict(device=dev, dtype=torch.float32)
        self.d_poses, self.d_M, self.d_tq = torch.empty(B, 4, 4, **f32), torch.empty(B, 4, 4, **f32), torch.empty(B, 7, **f32)
        self.d_records = torch.zeros(B, n_max, 4, **f32)
        self.d_count = torch.zeros(B, device=dev, dtype=torch.int32)
        ws = pointcloud.workspace_bytes(cfg)
        self.d_ws = torch.empty(ws, device=dev, dtype=torch.uint8) if ws else None
        self._ring = HostRing()
        super().__init__(depth_net, pose_net, target, pair, min_depth=min_depth, max_depth=max_depth, invert=invert,
                         graph=graph, warmup=warmup)

    @property
    def world(self):
        """The world pose on the device ([4,4], persistent; advanced once per call)."""
        return self.chain.world

    def reset(self, init=None):
        self.chain.reset(init)

    def _state(self):
        return [self.chain.world]

    def _run(self, target, pair):
        main = torch.cuda.current_stream()
        self.side.wait_stream(main)
        with torch.cuda.stream(self.side):
            aa, t = self.pose_net(pair)
            T = self._t(aa[:, 0], t[:, 0], invert=self.invert)
            self.chain.step(T, self.d_poses, self.d_M, self.d_tq)
        disp = self.depth_net(target)[("disp", 0)]
        _, depth = self._d2d(disp, self.min_depth, self.max_depth)
        main.wait_stream(self.side)
        self._pc.depth_to_cloud(disp, target, self.K, self.d_M if self.frame == "world" else None,
                                from_disp=(self.min_depth, self.max_depth), stride=self.stride, z_range=self.z_range,
                                out=self.d_records, count=self.d_count, workspace=self.d_ws)
        return T, depth, disp

    def __call__(self, target, pair):
        out = super().__call__(target, pair)
        slot = self._ring.next(records=self.d_records, count=self.d_count, tq=self.d_tq, world=self.chain.world)
        slot["count"].copy_(self.d_count, non_blocking=True)
        if self.z_range is not None and self.d2h == "count":
            slot["event"].record()
            slot["event"].synchronize()                         # the price of this mode: the call waits for the frame
            for b, c in enumerate(slot["count"].tolist()):
                slot["records"][b, :c].copy_(self.d_records[b, :c], non_blocking=True)
        else:
            slot["records"].copy_(self.d_records, non_blocking=True)
        slot["tq"].copy_(self.d_tq, non_blocking=True)
        slot["world"].copy_(self.chain.world, non_blocking=True)
        slot["event"].record()
        return Frame(out[0], out[1], out[2], slot, target.shape[0])


def prepare(depth_net, pose_net, scales=(0,)):
    """eval() both networks and restrict DepthNet to the disparity heads an inference caller reads."""
    depth_net.eval()
    pose_net.eval()
    depth_net.inference_scales = tuple(scales) if scales is not None else None
    return depth_net, pose_net
