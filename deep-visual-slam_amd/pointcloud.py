"""Output stage of the inference path on the device (csrc/cloud.hip): world pose chain and coloured point cloud.

What the reference's inference callers do on the host, in numpy, after the two networks:

  * ROS2 node visualizer_node.py:128-191   world_pose @ T, meshgrid back-projection, colours, create_pointcloud2, quaternion
  * vo/predict.py:69-98 + Visualizer.draw_pointcloud (vo/utils/visualization.py:157-193)   the same, in the world frame, y flipped
  * vo/eval_traj.py:85-121,138-147          z > 0 pixels only (boolean-mask order), T_global @ points, T_global @= T_local

`depth_to_cloud` writes 16-byte records {x, y, z, rgb}: exactly the bytes of `PointCloud2.data` that create_pointcloud2
(visualizer_node.py:26-56) builds (point_step 16, little-endian, rgb = r << 16 | g << 8 | b reinterpreted as float32).
`PoseChain` keeps the world pose on the device.  No autograd: this is an output stage.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import CloudCfg, DvsError, check, ptr

RECORD_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("rgb", "f4")])


def make_cfg(B, H, W, stride=1, from_disp=None, z_range=None, k_row_stride=4):
    """dvs_cloud_cfg.  stride: int or (stride_y, stride_x); from_disp: None (the input is depth) or (min_depth, max_depth);
    z_range: None (dense mode) or (z_lo, z_hi), z_hi None / <= 0 = no upper bound (compact mode)."""
    sy, sx = (stride, stride) if isinstance(stride, int) else stride
    cfg = CloudCfg()
    cfg.B, cfg.H, cfg.W, cfg.stride_y, cfg.stride_x = int(B), int(H), int(W), int(sy), int(sx)
    cfg.k_row_stride = int(k_row_stride)
    if from_disp is not None:
        cfg.from_disp, cfg.min_depth, cfg.max_depth = 1, float(from_disp[0]), float(from_disp[1])
    if z_range is not None:
        cfg.compact, cfg.z_lo = 1, float(z_range[0])
        cfg.z_hi = float(z_range[1]) if z_range[1] is not None else 0.0
    return cfg


def capacity(cfg):
    """Records per image a configuration can produce: ceil(H / stride_y) * ceil(W / stride_x)."""
    n = C.c_int()
    check(_lib.lib().dvs_cloud_capacity(C.byref(cfg), C.byref(n)), "dvs_cloud_capacity")
    return n.value


def workspace_bytes(cfg):
    return int(_lib.lib().dvs_cloud_workspace(C.byref(cfg)))


def _f32c(t):
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def depth_to_cloud(depth_or_disp, image, K, M=None, *, from_disp=None, stride=1, z_range=None, out=None, count=None,
                   index=None, workspace=None):
    """(records [B,n_max,4] fp32, count [B] int32) of depth_or_disp [B,1,H,W], image [B,3,H,W] in 0..1, K [B,4,4] or [B,3,3],
    M [B,4,4] or None (camera frame), on the current stream.  GPU tensors only.  With `out`, `count` (and, in compact mode,
    `workspace`: a uint8 tensor of `workspace_bytes(cfg)`) given and contiguous fp32 inputs nothing is allocated, so the call
    can sit in a captured graph.  index: optional int32 [B,n_max] receiving v * W + u of every record.
    Dense mode writes every kept pixel; compact mode (z_range) leaves records[b, count[b]:] untouched."""
    for t in (depth_or_disp, image, K):
        if not t.is_cuda:
            raise DvsError("depth_to_cloud: GPU tensors only (got %s); this package has no CPU path" % t.device)
    if depth_or_disp.dim() != 4 or depth_or_disp.shape[1] != 1:
        raise DvsError("depth_to_cloud: depth / disparity must be [B,1,H,W], got %s" % (tuple(depth_or_disp.shape),))
    B, _, H, W = depth_or_disp.shape
    if tuple(image.shape) != (B, 3, H, W):
        raise DvsError("depth_to_cloud: image must be [%d,3,%d,%d], got %s" % (B, H, W, tuple(image.shape)))
    if K.dim() != 3 or K.shape[0] != B or K.shape[1] != K.shape[2] or K.shape[1] not in (3, 4):
        raise DvsError("depth_to_cloud: K must be [B,3,3] or [B,4,4], got %s" % (tuple(K.shape),))
    if M is not None and tuple(M.shape) != (B, 4, 4):
        raise DvsError("depth_to_cloud: M must be [B,4,4], got %s" % (tuple(M.shape),))
    for name, t in (("out", out), ("count", count), ("index", index), ("workspace", workspace)):
        if t is not None and not t.is_contiguous():
            raise DvsError("depth_to_cloud: %s is written in place and must be contiguous, got %s with strides %s"
                           % (name, tuple(t.shape), tuple(t.stride())))
    cfg = make_cfg(B, H, W, stride, from_disp, z_range, K.shape[1])
    n_max = capacity(cfg)
    dev = depth_or_disp.device
    if out is None:
        out = torch.empty(B, n_max, 4, device=dev, dtype=torch.float32)
    if count is None:
        count = torch.empty(B, device=dev, dtype=torch.int32)
    if tuple(out.shape) != (B, n_max, 4) or out.dtype != torch.float32:
        raise DvsError("depth_to_cloud: out must be fp32 [%d,%d,4]" % (B, n_max))
    if tuple(count.shape) != (B,) or count.dtype != torch.int32:
        raise DvsError("depth_to_cloud: count must be int32 [%d]" % B)
    if index is not None and (tuple(index.shape) != (B, n_max) or index.dtype != torch.int32):
        raise DvsError("depth_to_cloud: index must be int32 [%d,%d]" % (B, n_max))
    ws = workspace_bytes(cfg)
    if ws and workspace is None:
        workspace = torch.empty(ws, device=dev, dtype=torch.uint8)
    if ws and workspace.numel() * workspace.element_size() < ws:
        raise DvsError("depth_to_cloud: workspace of %d bytes needed" % ws)
    check(_lib.lib().dvs_cloud_fwd(C.byref(cfg), ptr(_f32c(depth_or_disp)), ptr(_f32c(image)), ptr(_f32c(K)),
                                   ptr(_f32c(M)) if M is not None else None, ptr(out), ptr(count), ptr(index),
                                   ptr(workspace) if ws else None, _lib.stream()), "dvs_cloud_fwd")
    return out, count


class PoseChain:
    """world <- world @ T, frame by frame, on the device (visualizer_node.py:149, vo/predict.py:89-90, vo/eval_traj.py:138-147).

    left: optional fixed 4x4 folded into M = left @ world, e.g. Visualizer.slam_to_pyvista = diag(1, -1, 1, 1);
    init: start pose (identity by default; Visualizer starts at y = -2, vo/utils/visualization.py:44-46)."""

    def __init__(self, device, left=None, init=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise DvsError("PoseChain: GPU only (got %s); this package has no CPU path" % self.device)
        self.left = None if left is None else self._mat(left)
        self.world = torch.empty(4, 4, device=self.device, dtype=torch.float32)
        self.reset(init)

    def _mat(self, m):
        m = torch.as_tensor(np.asarray(m.detach().cpu() if torch.is_tensor(m) else m, dtype=np.float32))
        if tuple(m.shape) != (4, 4):
            raise DvsError("PoseChain: 4x4 matrix expected, got %s" % (tuple(m.shape),))
        return m.to(self.device).contiguous()

    def reset(self, init=None):
        self.world.copy_(self._mat(np.eye(4, dtype=np.float32) if init is None else init))

    def step(self, T, poses=None, M=None, tq=None, world=None):
        """T [B,4,4] -> (poses [B,4,4], M [B,4,4], tq [B,7] = tx, ty, tz, qx, qy, qz, qw) after each of the B steps; `world`
        is advanced B steps in place.  Pre-allocated outputs (and a contiguous fp32 T) make the call allocation-free.
        world: another [4,4] device tensor to advance instead of self.world (warm-up runs of a captured graph)."""
        if not T.is_cuda:
            raise DvsError("PoseChain.step: GPU tensors only (got %s)" % T.device)
        T = _f32c(T).reshape(-1, 4, 4)
        B = T.shape[0]
        new = lambda *s: torch.empty(*s, device=T.device, dtype=torch.float32)
        poses = new(B, 4, 4) if poses is None else poses
        M = new(B, 4, 4) if M is None else M
        tq = new(B, 7) if tq is None else tq
        world = self.world if world is None else world
        for name, t, shape in (("poses", poses, (B, 4, 4)), ("M", M, (B, 4, 4)), ("tq", tq, (B, 7)), ("world", world, (4, 4))):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise DvsError("PoseChain.step: %s is written in place and must be a contiguous fp32 GPU tensor %s, got %s %s "
                               "with strides %s" % (name, list(shape), t.dtype, tuple(t.shape), tuple(t.stride())))
        check(_lib.lib().dvs_pose_chain(ptr(T), ptr(self.left), ptr(world), ptr(poses), ptr(M), ptr(tq), B, _lib.stream()),
              "dvs_pose_chain")
        return poses, M, tq


def as_records(host, count=None):
    """Zero-copy numpy view of a host record buffer as RECORD_DTYPE; `.tobytes()` (or the buffer itself) of the result is
    PointCloud2.data as create_pointcloud2 lays it out.  host: CPU tensor or float32 array [n,4] (-> one view of the first
    `count` records) or [B,n,4] (-> a list of B views, count[b] records each).  count None: all n."""
    a = host.numpy() if torch.is_tensor(host) else np.asarray(host)
    if a.dtype != np.float32 or a.shape[-1] != 4 or not a.flags["C_CONTIGUOUS"] or a.ndim not in (2, 3):
        raise DvsError("as_records: contiguous float32 [n,4] or [B,n,4] host buffer expected")
    rec = a.view(RECORD_DTYPE)[..., 0]
    if a.ndim == 2:
        return rec if count is None else rec[:int(count)]
    if count is None:
        return [rec[b] for b in range(a.shape[0])]
    return [rec[b, :int(count[b])] for b in range(a.shape[0])]
