"""numpy restatement of the output stage (pointcloud.py / csrc/cloud.hip): dense / strided / compacted cloud, pose chain and
a robust quaternion, in a chosen precision.  The fp64 variant is pinned to the reference's own routines by
tests/golden/cloud_b2_48x64.npz (tests/test_cloud_cpu.py); the fp32 variant is the yardstick for what single precision
costs on the same inputs.  Used directly where no fixture fits (full size, strides)."""
import numpy as np


def disp_to_depth(disp, min_depth, max_depth, dtype=np.float64):
    """model/layers.py:16-26 on an array."""
    dt = np.dtype(dtype).type
    lo, hi = dt(1.0 / max_depth), dt(1.0 / min_depth)
    return dt(1.0) / (lo + (hi - lo) * np.asarray(disp, dtype))


def colours(image):
    """[3,H,W] float32 in 0..1 -> [H*W,3] uint8 as denormalize_image (vo/dataset/vo_loader.py:221-225): float32 product,
    clamp, truncation."""
    c = np.clip(np.asarray(image, np.float32) * np.float32(255.0), np.float32(0.0), np.float32(255.0)).astype(np.uint8)
    return c.reshape(3, -1).T.copy()


def pack_rgb(col):
    """[N,3] uint8 -> [N] float32 carrying r << 16 | g << 8 | b (visualizer_node.py:34-39)."""
    c = col.astype(np.uint32)
    return ((c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]).view(np.float32)


def cloud(z, image, K, M=None, dtype=np.float64, stride=(1, 1), z_range=None):
    """One image.  z [H,W] depth, image [3,H,W], K [3,3] or [4,4], M [4,4] or None -> (points [N,3] dtype, colours [N,3] uint8,
    index [N] int32 = v * W + u), in row-major pixel order.  z_range (lo, hi or None): keep lo < z (< hi) only."""
    dt = np.dtype(dtype).type
    H, W = z.shape
    sy, sx = stride
    vs, us = np.meshgrid(np.arange(0, H, sy), np.arange(0, W, sx), indexing="ij")
    us, vs = us.reshape(-1), vs.reshape(-1)
    idx = (vs * W + us).astype(np.int32)
    zs = np.asarray(z, dtype).reshape(-1)[idx]
    col = colours(image)[idx]
    if z_range is not None:
        keep = zs > dt(z_range[0])
        if z_range[1] is not None and z_range[1] > 0:
            keep &= zs < dt(z_range[1])
        us, vs, zs, idx, col = us[keep], vs[keep], zs[keep], idx[keep], col[keep]
    K = np.asarray(K, dtype)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    xs = (us.astype(dtype) - cx) / fx * zs
    ys = (vs.astype(dtype) - cy) / fy * zs
    pts = np.stack([xs, ys, zs], 1)
    if M is not None:
        M = np.asarray(M, dtype)
        pts = np.stack([M[r, 0] * xs + M[r, 1] * ys + M[r, 2] * zs + M[r, 3] for r in range(3)], 1)
    return pts.astype(dtype), col, idx


def records(points, col):
    """The node's 16-byte records (create_pointcloud2, visualizer_node.py:41-44) of points [N,3] and colours [N,3]."""
    rec = np.zeros(points.shape[0], dtype=[("x", "f4"), ("y", "f4"), ("z", "f4"), ("rgb", "f4")])
    rec["x"], rec["y"], rec["z"], rec["rgb"] = points[:, 0], points[:, 1], points[:, 2], pack_rgb(col)
    return rec


def pose_chain(T, init=None, left=None, dtype=np.float64):
    """world <- world @ T[b] (vo/eval_traj.py:138-147): (poses [B,4,4], M [B,4,4] = left @ poses) in dtype."""
    world = np.eye(4, dtype=dtype) if init is None else np.asarray(init, dtype)
    poses = []
    for t in np.asarray(T, dtype):
        world = world @ t
        poses.append(world)
    poses = np.stack(poses)
    M = poses if left is None else np.asarray(left, dtype)[None] @ poses
    return poses, M


def quaternion(R):
    """Unit quaternion (qx, qy, qz, qw), qw >= 0, of a 3x3 rotation: Shepperd's method (divide by the largest component)."""
    R = np.asarray(R, np.float64)
    t = np.trace(R)
    d = [t, R[0, 0], R[1, 1], R[2, 2]]
    k = int(np.argmax(d))
    if k == 0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif k == 1:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif k == 2:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def node_quaternion(R):
    """visualizer_node.py:182-186 (undefined where 1 + trace == 0)."""
    R = np.asarray(R, np.float64)
    qw = np.sqrt(1 + R[0, 0] + R[1, 1] + R[2, 2]) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw), qw])


def tq(world):
    """(tx, ty, tz, qx, qy, qz, qw) of a 4x4 world pose."""
    world = np.asarray(world, np.float64)
    return np.concatenate([world[:3, 3], quaternion(world[:3, :3])])
