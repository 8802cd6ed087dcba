"""CPU-side checks of the output stage (pointcloud.py / csrc/cloud.hip): the numpy restatement tests/cloud_ref.py against the
fixture recorded from the reference's own routines (tests/golden/make_golden_cloud.py), the argument checks of the new
C-ABI entries (they fail before any launch, so no GPU is needed), and the host-side record view."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_ref as R
from conftest import GOLDEN, load_golden

FIXTURE = "cloud_b2_48x64.npz"


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


def test_ref_reproduces_draw_pointcloud_and_colours(rec):
    """fp64 restatement == Visualizer.draw_pointcloud (world frame through left @ pose, and camera frame), colours equal."""
    left = rec["in/left"]
    for b in range(2):
        M = left.astype(np.float64) @ rec["in/pose"][b].astype(np.float64)
        pts, col, idx = R.cloud(rec["in/depth"][b, 0], rec["in/image"][b], rec["in/K"][b], M)
        assert np.abs(pts - rec["ref/vis_world"][b]).max() <= 1e-12
        assert np.array_equal(col, rec["ref/colors"][b])
        assert np.array_equal(idx, np.arange(48 * 64))
        cam, _, _ = R.cloud(rec["in/depth"][b, 0], rec["in/image"][b], rec["in/K"][b], left)
        assert np.abs(cam - rec["ref/vis_cam"][b]).max() <= 1e-12


def test_ref_reproduces_the_nodes_record_bytes(rec):
    """create_pointcloud2's bytes: x, y, z = float32(reference fp64), rgb field bit for bit, 16 bytes per point."""
    for b in range(2):
        node = rec["ref/node_bytes"][b]
        assert node.size == 48 * 64 * 16
        want = node.view([("x", "f4"), ("y", "f4"), ("z", "f4"), ("rgb", "f4")])
        pts, col, _ = R.cloud(rec["in/depth"][b, 0], rec["in/image"][b], rec["in/K"][b])
        got = R.records(pts, col)
        assert np.array_equal(got["rgb"].view(np.uint32), want["rgb"].view(np.uint32))
        cam = rec["ref/vis_cam"][b] * np.array([1.0, -1.0, 1.0])
        for i, f in enumerate("xyz"):
            assert np.array_equal(want[f], cam[:, i].astype(np.float32))
            assert np.abs(got[f].astype(np.float64) - cam[:, i]).max() <= 2 ** -23 * np.abs(cam[:, i]).max()


def test_ref_reproduces_eval_traj_mask_and_order(rec):
    for b in range(2):
        pts, _, idx = R.cloud(rec["in/depth_masked"][b, 0], rec["in/image"][b], rec["in/K"][b], rec["in/pose"][b],
                              z_range=(0.0, None))
        assert np.array_equal(idx, rec["ref/eval_index%d" % b])
        assert 0 < idx.size < 48 * 64
        assert np.abs(pts - rec["ref/eval_points%d" % b]).max() <= 1e-12


def test_ref_reproduces_the_pose_chain(rec):
    poses, M = R.pose_chain(rec["chain/T"], left=rec["in/left"])
    assert np.array_equal(poses, rec["chain/T_global"])
    assert np.array_equal(M[:, 1], -poses[:, 1]) and np.array_equal(M[:, 0], poses[:, 0])
    # away from a half turn the node's formula is the same quaternion -- up to how far the products of fp32 matrices are from
    # orthogonal (<= 64 steps x 2^-23 per entry), which the node's formula passes on and the unit quaternion here does not
    for p in poses[::9]:
        assert np.abs(R.quaternion(p[:3, :3]) - R.node_quaternion(p[:3, :3])).max() < 64 * 2 ** -23
    half = np.diag([-1.0, 1.0, -1.0])                      # half turn about y: 1 + trace == 0
    assert np.allclose(np.abs(R.quaternion(half)), [0, 1, 0, 0])
    assert abs(np.linalg.norm(R.quaternion(poses[-1][:3, :3])) - 1) < 1e-12


def test_disp_to_depth_matches_the_fixture(rec):
    d = R.disp_to_depth(rec["in/disp"], 0.1, 10.0, np.float32)
    assert np.abs(d.astype(np.float64) - rec["in/depth"]).max() <= 2 * 2 ** -23 * rec["in/depth"].max()


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_committed_fixture(rec, tmp_path):
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import make_golden_cloud as m; "
            "np.savez(sys.argv[1], **m.generate())" % GOLDEN)
    out = str(tmp_path / "again.npz")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", MPLBACKEND="Agg")
    r = subprocess.run([sys.executable, "-c", code, out], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    with np.load(out) as z:
        assert sorted(z.files) == sorted(rec)
        for k in z.files:
            assert z[k].dtype == rec[k].dtype and z[k].shape == rec[k].shape, k
            assert z[k].tobytes() == rec[k].tobytes(), k


def _cfg(lib, **kw):
    base = dict(B=1, H=48, W=64, stride_y=1, stride_x=1, from_disp=0, compact=0, k_row_stride=4, min_depth=0.1,
                max_depth=10.0, z_lo=0.0, z_hi=0.0)
    base.update(kw)
    cfg = lib.CloudCfg()
    for k, v in base.items():
        setattr(cfg, k, v)
    return cfg


def test_capacity(built):
    l = built.lib()
    n = C.c_int()
    for H, W, sy, sx in ((48, 64, 1, 1), (480, 640, 1, 1), (50, 66, 2, 2), (50, 66, 3, 2), (7, 5, 3, 4), (1, 1, 5, 5)):
        assert l.dvs_cloud_capacity(C.byref(_cfg(built, H=H, W=W, stride_y=sy, stride_x=sx)), C.byref(n)) == 0
        assert n.value == -(-H // sy) * -(-W // sx)
    from deep_visual_slam_amd import pointcloud
    assert pointcloud.capacity(pointcloud.make_cfg(2, 50, 66, (3, 2))) == 17 * 33
    assert pointcloud.workspace_bytes(pointcloud.make_cfg(2, 480, 640)) == 0
    assert pointcloud.workspace_bytes(pointcloud.make_cfg(2, 480, 640, z_range=(0.0, None))) >= 2 * 300 * 4


def test_bad_cloud_arguments_fail_before_any_launch(built):
    l = built.lib()
    n = C.c_int()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    p = (p + 15) & ~15
    bad = [(dict(stride_y=0), b"stride"), (dict(stride_x=-1), b"stride"), (dict(B=0), b"B="), (dict(H=0), b"H="),
           (dict(W=-3), b"W="), (dict(k_row_stride=5), b"k_row_stride"), (dict(k_row_stride=2), b"k_row_stride"),
           (dict(from_disp=1, min_depth=10.0, max_depth=10.0), b"min_depth"),
           (dict(from_disp=1, min_depth=10.0, max_depth=0.1), b"min_depth")]
    for kw, word in bad:
        cfg = _cfg(built, **kw)
        assert l.dvs_cloud_capacity(C.byref(cfg), C.byref(n)) < 0, kw
        assert word in l.dvs_last_error(), (kw, l.dvs_last_error())
        assert l.dvs_cloud_fwd(C.byref(cfg), p, p, p, None, p, p, None, None, None) < 0, kw
        assert word in l.dvs_last_error()
        assert l.dvs_cloud_workspace(C.byref(cfg)) == 0
    ok = _cfg(built)
    assert l.dvs_cloud_capacity(None, C.byref(n)) < 0 and b"null" in l.dvs_last_error()
    assert l.dvs_cloud_capacity(C.byref(ok), None) < 0 and b"null" in l.dvs_last_error()
    args = [p, p, p, None, p, p, None, None, None]          # depth, image, K, M, records, count, index, workspace, stream
    for missing in (0, 1, 2, 4, 5):
        a = list(args)
        a[missing] = None
        assert l.dvs_cloud_fwd(C.byref(ok), *a) < 0, missing
        assert b"null" in l.dvs_last_error()
    assert l.dvs_cloud_fwd(None, *args) < 0 and b"null" in l.dvs_last_error()
    a = list(args)
    a[4] = p + 4                                             # records not 16-byte aligned
    assert l.dvs_cloud_fwd(C.byref(ok), *a) < 0 and b"aligned" in l.dvs_last_error()
    assert l.dvs_cloud_fwd(C.byref(_cfg(built, compact=1)), *args) < 0 and b"workspace" in l.dvs_last_error()
    assert l.dvs_pose_chain(None, None, p, None, None, None, 1, None) < 0 and b"null" in l.dvs_last_error()
    assert l.dvs_pose_chain(p, None, None, None, None, None, 1, None) < 0 and b"null" in l.dvs_last_error()
    assert l.dvs_pose_chain(p, None, p, None, None, None, 0, None) < 0 and b"B=" in l.dvs_last_error()


def test_cpu_tensors_are_rejected(built):
    from deep_visual_slam_amd import pointcloud
    with pytest.raises(built.DvsError):
        pointcloud.depth_to_cloud(torch.zeros(1, 1, 8, 8), torch.zeros(1, 3, 8, 8), torch.eye(4)[None])
    with pytest.raises(built.DvsError):
        pointcloud.PoseChain("cpu")


def test_as_records_is_the_nodes_byte_layout(rec):
    from deep_visual_slam_amd import pointcloud
    assert pointcloud.RECORD_DTYPE.itemsize == 16
    want = rec["ref/node_bytes"][0].view(pointcloud.RECORD_DTYPE)
    host = torch.zeros(2, want.size + 5, 4)                  # capacity larger than the count, two images
    flat = np.stack([want[f] for f in ("x", "y", "z", "rgb")], 1)
    host[0, :want.size] = torch.from_numpy(flat.view(np.int32)).view(torch.float32)       # bit-preserving (rgb may be a NaN pattern)
    views = pointcloud.as_records(host, [want.size, 0])
    assert len(views) == 2 and views[1].size == 0
    assert views[0].dtype == pointcloud.RECORD_DTYPE and views[0].tobytes() == rec["ref/node_bytes"][0].tobytes()
    assert np.shares_memory(views[0], host.numpy())          # zero-copy
    one = pointcloud.as_records(host[0], 7)
    assert one.shape == (7,) and one.tobytes() == rec["ref/node_bytes"][0].tobytes()[:7 * 16]
    assert pointcloud.as_records(host[0]).shape == (want.size + 5,)
    with pytest.raises(Exception):
        pointcloud.as_records(torch.zeros(4, 3))
