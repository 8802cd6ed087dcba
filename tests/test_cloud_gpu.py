"""Output stage on the GPU (csrc/cloud.hip, pointcloud.py, inference.CloudPredictor) against the fixture recorded from the
reference's own routines (tests/golden/cloud_b2_48x64.npz) and, where no fixture fits, against tests/cloud_ref.py.

Positions: within 3 x the largest error of cloud_ref's fp32 variant on the same inputs (measured in the test), never below
2 ulp of the largest |coordinate| -- the kernel may contract to FMAs and divide differently from numpy.  Colours, record
order, counts and indices: bit for bit."""
import numpy as np
import pytest
import torch

import cloud_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
NAN_PATTERN = 0x7FC0BEEF


@pytest.fixture(scope="module")
def rec():
    return load_golden("cloud_b2_48x64.npz")


def bound(ref64, ref32):
    """3 x the fp32 restatement's own error, floor 2 ulp of the largest |coordinate|."""
    floor = 2.0 * float(np.spacing(np.float32(np.abs(ref64).max())))
    return max(3.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()), floor)


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def split(records, n=None):
    """device [n_max,4] -> (xyz float64 [n,3], rgb bits uint32 [n])."""
    a = records.detach().cpu().numpy()
    a = a if n is None else a[:n]
    return a[:, :3].astype(np.float64), a[:, 3].copy().view(np.uint32)


def rgb_bits(col):
    return R.pack_rgb(col).view(np.uint32)


def check_cloud(got_xyz, got_rgb, want64, want32, col):
    assert got_xyz.shape == want64.shape
    err, b = float(np.abs(got_xyz - want64).max()) if want64.size else 0.0, bound(want64, want32) if want64.size else 0.0
    print("cloud: max |err| %.3e, bound %.3e (%d points)" % (err, b, want64.shape[0]))
    assert err <= b, (err, b)
    assert np.array_equal(got_rgb, rgb_bits(col))


@pytest.mark.parametrize("from_disp", [False, True])
def test_fixture_dense_camera_and_world(gpu_device, rec, from_disp):
    from deep_visual_slam_amd import pointcloud
    image, K, left = rec["in/image"], rec["in/K"], rec["in/left"]
    src = rec["in/disp"] if from_disp else rec["in/depth"]
    fd = (0.1, 10.0) if from_disp else None
    M = np.stack([left @ rec["in/pose"][b] for b in range(2)])          # a sign flip of one row: exact in fp32
    for frame in ("camera", "world"):
        recs, count = pointcloud.depth_to_cloud(dev(src, gpu_device), dev(image, gpu_device), dev(K, gpu_device),
                                                dev(M, gpu_device) if frame == "world" else None, from_disp=fd)
        torch.cuda.synchronize()
        assert recs.shape == (2, 48 * 64, 4) and count.tolist() == [48 * 64] * 2
        for b in range(2):
            want = rec["ref/vis_world"][b] if frame == "world" else rec["ref/vis_cam"][b] * np.array([1.0, -1.0, 1.0])
            z32 = R.disp_to_depth(src[b, 0], 0.1, 10.0, np.float32) if from_disp else src[b, 0]
            ref32, _, _ = R.cloud(z32, image[b], K[b], M[b] if frame == "world" else None, np.float32)
            xyz, rgb = split(recs[b])
            check_cloud(xyz, rgb, want, ref32, rec["ref/colors"][b])
            if frame == "camera" and not from_disp:                     # the node's PointCloud2.data: rgb field bit for bit
                node = rec["ref/node_bytes"][b].view(pointcloud.RECORD_DTYPE)
                host = pointcloud.as_records(recs[b].cpu())
                assert np.array_equal(host["rgb"].view(np.uint32), node["rgb"].view(np.uint32))


def nan_filled(B, n, device):
    return torch.full((B, n, 4), 0, dtype=torch.int32, device=device).fill_(NAN_PATTERN).view(torch.float32)


def test_fixture_compact_matches_eval_traj(gpu_device, rec):
    from deep_visual_slam_amd import pointcloud
    image, K, pose = rec["in/image"], rec["in/K"], rec["in/pose"]
    n_max = 48 * 64
    cases = {"masked": rec["in/depth_masked"], "none kept": np.zeros_like(rec["in/depth"]), "all kept": rec["in/depth"]}
    for name, depth in cases.items():
        out = nan_filled(2, n_max, gpu_device)
        index = torch.full((2, n_max), -7, dtype=torch.int32, device=gpu_device)
        recs, count = pointcloud.depth_to_cloud(dev(depth, gpu_device), dev(image, gpu_device), dev(K, gpu_device),
                                                dev(pose, gpu_device), z_range=(0.0, None), out=out, index=index)
        torch.cuda.synchronize()
        assert recs.data_ptr() == out.data_ptr()
        for b in range(2):
            want64, col, idx = R.cloud(depth[b, 0], image[b], K[b], pose[b], z_range=(0.0, None))
            ref32, _, _ = R.cloud(depth[b, 0], image[b], K[b], pose[b], np.float32, z_range=(0.0, None))
            n = int(count[b])
            assert n == idx.size, name
            if name == "masked":
                assert np.array_equal(idx, rec["ref/eval_index%d" % b])
                want64 = rec["ref/eval_points%d" % b]
            assert n == {"masked": n, "none kept": 0, "all kept": n_max}[name]
            assert np.array_equal(index[b, :n].cpu().numpy(), idx)
            assert bool((index[b, n:] == -7).all())
            xyz, rgb = split(recs[b], n)
            check_cloud(xyz, rgb, want64, ref32, col)
            tail = out[b, n:].view(torch.int32)
            assert bool((tail == NAN_PATTERN).all()), "%s: records at or beyond count[b] were written" % name


def test_fullsize_compact_range_from_disp(gpu_device):
    from deep_visual_slam_amd import pointcloud
    B, H, W, z_lo, z_hi = 2, 480, 640, 0.5, 5.0
    g = torch.Generator().manual_seed(31)
    disp = torch.rand(B, 1, H, W, generator=g).numpy()
    image = torch.rand(B, 3, H, W, generator=g).numpy()
    near = lambda d: (np.abs(d / z_lo - 1.0) < 1e-4) | (np.abs(d / z_hi - 1.0) < 1e-4)
    disp[near(R.disp_to_depth(disp, 0.1, 10.0))] = 0.5                  # depth 0.198: far from both limits
    assert int(near(R.disp_to_depth(disp, 0.1, 10.0)).sum()) == 0      # a condition on the input, not on the kernel
    K = np.tile(np.array([[0.58 * W, 0, 0.5 * W], [0, 0.77 * H, 0.5 * H], [0, 0, 1]], np.float32), (B, 1, 1))   # [B,3,3]
    pose = load_golden("cloud_b2_48x64.npz")["in/pose"]
    index = torch.empty(B, H * W, dtype=torch.int32, device=gpu_device)
    out = nan_filled(B, H * W, gpu_device)
    recs, count = pointcloud.depth_to_cloud(dev(disp, gpu_device), dev(image, gpu_device), dev(K, gpu_device),
                                            dev(pose, gpu_device), from_disp=(0.1, 10.0), z_range=(z_lo, z_hi), out=out,
                                            index=index)
    torch.cuda.synchronize()
    for b in range(B):
        want64, col, idx = R.cloud(R.disp_to_depth(disp[b, 0], 0.1, 10.0), image[b], K[b], pose[b], z_range=(z_lo, z_hi))
        ref32, _, idx32 = R.cloud(R.disp_to_depth(disp[b, 0], 0.1, 10.0, np.float32), image[b], K[b], pose[b], np.float32,
                                  z_range=(z_lo, z_hi))
        assert np.array_equal(idx, idx32)
        n = int(count[b])
        assert n == idx.size and 0 < n < H * W
        assert np.array_equal(index[b, :n].cpu().numpy(), idx)
        xyz, rgb = split(recs[b], n)
        check_cloud(xyz, rgb, want64, ref32, col)
        assert bool((out[b, n:].view(torch.int32) == NAN_PATTERN).all())


def unaligned(a, device):
    """The same values in a contiguous device tensor whose address is 4 bytes past a 16-byte boundary."""
    t = torch.empty(a.size + 1, dtype=torch.float32, device=device)[1:].view(*a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


@pytest.mark.parametrize("H,W,stride,shift", [(48, 64, (2, 2), False), (48, 64, (3, 2), False), (48, 64, (3, 1), False),
                                              (50, 66, (1, 1), False), (50, 66, (3, 2), False), (48, 64, (1, 1), True),
                                              (48, 64, (2, 1), True)])
def test_strides_odd_shapes_and_unaligned_inputs(gpu_device, H, W, stride, shift):
    from deep_visual_slam_amd import pointcloud
    B = 2
    g = torch.Generator().manual_seed(100 + H + 7 * stride[0] + stride[1])
    depth = (torch.rand(B, 1, H, W, generator=g) * 9 + 0.2).numpy()
    depth[torch.rand(B, 1, H, W, generator=g).numpy() < 0.25] = 0.0
    image = torch.rand(B, 3, H, W, generator=g).numpy()
    K = np.tile(np.array([[0.6 * W, 0, 0.48 * W, 0], [0, 0.8 * H, 0.51 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32), (B, 1, 1))
    pose = load_golden("cloud_b2_48x64.npz")["in/pose"]
    put = unaligned if shift else dev
    n_max = -(-H // stride[0]) * -(-W // stride[1])
    for z_range in (None, (0.0, 6.0)):
        out = nan_filled(B, n_max, gpu_device)
        index = torch.full((B, n_max), -7, dtype=torch.int32, device=gpu_device)
        recs, count = pointcloud.depth_to_cloud(put(depth, gpu_device), put(image, gpu_device), dev(K, gpu_device),
                                                dev(pose, gpu_device), stride=stride, z_range=z_range, out=out, index=index)
        torch.cuda.synchronize()
        for b in range(B):
            want64, col, idx = R.cloud(depth[b, 0], image[b], K[b], pose[b], stride=stride, z_range=z_range)
            ref32, _, _ = R.cloud(depth[b, 0], image[b], K[b], pose[b], np.float32, stride=stride, z_range=z_range)
            n = int(count[b])
            assert n == idx.size and (z_range is not None or n == n_max)
            assert np.array_equal(index[b, :n].cpu().numpy(), idx)
            xyz, rgb = split(recs[b], n)
            check_cloud(xyz, rgb, want64, ref32, col)
            assert bool((out[b, n:].view(torch.int32) == NAN_PATTERN).all())


def quat_close(got, want, tol):
    """Equal up to the sign convention where qw is (numerically) zero."""
    d = min(np.abs(got - want).max(), np.abs(got + want).max()) if abs(want[3]) < 1e-3 else np.abs(got - want).max()
    return d <= tol


def test_pose_chain(gpu_device, rec):
    from deep_visual_slam_amd import pointcloud
    T, left = rec["chain/T"], rec["in/left"]
    Td = dev(T, gpu_device)
    a = pointcloud.PoseChain(gpu_device, left=left)
    poses, M, tq = a.step(Td)
    b = pointcloud.PoseChain(gpu_device, left=left)
    one = [b.step(Td[i:i + 1]) for i in range(64)]
    torch.cuda.synchronize()
    assert torch.equal(a.world, b.world) and torch.equal(a.world, poses[-1])         # bit for bit
    assert torch.equal(torch.cat([o[0] for o in one]), poses) and torch.equal(torch.cat([o[2] for o in one]), tq)
    want = rec["chain/T_global"]
    ref32, _ = R.pose_chain(T, dtype=np.float32)
    lim = max(3.0 * float(np.abs(ref32.astype(np.float64) - want).max()), 64 * EPS * float(np.abs(want).max()))
    got = poses.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    print("pose chain: max |err| %.3e, bound %.3e" % (err, lim))
    assert err <= lim
    Mh = M.cpu().numpy()
    assert np.array_equal(Mh, left[None] @ poses.cpu().numpy())          # left is a sign flip: exact
    assert np.array_equal(Mh[:, 1], -poses.cpu().numpy()[:, 1])
    # quaternion against the fp64 routine on the kernel's own poses: ~16 fp32 roundings of unit-size numbers
    tqh = tq.cpu().numpy().astype(np.float64)
    for i in range(64):
        w = R.tq(got[i])
        assert np.array_equal(tqh[i, :3], got[i, :3, 3])
        assert quat_close(tqh[i, 3:], w[3:], 8 * EPS), (i, tqh[i], w)
        assert tqh[i, 6] >= 0 and abs(np.linalg.norm(tqh[i, 3:]) - 1) <= 4 * EPS
    # M = world when there is no left; init; a half turn about y (1 + trace == 0: the node's formula divides by zero)
    init = np.eye(4, dtype=np.float32)
    init[:3, 3] = [0.0, -2.0, 0.0]                                       # Visualizer's start pose
    c = pointcloud.PoseChain(gpu_device, init=init)
    assert np.array_equal(c.world.cpu().numpy(), init)
    half = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)
    p, m, q = c.step(dev(half[None], gpu_device))
    torch.cuda.synchronize()
    assert torch.equal(p, m) and np.array_equal(p[0].cpu().numpy(), init @ half)
    qh = q[0].cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(qh)) and np.array_equal(qh[:3], [0.0, -2.0, 0.0])
    assert quat_close(qh[3:], R.quaternion(half[:3, :3]), 8 * EPS), qh
    c.reset()
    assert np.array_equal(c.world.cpu().numpy(), np.eye(4, dtype=np.float32))


# ----------------------------------------------------------------------------------------------- CloudPredictor
def _randomise_bn(net, seed):
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.5 + 0.25)
            m.weight.data.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.num_features, generator=g) * 0.1)


@pytest.fixture(scope="module")
def eval_nets(gpu_device):
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.posenet_single import PoseNet
    torch.manual_seed(0)
    dn, pn = DepthNet(18, pretrained=False), PoseNet(18, pretrained=False, num_input_images=2)
    _randomise_bn(dn, 1)
    _randomise_bn(pn, 2)
    return dn.to(gpu_device).eval(), pn.to(gpu_device).eval()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def chain_bound(want64, ref32):
    return max(3.0 * float(np.abs(ref32.astype(np.float64) - want64).max()), 64 * EPS * float(np.abs(want64).max()))


@pytest.mark.parametrize("H,W,graph,z_range,d2h", [(96, 128, False, None, "full"), (96, 128, True, None, "full"),
                                                   (96, 128, True, (0.2, 5.0), "full"), (96, 128, True, (0.2, 5.0), "count"),
                                                   (480, 640, True, None, "full")])
def test_cloud_predictor(gpu_device, eval_nets, H, W, graph, z_range, d2h):
    from deep_visual_slam_amd import inference, pointcloud
    dn, pn = eval_nets
    inference.prepare(dn, pn, scales=(0,))
    try:
        g = torch.Generator().manual_seed(40 + H)
        frames = [(torch.rand(1, 3, H, W, generator=g).to(gpu_device), torch.rand(1, 6, H, W, generator=g).to(gpu_device))
                  for _ in range(5)]
        K = dev(np.array([[[0.58 * W, 0, 0.5 * W, 0], [0, 0.77 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], np.float32), gpu_device)
        left = np.diag([1.0, -1.0, 1.0, 1.0]).astype(np.float32)
        init = np.eye(4, dtype=np.float32)
        init[:3, 3] = [0.0, -2.0, 0.0]
        fp = inference.FramePredictor(dn, pn, torch.zeros_like(frames[0][0]), torch.zeros_like(frames[0][1]), graph=False)
        cp = inference.CloudPredictor(dn, pn, torch.zeros_like(frames[0][0]), torch.zeros_like(frames[0][1]), K, left=left,
                                      init=init, z_range=z_range, graph=graph, d2h=d2h)
        torch.cuda.synchronize()
        assert np.array_equal(cp.world.cpu().numpy(), init)             # warm-up and capture did not advance the pose
        n_max = H * W
        Ts, world64, world32, prev = [], init.astype(np.float64), init.copy(), None
        for i, (x, x6) in enumerate(frames):
            T0, depth0, disp0 = [t.clone() for t in fp(x, x6)]
            f = cp(x, x6)
            assert rel(f.T, T0) < 1e-5 and rel(f.depth, depth0) < 1e-5 and rel(f.disp, disp0) < 1e-5
            Th = f.T[0].cpu().numpy()
            world64, world32 = world64 @ Th.astype(np.float64), world32 @ Th
            wp = f.world_pose.copy()
            assert np.abs(wp.astype(np.float64) - world64).max() <= chain_bound(world64, world32)
            assert np.array_equal(wp, cp.world.cpu().numpy())
            assert np.array_equal(f.tq[0, :3], wp[:3, 3]) and quat_close(f.tq[0, 3:].astype(np.float64), R.quaternion(wp[:3, :3]), 8 * EPS)
            # the same cloud, made separately from the returned disparity and world pose
            M = (left @ wp)[None]
            recs, count = pointcloud.depth_to_cloud(f.disp, x, K, dev(M, gpu_device), from_disp=(0.1, 10.0), z_range=z_range)
            torch.cuda.synchronize()
            n = int(count[0])
            assert int(f.count[0]) == n and (z_range is not None or n == n_max)
            mine = f.records
            assert mine.dtype == pointcloud.RECORD_DTYPE and mine.shape == (n,)
            assert mine.tobytes() == pointcloud.as_records(recs[0].cpu(), n).tobytes()
            if prev is not None:                                        # frame i-1's view survived call i (two buffers)
                assert prev[0].tobytes() == prev[1]
            prev = (mine, mine.tobytes())
        if graph:                                                       # stale weights: re-capture, the pose advances once
            w0 = cp.world.cpu().numpy().copy()
            dn.load_state_dict({k: v.clone() for k, v in dn.state_dict().items()})
            assert cp.stale()
            f = cp(*frames[0])
            again = pointcloud.PoseChain(gpu_device, init=w0)          # the kernel's own single step from w0, bit for bit:
            again.step(f.T.clone())                                     # neither none nor two were taken
            torch.cuda.synchronize()
            assert not np.array_equal(f.T[0].cpu().numpy(), np.eye(4, dtype=np.float32))
            assert np.array_equal(f.world_pose, again.world.cpu().numpy())
            assert np.array_equal(cp.world.cpu().numpy(), again.world.cpu().numpy())
            assert not cp.stale()
    finally:
        dn.inference_scales = None
