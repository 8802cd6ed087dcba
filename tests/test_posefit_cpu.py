"""CPU-side checks of the pose fit (csrc/posefit.hip, raft_video.fit_pose, raft_video.PoseFlowStream): the fp32 restatement of
tests/posefit_ref.py against its fp64 form within the bound derived there, the Jacobian against a difference quotient, recovery of
the T behind the reference's own BackprojectDepth / Project3D (tests/golden/rigidflow.npz), the moving-block scene, and what can be
checked of the entry without a device: the header declares it, the binding lists it, the ABI is still 12, and every argument error
is raised before any launch."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import posefit_ref as P
import rigidflow_ref as R
from conftest import ROOT, load_golden

INF = float("inf")


@pytest.fixture(scope="module")
def rec():
    return load_golden("rigidflow.npz")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


# ---- 1. (a) against (b): the 30 sums ----------------------------------------------------------------------------------------------------
FAMILIES = [(H, W) for H in R.HEIGHTS for W in (1, 5, 64, 131)] + [P.BIG]


@pytest.mark.parametrize("H,W", FAMILIES, ids=["%dx%d" % s for s in FAMILIES])
def test_fp32_sums_against_fp64(H, W):
    """Every entry of the row, fp32 terms summed in fp64 against the all-fp64 form, within posefit_ref.fp32_bound (operation counts
    and sums of absolute values; first order).  The judged sets must be EQUAL: no seeded target lies within a rounding of the
    border.  Measured over these shapes: at most 0.13 of the bound (printed)."""
    worst = 0.0
    for seed, huber in enumerate((INF, 0.5, 1.0)):
        s = P.scene(H, W, seed=seed, noise=0.3, outliers=0.1)
        valid = R.mask(H, W, s.N, seed) if seed == 1 else None
        T0 = P.start(s.N, seed)
        a = P.terms(s.depth, s.flow, s.K, s.iK, T0, valid, huber, s.eps)
        bound, b = P.fp32_bound(s.depth, s.flow, s.K, s.iK, T0, valid, huber, s.eps)
        assert a.term.dtype == np.float32 and b.term.dtype == np.float64
        assert np.array_equal(a.judged, b.judged)
        ra, rb = P.normal(a), P.normal(b)
        assert np.array_equal(ra[:, 29], rb[:, 29]) and np.isfinite(rb).all()
        err = np.abs(ra - rb)
        with np.errstate(all="ignore"):
            share = float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))
        print("%dx%d seed %d huber %g: %d judged, %.3f of the bound" % (H, W, seed, huber, int(rb[:, 29].sum()), share))
        assert (err <= bound).all()
        worst = max(worst, share)
    print("%dx%d: %.3f of the bound" % (H, W, worst))


def test_families_do_what_they_are_for():
    H, W = 7, 64
    by = {c[0]: (c, P.run(c)) for c in P.cases(H, W)}
    assert len(by) == 7
    ls, hub = by["least squares"][1], by["huber"][1]
    assert ls.quadratic[ls.judged].all() and (ls.w[ls.judged] == 1).all()
    q = hub.quadratic[hub.judged]
    assert q.any() and (~q).any()                                                      # both weight branches occur
    assert (hub.w[hub.judged & ~hub.quadratic] < 1).all() and (hub.w[hub.judged & hub.quadratic] == 1).all()
    masked, valid = by["huber and valid"][1], by["huber and valid"][0][3]
    assert not masked.judged[valid == 0].any() and np.array_equal(masked.judged[valid != 0], hub.judged[valid != 0])
    bad, depth = by["depths of 0, negative, NaN, inf"][1], by["depths of 0, negative, NaN, inf"][0][1].depth[:, 0]
    for kind in (depth == 0, depth < 0, np.isnan(depth), np.isposinf(depth)):
        assert kind.any() and not bad.judged[kind].any()
    assert bad.judged.any()
    f = by["NaN and inf flow"][0][2]
    assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any()
    assert not by["NaN and inf flow"][1].judged[~np.isfinite(f).all(axis=1)].any()
    edge = by["edge"][1]
    assert (edge.tx[0] == W - 1).all() and (edge.ty[0] == H - 1).all() and edge.judged[0].all()
    assert not edge.judged[1].any() and (edge.tx[1] > W - 1).any()
    assert edge.judged[2].all() and (edge.tx[2] <= W - 1).all()
    for _, t in by.values():                                                           # a row over judged pixels is finite
        assert np.isfinite(P.normal(t)).all()


def test_jacobian_is_the_derivative_of_the_projection():
    """J against a central difference quotient of (px, py) under T <- exp(h xi_k) T, in fp64: the left perturbation, translation
    first."""
    s = P.scene(7, 13, N=1, seed=4)
    T = P.start(1, 4).astype(np.float64)
    t = P.terms(s.depth, s.flow, s.K, s.iK, T, dtype=np.float64)
    h = 1e-6
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        plus = P.terms(s.depth, s.flow, s.K, s.iK, (P.exp_se3(xi) @ T[0])[None], dtype=np.float64)
        minus = P.terms(s.depth, s.flow, s.K, s.iK, (P.exp_se3(-xi) @ T[0])[None], dtype=np.float64)
        for r, (a, b) in enumerate(((plus.px, minus.px), (plus.py, minus.py))):
            want = (a - b) / (2 * h)
            assert np.allclose(t.J[r][k] + 0 * want, want, rtol=1e-6, atol=1e-6), (k, r)


def test_exp_branches_agree_and_are_rigid():
    for scale in (1e-9, 9.9e-3, 1.01e-2, 0.5, 3.0):
        xi = np.array([0.3, -0.2, 0.1, 0.6, -0.48, 0.64]) * np.array([1, 1, 1, scale, scale, scale])
        E = P.exp_se3(xi)
        assert np.allclose(E[:3, :3] @ E[:3, :3].T, np.eye(3), atol=1e-14) and np.allclose(P.exp_se3(-xi) @ E, np.eye(4), atol=1e-14)


# ---- 2. convergence, recovery, the moving block -----------------------------------------------------------------------------------------
def test_clean_scene_converges_from_the_identity():
    """The issue's scene at 24x32, 77x131 and 7x13: (b) is within 2e-5 after 2 steps (up to the fp32 rounding of the flow it is
    given, ~1e-7 here) and at that rounding after 3."""
    for H, W in ((24, 32), (77, 131), (7, 13)):
        s = P.scene(H, W, N=1, seed=3)
        err = [float(np.abs(P.fit(s.depth, s.flow, s.K, s.iK, iters=it, huber=INF, dtype=np.float64)[0] - s.T).max()) for it in (2, 3)]
        print("%dx%d: %.2e after 2 steps, %.2e after 3" % (H, W, err[0], err[1]))
        assert err[0] < 2e-5 and err[1] < 1e-6


def test_recovery_of_the_reference_geometry(rec):
    """The flow the reference's BackprojectDepth / Project3D produce, from the identity: (b) returns the fixture's T on every
    scene of RECOVERY within RECOVERY_B, and (a) stays within RECOVERY_A_VS_B of (b) -- the measured figure the kernel's
    tolerance is four times of.  The two scenes left out keep fewer than 6 judged pixels: status 1, T the identity."""
    worst_b = worst_ab = 0.0
    for H, W in R.GOLDEN:
        depth, flow, K, iK, T = P.golden_scene(rec, H, W)
        Tb, sb, _ = P.fit(depth, flow, K, iK, iters=P.RECOVERY_ITERS, huber=INF, dtype=np.float64)
        Ta, sa, row = P.fit(depth, flow, K, iK, iters=P.RECOVERY_ITERS, huber=INF)
        if (H, W) not in P.RECOVERY:
            assert row[0, 29] < 6 and sa[0] == sb[0] == 1 and np.array_equal(Ta[0], np.eye(4, dtype=np.float32))
            continue
        eb, eab = float(np.abs(Tb - T).max()), float(np.abs(Ta.astype(np.float64) - Tb).max())
        print("%dx%d: %d judged, (b) - fixture %.2e, (a) - (b) %.2e" % (H, W, int(row[0, 29]), eb, eab))
        assert sa[0] == sb[0] == 0 and eb < P.RECOVERY_B and eab <= P.RECOVERY_A_VS_B
        worst_b, worst_ab = max(worst_b, eb), max(worst_ab, eab)
    print("worst: (b) - fixture %.2e, (a) - (b) %.2e" % (worst_b, worst_ab))
    assert len(P.RECOVERY) >= 3


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_moving_block(dtype):
    """24x32, a 7x7 block displaced by +5 px: the system is well conditioned, one Huber round is pulled by the block, two rounds
    label exactly the block as moving and recover the pose; one round is worse than two by at least 100x."""
    s, block = P.moving_block()
    row = P.normal(P.terms(s.depth, s.flow, s.K, s.iK, np.eye(4, dtype=np.float32)[None], dtype=dtype))
    kappa = float(np.linalg.cond(P.system(row[0])[0]))
    assert kappa < 1e6
    one = P.fit(s.depth, s.flow, s.K, s.iK, iters=4, dtype=dtype)[0]
    two, status, label, _ = P.two_rounds(s, dtype=dtype)
    e1, e2 = float(np.abs(one - s.T).max()), float(np.abs(two - s.T).max())
    print("kappa %.1f, one round %.2e, two rounds %.2e, %d static, %d moving, %d not judged"
          % (kappa, e1, e2, (label == 1).sum(), (label == 2).sum(), (label == 0).sum()))
    assert status[0] == 0 and np.array_equal(label[0] == 2, block) and block.sum() == 49
    assert e1 >= 100 * e2 and e2 <= P.RECOVERY_TOL


def test_degenerate_rows_skip_the_step():
    T = P.start(1)[0]
    s = P.scene(7, 13, N=1)
    row = P.normal(P.terms(s.depth, s.flow, s.K, s.iK, T[None]))[0]
    new, taken = P.step(row, T)
    assert taken and not np.array_equal(new, T)
    few = row.copy()
    few[29] = 5
    nan = row.copy()
    nan[3] = np.nan
    singular = row.copy()
    singular[:21] = 0.0
    negative = row.copy()
    negative[0] = -1.0
    for bad in (few, nan, singular, negative, np.zeros(30)):
        kept, taken = P.step(bad, T)
        assert not taken and kept is T


# ---- 3. header, binding, ABI, refusals --------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entries(built):
    src = open(os.path.join(ROOT, "include", "dvslam.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+dvs_pose_fit\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m and m.group(1).count(",") + 1 == 24
    assert re.search(r"\bsize_t\s+dvs_pose_fit_workspace\s*\(\s*int N, int H, int W\s*\)\s*;", code)
    for name, n in (("dvs_pose_fit", 24), ("dvs_pose_fit_workspace", 3)):
        assert name in built.exported_symbols() and len(built._SIGNATURES[name][1]) == n and hasattr(built.lib(), name)
    for line in ("qx = ((T[0][0]*X + T[0][1]*Y) + T[0][2]*Z) + T[0][3]", "A[r][k] = (K[r][k] - p_r*K[2][k]) / den",
                 "J[r] = (A[r][0], A[r][1], A[r][2], A[r][2]*qy - A[r][1]*qz, A[r][0]*qz - A[r][2]*qx, A[r][1]*qx - A[r][0]*qy)",
                 "w  = 1 if e2 <= huber*huber, else huber / sqrt(e2)", "A = H + damping * diag(H)"):
        assert line in src, line
    papers = open(os.path.join(ROOT, "PAPERS.md")).read()
    assert "D3VO" in papers and "Huber" in papers and "GeoNet" in papers
    kernel = open(os.path.join(ROOT, "deep-visual-slam_amd", "csrc", "posefit.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel and "atomic" not in kernel.replace("no atomics", "")
    assert "hipMemset" not in kernel


def test_abi_is_still_12(built):
    assert built.ABI_VERSION == 12 and built.lib().dvs_abi_version() == 12


def test_workspace_depends_on_the_shape_alone(built):
    ws = built.lib().dvs_pose_fit_workspace
    assert ws(1, 1, 1) == 240 and ws(3, 1, 1) == 3 * 240 and ws(1, 7, 131) == 240 and ws(1, 77, 131) == 10 * 240
    assert ws(1, 480, 640) == 150 * 240 and ws(2, 480, 640) == 2 * ws(1, 480, 640)      # 300 blocks of lanes: 150 groups, 2 walks
    assert ws(0, 5, 7) == 0 and ws(1, 0, 7) == 0 and ws(1, 5, (1 << 24) + 1) == 0 and ws(65536, 5, 7) == 0


P0 = 1 << 20      # non-NULL, 16-byte aligned "device pointers" a MiB apart: nothing dereferences them before the checks fail


def _entry(l, depth=P0, d_image=35, d_row=7, K=2 * P0, iK=3 * P0, T0=4 * P0, flow=5 * P0, f_image=70, f_plane=35, f_row=7, valid=6 * P0,
           T=7 * P0, status=8 * P0, normal=9 * P0, workspace=10 * P0, workspace_bytes=480, N=2, H=5, W=7, iters=4, huber=1.0,
           damping=1e-6, eps=1e-7):
    return l.dvs_pose_fit(depth, d_image, d_row, K, iK, T0, flow, f_image, f_plane, f_row, valid, T, status, normal, workspace,
                          workspace_bytes, N, H, W, iters, huber, damping, eps, None)


BAD_CALLS = [
    ("NULL depth", dict(depth=None)),
    ("NULL K", dict(K=None)),
    ("NULL inv_K", dict(iK=None)),
    ("NULL T0", dict(T0=None)),
    ("NULL flow", dict(flow=None)),
    ("NULL T", dict(T=None)),
    ("NULL status", dict(status=None)),
    ("NULL workspace", dict(workspace=None)),
    ("misaligned depth", dict(depth=P0 + 2)),
    ("misaligned T0", dict(T0=4 * P0 + 1)),
    ("misaligned flow", dict(flow=5 * P0 + 2)),
    ("misaligned T", dict(T=7 * P0 + 2)),
    ("misaligned status", dict(status=8 * P0 + 1)),
    ("misaligned normal", dict(normal=9 * P0 + 4)),
    ("misaligned workspace", dict(workspace=10 * P0 + 4)),
    ("N = 0", dict(N=0)),
    ("N = 65536", dict(N=65536)),
    ("H = 0", dict(H=0)),
    ("W = -1", dict(W=-1)),
    ("W past 2^24", dict(W=(1 << 24) + 1, H=1, d_row=1 << 25, d_image=1 << 25, f_row=1 << 25, f_plane=1 << 25, f_image=1 << 26)),
    ("too many lanes", dict(H=1 << 24, W=1 << 24, d_row=1 << 24, f_row=1 << 24)),
    ("depth row stride < W", dict(d_row=6)),
    ("depth image stride < the image", dict(d_image=34)),
    ("flow row stride < W", dict(f_row=6)),
    ("flow plane stride < the plane", dict(f_plane=34)),
    ("flow image stride < two planes", dict(f_image=69)),
    ("stride out of range", dict(d_row=1 << 41, d_image=1 << 45)),
    ("flow stride out of range", dict(f_row=1 << 41, f_plane=1 << 45, f_image=1 << 47)),
    ("huber = 0", dict(huber=0.0)),
    ("huber < 0", dict(huber=-1.0)),
    ("huber NaN", dict(huber=float("nan"))),
    ("damping < 0", dict(damping=-1e-6)),
    ("damping inf", dict(damping=INF)),
    ("damping NaN", dict(damping=float("nan"))),
    ("eps < 0", dict(eps=-1e-7)),
    ("eps NaN", dict(eps=float("nan"))),
    ("eps inf", dict(eps=INF)),
    ("iters = -1", dict(iters=-1)),
    ("iters = 65", dict(iters=65)),
    ("workspace short", dict(workspace_bytes=479)),
    ("T overlaps depth", dict(T=P0)),
    ("T overlaps the end of depth", dict(T=P0 + 4 * (35 + 4 * 7 + 6))),
    ("T overlaps T0 but is not T0", dict(T=4 * P0 + 64)),
    ("status overlaps flow", dict(status=5 * P0 + 16)),
    ("normal overlaps valid", dict(normal=6 * P0 + 64)),
    ("workspace overlaps K", dict(workspace=2 * P0 - 8)),
    ("workspace overlaps inv_K", dict(workspace=3 * P0 + 120)),
    ("status overlaps T", dict(status=7 * P0 + 124)),
    ("normal overlaps the workspace", dict(normal=10 * P0 + 472)),
]


@pytest.mark.parametrize("name,kw", BAD_CALLS, ids=[b[0] for b in BAD_CALLS])
def test_entry_refuses_bad_arguments(built, name, kw):
    l = built.lib()
    assert _entry(l, **kw) == -1                     # DVS_ERR_INVALID: no launch was tried (this machine has no GPU to refuse one)
    assert b"dvs_pose_fit" in l.dvs_last_error()


def test_messages_say_what_is_wrong(built):
    l = built.lib()
    assert _entry(l, d_row=6) < 0 and b"depth row stride 6 is below W=7" in l.dvs_last_error()
    assert _entry(l, huber=0.0) < 0 and b"huber=0 must be above 0" in l.dvs_last_error()
    assert _entry(l, iters=65) < 0 and b"iters=65 must be in 0 .. 64" in l.dvs_last_error()
    assert _entry(l, workspace_bytes=479) < 0 and b"workspace of 479 bytes is below dvs_pose_fit_workspace = 480" in l.dvs_last_error()
    assert _entry(l, T=4 * P0 + 64) < 0 and b"output T overlaps input T0" in l.dvs_last_error()
    assert _entry(l, normal=10 * P0 + 472) < 0 and b"output normal overlaps output workspace" in l.dvs_last_error()


def test_fit_pose_signature_and_cpu_tensors(built):
    from deep_visual_slam_amd import raft_video
    E = built.DvsError
    params = inspect.signature(raft_video.fit_pose).parameters
    assert list(params)[:11] == ["depth", "flow", "K", "inv_K", "T0", "valid", "iters", "huber", "damping", "eps", "normal"]
    assert [params[k].default for k in list(params)[3:11]] == [None, None, None, 4, 1.0, 1e-6, 1e-7, False]
    d, f, m = torch.ones(2, 1, 5, 7), torch.zeros(2, 2, 5, 7), torch.eye(4)
    with pytest.raises(E, match="fit_pose: depth: GPU tensors only .* no CPU path"):
        raft_video.fit_pose(d, f, m)


class _Stand:
    """What the argument checks read of a tensor (is_cuda, dtype, dim(), shape, device): a GPU tensor's stand-in on a machine
    without one."""

    def __init__(self, shape, dtype=torch.float32, device="cuda:0"):
        self.shape, self.dtype, self.device, self.is_cuda = torch.Size(shape), dtype, torch.device(device), True

    def dim(self):
        return len(self.shape)


def test_fit_pose_refuses_mismatches_before_any_launch(built, monkeypatch):
    """Every shape, dtype or device mismatch and every bad parameter: raised by the argument checks, which read nothing but the
    tensors' descriptions; neither the library nor a tensor method that would copy is reached."""
    from deep_visual_slam_amd import raft_video
    E = built.DvsError
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (_Stand, torch.Tensor)))
    monkeypatch.setattr(raft_video._lib, "lib", lambda: pytest.fail("the library was reached"))
    S = _Stand
    ok = dict(depth=S((2, 1, 5, 7)), flow=S((2, 2, 5, 7)), K=S((4, 4)), inv_K=S((2, 4, 4)), T0=S((2, 4, 4)),
              valid=S((2, 5, 7), dtype=torch.uint8))
    bad = [
        (dict(depth=S((2, 2, 5, 7))), r"depth: \[N,1,H,W\] or \[N,H,W\] expected, got \(2, 2, 5, 7\)"),
        (dict(depth=S((2, 1, 5, 7), dtype=torch.float64)), r"depth: fp32 only, got torch.float64"),
        (dict(flow=None), "flow: a measured flow"),
        (dict(flow=S((2, 2, 5, 8))), r"flow: \[2,2,5,7\] expected, got \(2, 2, 5, 8\)"),
        (dict(flow=S((2, 2, 5, 7), dtype=torch.float16)), r"flow: fp32 only"),
        (dict(T0=S((4, 4))), r"T0: \[2,4,4\] expected, got \(4, 4\)"),
        (dict(T0=S((2, 4, 4), dtype=torch.float64)), r"T0: fp32 only"),
        (dict(T0=S((2, 4, 4), device="cuda:1")), r"T0 is on cuda:1, depth on cuda:0"),
        (dict(K=S((3, 3))), r"K: \[2,4,4\] or \[4,4\] expected, got \(3, 3\)"),
        (dict(inv_K=S((2, 3, 3))), r"inv_K: \[2,4,4\] or \[4,4\] expected"),
        (dict(valid=S((2, 5, 7))), r"valid: uint8 \[2,5,7\] expected .* got torch.float32"),
        (dict(valid=S((2, 5, 7), dtype=torch.uint8, device="cuda:1")), r"valid is on cuda:1"),
        (dict(iters=-1), r"iters=-1 must be in 0 \.\. 64"),
        (dict(iters=65), r"iters=65 must be in 0 \.\. 64"),
        (dict(huber=0.0), "huber=0.0 must be above 0"),
        (dict(huber=float("nan")), "huber=nan must be above 0"),
        (dict(damping=-1.0), ".* must be finite and not negative"),
        (dict(damping=INF), ".* must be finite and not negative"),
        (dict(eps=float("nan")), ".* must be finite and not negative"),
    ]
    for kw, msg in bad:
        with pytest.raises(E, match="fit_pose: " + msg):
            raft_video.fit_pose(**{**ok, **kw})
    for kw in (dict(T0=None, iters=-1), dict(T0=None, K=S((3, 3)))):                   # without a guess the same checks are made
        with pytest.raises(E, match="fit_pose: "):
            raft_video.fit_pose(**{**ok, **kw})


def test_stream_signatures(built):
    """PoseFlowStream is a subclass: RigidFlowStream's and FlowStream's constructors and FlowStream.push keep their signatures,
    FlowFrame its positional part; the new fields are None elsewhere."""
    from deep_visual_slam_amd import raft, raft_video
    params = inspect.signature(raft_video.PoseFlowStream.__init__).parameters
    assert list(params)[-4:-1] == ["pose_iters", "pose_huber", "pose_rounds"]
    assert [params[k].default for k in list(params)[-4:-1]] == [4, 1.0, 2]
    assert list(inspect.signature(raft_video.PoseFlowStream.push).parameters) == ["self", "frame", "depth", "K", "inv_K", "T"]
    assert list(inspect.signature(raft_video.FlowStream.push).parameters) == ["self", "frame", "depth", "T", "K", "inv_K"]
    assert list(inspect.signature(raft_video.FlowFrame.__init__).parameters)[:11] == [
        "self", "flow_low", "flow_up", "image", "slot", "flow_low_bw", "flow_up_bw", "valid", "valid_bw", "rigid", "motion"]
    model = raft.SmallRAFT().eval()
    pose = raft_video.PoseFlowStream(model, iters=3, bidirectional=True, rigid_beta=0.75, pose_iters=5, pose_rounds=1, pose_huber=2.0)
    assert isinstance(pose, raft_video.RigidFlowStream) and pose.rigid is True
    assert (pose.iters, pose.bidirectional, pose.rigid_beta, pose.pose_iters, pose.pose_rounds, pose.pose_huber) == (3, True, 0.75, 5, 1, 2.0)
    for kw in (dict(pose_iters=0), dict(pose_iters=65), dict(pose_rounds=0), dict(pose_huber=0.0), dict(pose_huber=float("nan"))):
        with pytest.raises(built.DvsError, match="pose_iters"):
            raft_video.PoseFlowStream(model, **kw)
    frame = raft_video.FlowFrame(None, None, None)
    assert (frame.T, frame.pose_status) == (None, None)
    with pytest.raises(built.DvsError, match="host=True only"):
        frame.T_host
