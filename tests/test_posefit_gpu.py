"""dvs_pose_fit on the GPU (csrc/posefit.hip, raft_video.fit_pose) against tests/posefit_ref.py.

The accumulate launch forms the same fp32 terms as the restatement (a) -- every operation is correctly rounded on both sides and
contraction is off -- and adds them in fp64 in another order: the judged count must be EQUAL, a single pixel's terms the SAME BITS
(a one-hot mask isolates them), and every sum within n 2^-53 sum|term| (posefit_ref.sum_bound: the bound the issue sets).  The update
launch is held against the fp64 update of posefit_ref applied to the kernel's OWN row.  Shapes: W in {1, 3, 4, 5, 63, 64, 65, 131} x
H in {1, 2, 7} and 131x77, N in {1, 3}.  Measured on the MI355X: DESIGN.md section 26."""
import functools

import numpy as np
import pytest
import torch

import layouts
import posefit_ref as P
import rigidflow_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import raft_video
    return raft_video


@functools.lru_cache(maxsize=None)
def cases(H, W):
    return P.cases(H, W)


def dev(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def args_of(case, device, N=3):
    name, s, flow, valid, huber, T0 = case
    return dict(depth=dev(s.depth[:N], device), flow=dev(flow[:N], device), K=dev(s.K, device), inv_K=dev(s.iK, device),
                T0=dev(T0[:N], device), valid=dev(None if valid is None else valid[:N], device), huber=huber, eps=s.eps)


def want_of(case, N=3):
    name, s, flow, valid, huber, T0 = case
    return P.terms(s.depth[:N], flow[:N], s.K, s.iK, T0[:N], None if valid is None else valid[:N], huber, s.eps)


SHAPES = P.SIZES + [P.BIG]


@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_accumulation_against_the_restatement(gpu_device, V, H, W):
    """iters = 0 with normal: the sums at T0.  T comes back as T0 (bits) and status 0."""
    worst, launches, branches = 0.0, 0, [False, False]
    for case in cases(H, W):
        for N in (3, 1):
            want = want_of(case, N)
            kw = args_of(case, gpu_device, N)
            T, status, row = V.fit_pose(iters=0, normal=True, **kw)
            assert row.dtype == torch.float64 and tuple(row.shape) == (N, 30) and status.dtype == torch.int32
            assert torch.equal(T.view(torch.int32), kw["T0"].view(torch.int32)) and not status.any()
            got, ref, bound = row.cpu().numpy(), P.normal(want), P.sum_bound(want)
            assert np.array_equal(got[:, 29], ref[:, 29]), case[0]                     # the judged count
            err = np.abs(got - ref)
            assert (err <= bound).all(), (case[0], N, float((err - bound).max()))
            with np.errstate(all="ignore"):
                worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
            launches += 1
            j = want.judged
            branches[0] |= bool(want.quadratic[j].any())
            branches[1] |= bool((~want.quadratic[j]).any())
    print("%dx%d: %d launches, at most %.3f of n 2^-53 sum|term|" % (H, W, launches, worst))
    assert all(branches)                                                                # both weight branches occurred


@pytest.mark.parametrize("H,W", [(7, 5), (7, 4)], ids=["scalar", "vector"])
def test_one_pixel_terms_are_the_same_bits(gpu_device, V, H, W):
    """A mask with one pixel set per image: the row IS that pixel's 30 fp32 terms, widened -- bit for bit the restatement's."""
    case = cases(H, W)[1]
    assert case[0] == "huber"
    want = want_of(case)
    kw = args_of(case, gpu_device)
    term = want.term.astype(np.float64)
    seen = 0
    for y in range(H):
        for x in range(W):
            mask = np.zeros((3, H, W), np.uint8)
            mask[:, y, x] = 1
            row = V.fit_pose(iters=0, normal=True, **{**kw, "valid": dev(mask, gpu_device)})[2].cpu().numpy()
            for n in range(3):
                ref = term[n, :, y, x] if want.judged[n, y, x] else np.zeros(30)
                assert np.array_equal(row[n].view(np.int64), ref.view(np.int64)), (n, y, x)
                seen += int(want.judged[n, y, x])
    assert seen > H * W


UPDATE_SHAPES = [(1, 64), (2, 5), (7, 4), (7, 65), (7, 131), P.BIG]


@pytest.mark.parametrize("H,W", UPDATE_SHAPES, ids=["%dx%d" % s for s in UPDATE_SHAPES])
def test_update_against_fp64_on_the_kernels_own_row(gpu_device, V, H, W):
    """One iteration against posefit_ref.step applied to the row the kernel itself summed at T0; the bound is
    posefit_ref.update_bound, derived there: the fp32 rounding of the result plus kappa(A) c 2^-53 |xi| carried through exp and
    the product with T0."""
    worst = 0.0
    for case in cases(H, W)[:3]:
        kw = args_of(case, gpu_device)
        _, _, row = V.fit_pose(iters=0, normal=True, **kw)
        T1, status = V.fit_pose(iters=1, **kw)
        row, T1, T0 = row.cpu().numpy(), T1.cpu().numpy(), kw["T0"].cpu().numpy()
        same = 0
        for n in range(3):
            xi = P.solve(row[n])
            ref, taken = P.step(row[n], T0[n], dtype=np.float64)
            assert int(status[n]) == (0 if taken else 1)
            if not taken:
                assert np.array_equal(P.bits(T1[n]), P.bits(T0[n]))
                continue
            bound, kappa = P.update_bound(row[n], xi, ref, T0[n])
            err = np.abs(T1[n].astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (case[0], n, kappa)
            same += int(np.array_equal(P.bits(T1[n]), P.bits(ref.astype(np.float32))))
        print("%dx%d %s: %d of 3 images bit-equal to the rounded fp64 update, at most %.3f of the bound" % (H, W, case[0], same, worst))


def test_degenerate_inputs_keep_T0(gpu_device, V):
    """1x1; fewer than 6 judged pixels; everything masked; a singular system (constant zero depth): status 1 and T = T0 as bits,
    for every iteration of the call; the other images of the batch are fitted as if alone."""
    raw = lambda t: t.view(torch.int32)
    one = args_of(cases(1, 1)[0], gpu_device)
    T, status = V.fit_pose(iters=4, **one)
    assert status.tolist() == [1, 1, 1] and torch.equal(raw(T), raw(one["T0"]))
    case = cases(7, 13)[0]
    kw = args_of(case, gpu_device)
    judged = want_of(case).judged
    five = np.zeros((3, 7, 13), np.uint8)
    for n in (0, 2):
        ys, xs = np.nonzero(judged[n])
        five[n, ys[:5], xs[:5]] = 1
    five[1] = 1
    T, status, row = V.fit_pose(iters=4, normal=True, **{**kw, "valid": dev(five, gpu_device)})
    assert status.tolist() == [1, 0, 1] and row[:, 29].tolist()[0::2] == [5.0, 5.0]
    assert torch.equal(raw(T[0]), raw(kw["T0"][0])) and torch.equal(raw(T[2]), raw(kw["T0"][2]))
    alone = V.fit_pose(iters=4, **{k: (v[1:2] if torch.is_tensor(v) and v.dim() >= 3 and v.shape[0] == 3 else v) for k, v in kw.items()})
    assert torch.equal(raw(T[1]), raw(alone[0][0])) and not torch.equal(raw(T[1]), raw(kw["T0"][1]))
    T, status = V.fit_pose(iters=4, **{**kw, "valid": torch.zeros(3, 7, 13, dtype=torch.uint8, device=gpu_device)})
    assert status.tolist() == [1, 1, 1] and torch.equal(raw(T), raw(kw["T0"]))
    T, status, row = V.fit_pose(iters=4, normal=True, **{**kw, "depth": torch.zeros_like(kw["depth"])})
    assert status.tolist() == [1, 1, 1] and torch.equal(raw(T), raw(kw["T0"])) and not row.any()


def test_singular_and_overflowing_systems_keep_T0(gpu_device, V):
    """The update's other two refusals, with every pixel judged.  (1) K's first column is zero: no pixel's projection depends on a
    translation along x, J[r][0] = 0 exactly, so H[0][0] = 0 and the first pivot is not positive, whatever the damping.  (2) depth
    1e-30 with eps = 0: den ~ 1e-30, A = f / den ~ 2e31 and its square overflows fp32, so sums are +inf (e stays finite: p is a
    quotient of two small numbers).  Both: status 1, T = T0 as bits, the row says why; a healthy image beside them is fitted."""
    raw = lambda t: t.view(torch.int32)
    H, W = 7, 13
    s = P.scene(H, W, N=3, noise=0.3)
    K = np.broadcast_to(s.K, (3, 4, 4)).copy()
    K[0, :, 0] = 0.0
    depth = s.depth.copy()
    depth[2] = 1e-30
    flow = s.flow.copy()
    flow[0] = 0.0
    flow[2] = 0.0
    T0 = P.start(3)
    T0[2] = np.eye(4, dtype=np.float32)
    kw = dict(depth=dev(depth, gpu_device), flow=dev(flow, gpu_device), K=dev(K, gpu_device), inv_K=dev(s.iK, gpu_device),
              T0=dev(T0, gpu_device), huber=INF, eps=0.0)
    T, status, row = V.fit_pose(iters=3, normal=True, **kw)
    row = row.cpu().numpy()
    assert status.tolist() == [1, 0, 1]
    assert torch.equal(raw(T[0]), raw(kw["T0"][0])) and torch.equal(raw(T[2]), raw(kw["T0"][2])) and not torch.equal(raw(T[1]), raw(kw["T0"][1]))
    assert row[0, 29] == H * W and np.isfinite(row[0]).all() and row[0, 0] == 0.0          # every pixel judged, a zero pivot
    assert row[2, 29] == H * W and np.isposinf(row[2, 0])                                  # every pixel judged, a sum overflowed
    want = P.terms(depth, flow, K, s.iK, T0, None, INF, 0.0)
    assert want.judged[0].all() and want.judged[2].all()
    assert P.solve(P.normal(want)[0]) is None and P.solve(P.normal(want)[2]) is None       # the restatement refuses them too


def test_recovery_of_the_reference_geometry(gpu_device, V):
    """The flow of the reference's BackprojectDepth / Project3D (tests/golden/rigidflow.npz) from the identity, 6 plain
    least-squares steps: the kernel's T against the all-fp64 fit (b) within RECOVERY_TOL = 4 x the measured deviation of (a)
    from (b), and so within RECOVERY_B + RECOVERY_TOL of the fixture's T."""
    rec = load_golden("rigidflow.npz")
    worst = 0.0
    for H, W in P.RECOVERY:
        depth, flow, K, iK, T = P.golden_scene(rec, H, W)
        Tb = P.fit(depth, flow, K, iK, iters=P.RECOVERY_ITERS, huber=INF, dtype=np.float64)[0]
        got, status = V.fit_pose(dev(depth, gpu_device), dev(flow, gpu_device), dev(K, gpu_device), dev(iK, gpu_device),
                                 iters=P.RECOVERY_ITERS, huber=INF)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - Tb).max())
        print("%dx%d: kernel - (b) %.2e, kernel - fixture %.2e" % (H, W, err, np.abs(got.cpu().numpy() - T).max()))
        assert int(status[0]) == 0 and err <= P.RECOVERY_TOL
        assert float(np.abs(got.cpu().numpy() - T).max()) <= P.RECOVERY_B + P.RECOVERY_TOL
        worst = max(worst, err)
    print("worst kernel - (b): %.2e of %.2e allowed" % (worst, P.RECOVERY_TOL))


def test_moving_block(gpu_device, V):
    """24x32, a 7x7 block displaced by +5 px, by fit_pose and rigid_flow composed by hand as PoseFlowStream composes them."""
    s, block = P.moving_block()
    d, f, K, iK = (dev(a, gpu_device) for a in (s.depth, s.flow, s.K, s.iK))
    one, status, row = V.fit_pose(d, f, K, iK, iters=4, normal=True)
    at_identity = V.fit_pose(d, f, K, iK, iters=0, normal=True)[2].cpu().numpy()
    kappa = float(np.linalg.cond(P.system(at_identity[0])[0]))
    assert kappa < 1e6 and int(status[0]) == 0
    _, label = V.rigid_flow(d, one, K, iK, flow=f)
    two, status = V.fit_pose(d, f, K, iK, T0=one, valid=(label == 1).view(torch.uint8), iters=4)
    _, label = V.rigid_flow(d, two, K, iK, flow=f)
    e1, e2 = float(np.abs(one.cpu().numpy() - s.T).max()), float(np.abs(two.cpu().numpy() - s.T).max())
    print("kappa %.1f, one round %.2e, two rounds %.2e" % (kappa, e1, e2))
    assert int(status[0]) == 0 and np.array_equal(label.cpu().numpy()[0] == 2, block)
    assert e1 >= 100 * e2 and e2 <= P.RECOVERY_TOL


# ---- layouts, repeats, the raw entry ----------------------------------------------------------------------------------------------------
VIEW_SIZES = [(7, 131), (2, 64), (7, 4), (1, 1)]
IN_PLACE = ("planar", "offset", "batch_slice", "chan_slice", "crop")


def raws(out):
    return [t.view(torch.int32) if t.dtype != torch.float64 else t.view(torch.int64) for t in out]


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(raws(a), raws(b)))


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", VIEW_SIZES, ids=["%dx%d" % s for s in VIEW_SIZES])
def test_views_give_the_bits_of_the_dense_run(gpu_device, V, H, W, N):
    """Every fp32 view of tests/layouts.py of depth [N,1,H,W] and flow [N,2,H,W]: T, status and the sums of the dense run, bit for
    bit (the vector and the scalar form add the same terms in the same order); the kinds whose rows are dense are read in place."""
    kw = args_of(cases(H, W)[2], gpu_device, N)
    base = V.fit_pose(iters=2, normal=True, **kw)
    seen = []
    for kind, v in layouts.views(kw["depth"]):
        kept = V._planes(v[:, 0])[0]
        if kind in IN_PLACE:
            assert kept.data_ptr() == v.data_ptr(), kind
        assert same(V.fit_pose(iters=2, normal=True, **{**kw, "depth": v}), base), kind
        assert same(V.fit_pose(iters=2, normal=True, **{**kw, "depth": v[:, 0]}), base), kind
        seen.append(kind)
    assert set(IN_PLACE) <= set(seen)
    seen = []
    for kind, v in layouts.views(kw["flow"]):
        kept = V._rows(v)[0]
        if kind in IN_PLACE:
            assert kept is v, kind
        assert same(V.fit_pose(iters=2, normal=True, **{**kw, "flow": v}), base), kind
        seen.append(kind)
    assert set(IN_PLACE) <= set(seen)


def test_unpadded_view_of_a_padded_flow_whose_padding_is_nan(gpu_device, V):
    H, W, N = 130, 141, 2
    s = P.scene(H, W, N=N, noise=0.3, outliers=0.1)
    kw = dict(depth=dev(s.depth, gpu_device), K=dev(s.K, gpu_device), inv_K=dev(s.iK, gpu_device), valid=dev(R.mask(H, W, N), gpu_device))
    flow = dev(s.flow, gpu_device)
    padder = V.InputPadder((H, W))
    left, right, top, bottom = padder._pad
    padded = torch.full((N, 2, top + H + bottom, left + W + right), float("nan"), device=gpu_device)
    up = padder.unpad(padded)
    up.copy_(flow)
    assert V._rows(up)[0] is up and not up.is_contiguous()
    a, b = V.fit_pose(flow=up, normal=True, **kw), V.fit_pose(flow=flow, normal=True, **kw)
    assert same(a, b) and a[1].tolist() == [0, 0] and bool(torch.isfinite(a[2]).all()) and bool(torch.isfinite(a[0]).all())


def test_repeats_and_ignores_batch_neighbours(gpu_device, V):
    kw = args_of(cases(7, 64)[2], gpu_device)
    first, second = V.fit_pose(normal=True, **kw), V.fit_pose(normal=True, **kw)
    assert same(first, second)
    other = dict(kw)
    other["depth"], other["flow"], other["T0"] = kw["depth"].clone(), kw["flow"].clone(), kw["T0"].clone()
    other["depth"][0] *= 1.5
    other["flow"][2] += 0.25
    other["T0"][2, 0, 3] += 0.05
    moved = V.fit_pose(normal=True, **other)
    assert all(torch.equal(x[1], y[1]) for x, y in zip(raws(first), raws(moved)))
    assert not torch.equal(raws(first)[0][0], raws(moved)[0][0]) and not torch.equal(raws(first)[0][2], raws(moved)[0][2])
    alone = V.fit_pose(normal=True, **{k: (v[1:2] if torch.is_tensor(v) and v.dim() >= 3 else v) for k, v in kw.items()})
    assert all(torch.equal(x[0], y[1]) for x, y in zip(raws(alone), raws(first)))
    ws = V.pose_fit_workspace(3, 7, 64, gpu_device)
    assert same(V.fit_pose(normal=True, workspace=ws, **kw), first)                 # a workspace of the caller's


def test_raw_entry_in_place_and_without_a_fit(gpu_device, V):
    """T == T0 fits in place; iters = 0 without normal copies T0 and clears status; T0=None is the identity."""
    from deep_visual_slam_amd import _lib as L
    H, W, N = 7, 64, 3
    kw = args_of(cases(H, W)[1], gpu_device)
    want = V.fit_pose(iters=3, **kw)
    K, iK = kw["K"].expand(N, 4, 4).contiguous(), kw["inv_K"].expand(N, 4, 4).contiguous()     # kept alive across the calls
    ws = V.pose_fit_workspace(N, H, W, gpu_device)

    def entry(T0, T, status, iters):
        L.check(L.lib().dvs_pose_fit(kw["depth"].data_ptr(), H * W, W, K.data_ptr(), iK.data_ptr(), T0.data_ptr(), kw["flow"].data_ptr(),
                                     2 * H * W, H * W, W, None, T.data_ptr(), status.data_ptr(), None, ws.data_ptr(), ws.numel(), N, H, W,
                                     iters, kw["huber"], 1e-6, kw["eps"], L.stream()), "dvs_pose_fit")
        torch.cuda.synchronize()

    T = kw["T0"].clone()
    status = torch.full((N,), 7, dtype=torch.int32, device=gpu_device)
    entry(T, T, status, 3)
    assert same((T, status), want)
    T = torch.full((N, 4, 4), 9.0, device=gpu_device)
    status.fill_(7)
    entry(kw["T0"], T, status, 0)
    assert torch.equal(T.view(torch.int32), kw["T0"].view(torch.int32)) and not status.any()
    eye = torch.eye(4, device=gpu_device).repeat(N, 1, 1)
    assert same(V.fit_pose(**{**kw, "T0": None}), V.fit_pose(**{**kw, "T0": eye}))
