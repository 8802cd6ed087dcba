"""dvs_rigid_flow on the GPU (csrc/rigidflow.hip, raft_video.rigid_flow) against the fp32 restatement of tests/rigidflow_ref.py,
EXACTLY: rigid and excess as int32 bit patterns, the labels byte for byte.  Every operation involved (+, -, *, /, the comparisons)
is correctly rounded on both sides and contraction is off in the kernel, so there is no tolerance.

Shapes: the smallest at which a four-pixels-per-lane kernel can go wrong -- W in {1, 3, 4, 5, 63, 64, 65, 131} x H in {1, 2, 7},
N in {1, 3} -- and 131x77 (more than one workgroup).  Inputs: rigidflow_ref.cases (with and without a flow and a mask; depths of 0,
negative, NaN and +inf; a pose that puts part of the image behind the camera; projections exactly on W - 1 / H - 1 and one fp32
step past them; NaN and +-inf flow entries; other alpha, beta, eps, and eps = 0).  Measured on the MI355X: DESIGN.md section 24."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import layouts
import rigidflow_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import raft_video
    return raft_video


@functools.lru_cache(maxsize=None)
def cases(H, W):
    """[(case, the restatement's answer)] at one shape, made once."""
    return [(c, R.run(c)) for c in R.cases(H, W)]


def sub(case, N):
    """The first N images of a case, with K and inv_K as [N,4,4]."""
    name, s, flow, valid, alpha, beta = case
    t = SimpleNamespace(depth=s.depth[:N], T=s.T[:N], K=np.broadcast_to(s.K, (N, 4, 4)).copy(), iK=np.broadcast_to(s.iK, (N, 4, 4)).copy(),
                          eps=s.eps, H=s.H, W=s.W, N=N)
    return name, t, None if flow is None else flow[:N], None if valid is None else valid[:N], alpha, beta


def dev_args(case, dev):
    name, s, flow, valid, alpha, beta = case
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(depth=t(s.depth), T=t(s.T), K=t(s.K), inv_K=t(s.iK), flow=t(flow), valid=t(valid), alpha=alpha, beta=beta, eps=s.eps,
                excess=flow is not None)


def differing(got, want):
    """Elements of rigid (and, with a flow, of label and excess) that differ from the restatement."""
    got = got if isinstance(got, tuple) else (got,)
    rigid = got[0].cpu().numpy()
    assert rigid.dtype == np.float32 and rigid.shape == want.rigid.shape and got[0].is_contiguous()
    bad = int((R.bits(rigid) != R.bits(want.rigid)).sum())
    assert (len(got) == 3) == hasattr(want, "label")
    if len(got) == 3:
        label, excess = got[1].cpu().numpy(), got[2].cpu().numpy()
        assert label.dtype == np.uint8 and excess.dtype == np.float32 and label.shape == want.label.shape == excess.shape
        bad += int((label != want.label).sum()) + int((R.bits(excess) != R.bits(want.excess)).sum())
    return bad


SHAPES = R.SIZES + [R.BIG]


@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_kernel_equals_the_restatement_exactly(gpu_device, V, H, W):
    """Every family at N = 3 with a [4,4] K, and at N = 1 with [N,4,4] matrices and the [N,H,W] depth form."""
    wrong, launches = 0, 0
    for case, want in cases(H, W):
        for N in (3, 1):
            c, w = (case, want) if N == 3 else (sub(case, 1), R.run(sub(case, 1)))
            kw = dev_args(c, gpu_device)
            if N == 1:
                kw["depth"] = kw["depth"][:, 0]
            bad = differing(V.rigid_flow(**kw), w)
            if bad:
                print("%dx%d %s N=%d: %d elements differ" % (H, W, case[0], N, bad))
            wrong += bad
            launches += 1
    print("%dx%d: %d elements differ over %d launches" % (H, W, wrong, launches))
    assert wrong == 0


def test_return_forms(gpu_device, V):
    case, want = cases(7, 65)[2]
    assert case[0] == "flow and valid"
    kw = dev_args(case, gpu_device)
    rigid, label = V.rigid_flow(**{**kw, "excess": False})
    assert tuple(rigid.shape) == (3, 2, 7, 65) and label.dtype == torch.uint8 and tuple(label.shape) == (3, 7, 65)
    assert np.array_equal(label.cpu().numpy(), want.label)
    only = V.rigid_flow(kw["depth"], kw["T"], kw["K"], kw["inv_K"])
    assert torch.is_tensor(only) and np.array_equal(R.bits(only.cpu().numpy()), R.bits(want.rigid))
    # inv_K=None: K inverted on the device; close to the rounded fp64 inverse, not promised bit for bit
    auto = V.rigid_flow(kw["depth"], kw["T"], kw["K"])
    assert tuple(auto.shape) == tuple(only.shape) and float((auto - only).abs().median()) < 1e-3


def test_translating_scene(gpu_device, V):
    """Constant depth and a translation along x: the rigid flow is fx * tx / d = (4, 0) exactly; a measured flow that equals it
    except on an 8x8 square displaced by (+5, 0) is labelled 2 exactly on the square and 1 elsewhere inside."""
    s, flow, want, label = R.translating_scene()
    kw = dev_args(("scene", s, flow, None, R.ALPHA, R.BETA), gpu_device)
    rigid, got, _ = V.rigid_flow(**kw)
    assert np.array_equal(R.bits(rigid.cpu().numpy()), R.bits(want)) and np.array_equal(got.cpu().numpy(), label)
    assert int((label == 2).sum()) == 64 and int((label == 0).sum()) == 4 * 24


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
VIEW_SIZES = [(7, 131), (2, 64), (7, 4), (1, 1)]
IN_PLACE = ("planar", "offset", "batch_slice", "chan_slice", "crop")       # rows stay dense: read through the strides


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", VIEW_SIZES, ids=["%dx%d" % s for s in VIEW_SIZES])
def test_views_are_read_in_place_or_copied_once(gpu_device, V, H, W, N):
    """Every fp32 view of tests/layouts.py of depth [N,1,H,W] and of flow [N,2,H,W] gives the bits of the dense run (what a view
    does not cover holds a sentinel); the kinds whose rows are dense are read in place (the tensor handed to the entry has the
    view's own data_ptr and strides), the others through one dense copy."""
    case = sub(cases(H, W)[2][0], N)
    want = R.run(case)
    kw = dev_args(case, gpu_device)
    seen = []
    for kind, v in layouts.views(kw["depth"]):
        assert torch.equal(v, kw["depth"])
        plane = v[:, 0]
        kept, image, row = V._planes(plane)
        if kind in IN_PLACE:
            assert kept.data_ptr() == plane.data_ptr() and kept.stride() == plane.stride(), kind
        elif kind == "transposed":
            assert kept.data_ptr() != plane.data_ptr() and kept.is_contiguous() and (image, row) == (H * W, W), kind
        assert differing(V.rigid_flow(**{**kw, "depth": v}), want) == 0, kind
        assert differing(V.rigid_flow(**{**kw, "depth": plane}), want) == 0, kind
        seen.append(kind)
    assert set(IN_PLACE) <= set(seen)
    seen = []
    for kind, v in layouts.views(kw["flow"]):
        assert torch.equal(v, kw["flow"])
        kept = V._rows(v)
        if kind in IN_PLACE:
            assert kept[0] is v and kept[0].data_ptr() == v.data_ptr() and kept[0].stride() == v.stride(), kind
        elif kind in ("cl", "transposed", "expanded") and W > 1 and H > 1:
            assert kept[0] is not v and kept[0].is_contiguous() and kept[1:] == (2 * H * W, H * W, W), kind
        assert differing(V.rigid_flow(**{**kw, "flow": v}), want) == 0, kind
        seen.append(kind)
    assert set(IN_PLACE) <= set(seen)


def test_unpadded_view_of_a_padded_flow_is_read_in_place(gpu_device, V):
    """The stream's case: InputPadder.unpad of a padded [N,2,136,144] flow.  No copy (data_ptr and strides are the view's own) and
    the padding, which holds NaN here, is not part of the image."""
    H, W, N = 130, 141, 2
    s = R.scene(H, W, N=N)
    flow, valid = R.measured(s, band=False), R.mask(H, W, N)
    case = ("padded", s, flow, valid, R.ALPHA, R.BETA)
    kw = dev_args(case, gpu_device)
    padder = V.InputPadder((H, W))
    left, right, top, bottom = padder._pad
    padded = torch.full((N, 2, top + H + bottom, left + W + right), float("nan"), device=gpu_device)
    up = padder.unpad(padded)
    up.copy_(kw["flow"])
    kept, image, plane, row = V._rows(up)
    assert kept is up and kept.data_ptr() == up.data_ptr() and kept.stride() == up.stride()
    assert (image, plane, row) == (2 * 136 * 144, 136 * 144, 144)
    assert differing(V.rigid_flow(**{**kw, "flow": up}), R.run(case)) == 0


def test_repeats_and_ignores_batch_neighbours(gpu_device, V):
    case, want = cases(7, 64)[2]
    kw = dev_args(case, gpu_device)
    raw = lambda t: t.view(torch.uint8) if t.dtype == torch.uint8 else t.view(torch.int32)
    first, second = V.rigid_flow(**kw), V.rigid_flow(**kw)
    assert all(torch.equal(raw(x), raw(y)) for x, y in zip(first, second))
    other = dict(kw)
    other["depth"], other["flow"], other["T"] = kw["depth"].clone(), kw["flow"].clone(), kw["T"].clone()
    other["depth"][0] *= 1.5
    other["flow"][2] = 17.0
    other["T"][2, 0, 3] += 0.25
    moved = V.rigid_flow(**other)
    for x, y in zip(first, moved):
        assert torch.equal(raw(x[1]), raw(y[1]))
    assert not torch.equal(raw(first[0][0]), raw(moved[0][0])) and not torch.equal(raw(first[0][2]), raw(moved[0][2]))
    alone = V.rigid_flow(**{**kw, **{k: kw[k][1:2] for k in ("depth", "T", "flow", "valid")}})
    assert all(torch.equal(raw(x[0]), raw(y[1])) for x, y in zip(alone, first))


@pytest.mark.parametrize("H,W", [(7, 64), (7, 5)], ids=["vector", "scalar"])
def test_every_null_output_combination(gpu_device, V, H, W):
    """The entry itself with each of its three outputs present or NULL: what is present is exact, what is NULL is not missed; all
    three NULL launches nothing."""
    from deep_visual_slam_amd import _lib as L
    case, want = cases(H, W)[2]
    c = sub(case, 3)
    kw = dev_args(c, gpu_device)
    N = 3
    answers = (want.rigid, want.excess, want.label)
    shapes = ((N, 2, H, W), (N, H, W), (N, H, W))
    for mask in range(8):
        outs = [torch.full(shapes[i], 7, device=gpu_device, dtype=torch.uint8 if i == 2 else torch.float32) if mask >> i & 1 else None
                for i in range(3)]
        ptrs = [t.data_ptr() if t is not None else None for t in outs]
        L.check(L.lib().dvs_rigid_flow(kw["depth"].data_ptr(), H * W, W, kw["K"].data_ptr(), kw["inv_K"].data_ptr(), kw["T"].data_ptr(),
                                       kw["flow"].data_ptr(), 2 * H * W, H * W, W, kw["valid"].data_ptr(), *ptrs, N, H, W, case[4], case[5],
                                       c[1].eps, L.stream()), "dvs_rigid_flow")
        for t, ans in zip(outs, answers):
            if t is not None:
                got = t.cpu().numpy()
                assert np.array_equal(got, ans) if ans.dtype == np.uint8 else np.array_equal(R.bits(got), R.bits(ans)), mask
    # without a flow: rigid alone
    rigid = torch.full(shapes[0], 7, device=gpu_device, dtype=torch.float32)
    L.check(L.lib().dvs_rigid_flow(kw["depth"].data_ptr(), H * W, W, kw["K"].data_ptr(), kw["inv_K"].data_ptr(), kw["T"].data_ptr(), None, 0, 0,
                                   0, None, rigid.data_ptr(), None, None, N, H, W, case[4], case[5], c[1].eps, L.stream()), "dvs_rigid_flow")
    assert np.array_equal(R.bits(rigid.cpu().numpy()), R.bits(want.rigid))
