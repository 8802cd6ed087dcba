"""dvs_flow_consistency on the GPU (csrc/flowcons.hip, raft_video.flow_consistency) against the fp32 restatement of
tests/flowcons_ref.py, EXACTLY: excess as int32 bit patterns, the masks byte for byte.  Every operation involved (+, -, *, floor,
the comparisons) is correctly rounded on both sides and contraction is off in the kernel, so there is no tolerance.

Shapes: the smallest at which a four-pixels-per-lane kernel can go wrong -- W in {1, 3, 4, 5, 63, 64, 65, 131} x H in {1, 2, 7},
N in {1, 3} -- and 131x77 (more than one workgroup).  Inputs: flowcons_ref.cases (noise from everything-valid to mostly-outside,
the smooth field and its negative, zero flow, flows that land exactly on and just past W - 1 / H - 1, NaN and +-inf entries).
Measured on the MI355X: see DESIGN.md section 23."""
import functools

import numpy as np
import pytest
import torch

import flowcons_ref as R
import layouts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import raft_video
    return raft_video


@functools.lru_cache(maxsize=None)
def cases(H, W):
    """[(name, a, b, (direction a, direction b))] at one shape: inputs and the restatement's answer, made once."""
    return [(name, a, b, R.consistency(a, b)) for name, a, b in R.cases(H, W)]


def differing(got, want):
    """Elements of (valid_fw, valid_bw, excess_fw, excess_bw) that differ from the restatement's two directions."""
    valid_a, valid_b, excess_a, excess_b = (t.cpu().numpy() for t in got)
    bad = 0
    for valid, excess, r in ((valid_a, excess_a, want[0]), (valid_b, excess_b, want[1])):
        assert valid.dtype == np.uint8 and excess.dtype == np.float32 and valid.shape == r.valid.shape == excess.shape
        bad += int((valid != r.valid).sum()) + int((R.bits(excess) != R.bits(r.excess)).sum())
    return bad


def run(V, a, b, dev, **kw):
    return V.flow_consistency(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), excess=True, **kw)


SHAPES = R.SIZES + [R.BIG]


@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_kernel_equals_the_restatement_exactly(gpu_device, V, H, W):
    wrong, launches = 0, 0
    for name, a, b, want in cases(H, W):
        for N in sorted({1, a.shape[0]}):
            sub = tuple(R.direction(x[:N], y[:N]) for x, y in ((a, b), (b, a))) if N < a.shape[0] else want
            got = run(V, a[:N], b[:N], gpu_device)
            bad = differing(got, sub)
            if bad:
                print("%dx%d %s N=%d: %d elements differ" % (H, W, name, N, bad))
            wrong += bad
            launches += 1
            assert got[0].is_contiguous() and got[2].is_contiguous() and tuple(got[1].shape) == (N, H, W)
    print("%dx%d: %d elements differ over %d launches" % (H, W, wrong, launches))
    assert wrong == 0


def test_thresholds_and_the_single_image_form(gpu_device, V):
    name, a, b, _ = cases(7, 65)[1]
    assert name == "noise0.7"
    for alpha, beta in ((0.0, 0.0), (0.05, 0.25), (1.0, 4.0)):
        assert differing(run(V, a, b, gpu_device, alpha=alpha, beta=beta), R.consistency(a, b, alpha, beta)) == 0
    strict, loose = R.consistency(a, b, 0.0, 0.0)[0].valid, R.consistency(a, b, 1.0, 4.0)[0].valid
    assert strict.sum() < loose.sum()                                       # the thresholds were used
    one = V.flow_consistency(torch.from_numpy(a[1]).to(gpu_device), torch.from_numpy(b[1]).to(gpu_device))
    assert len(one) == 2 and tuple(one[0].shape) == (7, 65) and one[0].dtype == torch.uint8
    want = R.consistency(a[1:2], b[1:2])
    assert np.array_equal(one[0].cpu().numpy(), want[0].valid[0]) and np.array_equal(one[1].cpu().numpy(), want[1].valid[0])


def test_occluder_scene(gpu_device, V):
    """A static background and an 8x8 square displaced by (+5, 0): the forward mask is 0 exactly on the 5x8 pixels the square newly
    covers, the backward mask exactly on the 5x8 pixels it uncovers."""
    a, b, want, want_bw = R.occluder()
    valid, valid_bw = V.flow_consistency(torch.from_numpy(a).to(gpu_device), torch.from_numpy(b).to(gpu_device))
    assert np.array_equal(valid.cpu().numpy(), want) and np.array_equal(valid_bw.cpu().numpy(), want_bw)
    assert int((1 - want).sum()) == 40 and int((1 - want_bw).sum()) == 40


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
VIEW_SIZES = [(7, 131), (2, 64), (7, 4), (1, 1)]
IN_PLACE = ("planar", "offset", "batch_slice", "chan_slice", "crop")       # rows stay dense: read through the strides


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", VIEW_SIZES, ids=["%dx%d" % s for s in VIEW_SIZES])
def test_views_are_read_in_place_or_copied_once(gpu_device, V, H, W, N):
    """Every fp32 view of tests/layouts.py of either flow gives the bits of the dense run (what a view does not cover holds a
    sentinel); the kinds whose rows are dense are read in place."""
    a, b = (t[:N] for t in R.noise(H, W, 0.7))
    want = R.consistency(a, b)
    da, db = torch.from_numpy(a).to(gpu_device), torch.from_numpy(b).to(gpu_device)
    seen = []
    for (kind, va), (kind_b, vb) in zip(layouts.views(da), layouts.views(db)):
        assert kind == kind_b and torch.equal(va, da) and torch.equal(vb, db)
        kept = V._rows(va)
        if kind in IN_PLACE:
            assert kept[0] is va, kind
        elif kind in ("cl", "transposed", "expanded") and W > 1 and H > 1:
            assert kept[0] is not va and kept[0].is_contiguous() and kept[1:] == (2 * H * W, H * W, W), kind
        for x, y in ((va, vb), (va, db), (da, vb)):
            assert differing(V.flow_consistency(x, y, excess=True), want) == 0, kind
        seen.append(kind)
    assert set(IN_PLACE) <= set(seen)


def test_unpadded_view_of_a_padded_flow_is_read_in_place(gpu_device, V):
    """FlowStream's case: InputPadder.unpad of a padded [2N,2,Hp,Wp] flow, split into its two halves.  No copy (data_ptr and
    strides are the view's own) and the padding, which holds NaN here, is not part of the image."""
    H, W, N = 130, 141, 2
    a, b = (t[:N] for t in R.noise(H, W, 3.0))
    padder = V.InputPadder((H, W))
    left, right, top, bottom = padder._pad
    padded = torch.full((2 * N, 2, top + H + bottom, left + W + right), float("nan"), device=gpu_device)
    up = padder.unpad(padded)
    up[:N], up[N:] = torch.from_numpy(a).to(gpu_device), torch.from_numpy(b).to(gpu_device)
    fw, bw = up[:N], up[N:]
    for v in (fw, bw):
        kept, image, plane, row = V._rows(v)
        assert kept is v and kept.data_ptr() == v.data_ptr() and kept.stride() == v.stride()
        assert (image, plane, row) == (2 * 136 * 144, 136 * 144, 144)
    assert differing(V.flow_consistency(fw, bw, excess=True), R.consistency(a, b)) == 0


def test_repeats_and_ignores_batch_neighbours(gpu_device, V):
    name, a, b, want = cases(7, 64)[1]
    first, second = run(V, a, b, gpu_device), run(V, a, b, gpu_device)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(first, second))
    other_a, other_b = a.copy(), b.copy()
    other_a[0], other_b[2] = -other_a[0], 17.0
    moved = run(V, other_a, other_b, gpu_device)
    for x, y in zip(first, moved):
        assert torch.equal(x[1].view(torch.uint8), y[1].view(torch.uint8))
    assert not torch.equal(first[2][0].view(torch.uint8), moved[2][0].view(torch.uint8))
    alone = run(V, a[1:2], b[1:2], gpu_device)
    assert all(torch.equal(x[0].view(torch.uint8), y[1].view(torch.uint8)) for x, y in zip(alone, first))


@pytest.mark.parametrize("H,W", [(7, 64), (7, 5)], ids=["vector", "scalar"])
def test_every_null_output_combination(gpu_device, V, H, W):
    """The entry itself with each of its four outputs present or NULL: what is present is exact, what is NULL is not missed; all
    four NULL launches nothing."""
    from deep_visual_slam_amd import _lib as L
    name, a, b, want = cases(H, W)[1]
    N = a.shape[0]
    da, db = torch.from_numpy(a).to(gpu_device), torch.from_numpy(b).to(gpu_device)
    answers = (want[0].valid, want[1].valid, want[0].excess, want[1].excess)
    for mask in range(16):
        outs = [torch.full((N, H, W), 7, device=gpu_device, dtype=torch.uint8 if i < 2 else torch.float32) if mask >> i & 1 else None
                for i in range(4)]
        ptrs = [t.data_ptr() if t is not None else None for t in outs]
        L.check(L.lib().dvs_flow_consistency(da.data_ptr(), 2 * H * W, H * W, W, db.data_ptr(), 2 * H * W, H * W, W, *ptrs, N, H, W,
                                             R.ALPHA, R.BETA, L.stream()), "dvs_flow_consistency")
        for t, ans in zip(outs, answers):
            if t is not None:
                got = t.cpu().numpy()
                assert np.array_equal(got, ans) if ans.dtype == np.uint8 else np.array_equal(R.bits(got), R.bits(ans)), mask
