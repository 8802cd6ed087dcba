"""_host.dense_view, the one rule by which a wrapper reads a view in place through its strides or makes one dense copy, over the
view zoo of tests/layouts.py.  Pure stride arithmetic: CPU tensors, no device, no library.  The four operand forms of raft_video:
a flow [N,2,H,W] (dvs_flow_consistency, dvs_rigid_flow), a depth [N,H,W] (dvs_rigid_flow), uint8 frames [N,H,W,3] with inner=3
(dvs_frame_ingest) and the flow of dvs_flow_to_image, which takes no image stride."""
import pytest
import torch

import layouts
from deep_visual_slam_amd import raft_video
from deep_visual_slam_amd._host import dense_view

SIZES = [(N, H, W) for N in (1, 3) for H in (1, 2, 5) for W in (1, 2, 7)]
IN_PLACE = ("planar", "offset", "batch_slice", "chan_slice", "size1")


def _flow_image(v):
    """raft_video._strided in dense_view's form: the image stride the entry assumes is two planes."""
    kept, plane, row = raft_video._strided(v)
    return kept, 2 * plane, plane, row


FORMS = {"flow": (lambda N, H, W: (N, 2, H, W), torch.float32, 1, dense_view),
         "depth": (lambda N, H, W: (N, H, W), torch.float32, 1, dense_view),
         "frame": (lambda N, H, W: (N, H, W, 3), torch.uint8, 3, lambda v: dense_view(v, inner=3)),
         "flow_image": (lambda N, H, W: (N, 2, H, W), torch.float32, 1, _flow_image)}


def _source(shape, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randint(0, 200, shape, dtype=torch.uint8, generator=g) if dtype == torch.uint8 else torch.randn(shape, generator=g)


def _read(kept, strides, v, inner):
    """`v`'s elements as a kernel that is handed (kept, strides) addresses them.  What a view does not cover holds the sentinel,
    so a wrong stride is a wrong value."""
    return torch.as_strided(kept, tuple(v.shape), tuple(strides) + ((1,) if inner == 1 else (inner, 1)), kept.storage_offset())


def _is_copy(kept, v):
    return kept is not v and kept.is_contiguous() and kept.storage_offset() == 0 and torch.equal(kept, v)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("N,H,W", SIZES)
def test_every_view_is_read_in_place_or_copied_once(form, N, H, W):
    shape, dtype, inner, view = FORMS[form]
    t = _source(shape(N, H, W), dtype)
    seen = []
    for kind, v in layouts.views(t):
        seen.append(kind)
        kept, *strides = view(v)
        assert len(strides) == v.dim() - (1 if inner == 1 else 2), kind
        assert torch.equal(_read(kept, strides, v, inner), t), (kind, strides, v.stride())
        assert kept is v or _is_copy(kept, v), kind
        apart = form == "flow_image" and kind == "chan_slice" and N > 1           # images four planes apart: no stride says that
        if kind in IN_PLACE and not apart or (kind == "crop" and inner == 1):
            assert kept is v, (kind, v.stride())
        if kind == "transposed" or apart or (kind == "crop" and inner == 3 and W > 1):
            assert _is_copy(kept, v), (kind, v.stride())
    assert {"planar", "offset", "batch_slice", "chan_slice", "crop"} <= set(seen)
    assert ("transposed" in seen) == (t.shape[-1] > 1 and t.shape[-2] > 1) and ("size1" in seen) == (1 in t.shape)


@pytest.mark.parametrize("form", ["flow", "flow_image"])
def test_a_view_that_overlaps_itself_is_copied(form):
    view = FORMS[form][3]
    base = torch.arange(200.0)
    H, W = 3, 4
    for what, strides in (("a zero stride", (0, H * W, W, 1)), ("overlapping rows", (2 * H * W, H * W, 2, 1)),
                          ("overlapping images", (H * W, H * W, W, 1)), ("a zero row stride", (2 * H * W, H * W, 0, 1))):
        v = base.as_strided((2, 2, H, W), strides, 3)
        kept, *got = view(v)
        assert _is_copy(kept, v) and got == [2 * H * W, H * W, W], what
    v = base.as_strided((2, H, W), (H * W - 1, W, 1))                         # a depth whose images share a pixel
    kept, *got = dense_view(v)
    assert _is_copy(kept, v) and got == [H * W, W]
    v = torch.arange(200, dtype=torch.uint8).as_strided((2, H, W, 3), (3 * H * W, 3 * W, 2, 1))       # pixels that share a byte
    kept, *got = dense_view(v, inner=3)
    assert _is_copy(kept, v) and got == [3 * H * W, 3 * W]


@pytest.mark.parametrize("N", [1, 3])
def test_flow_to_image_copies_a_batch_whose_images_are_not_two_planes_apart(N):
    H, W = 5, 7
    t = _source((N, 2, H, W), torch.float32)
    for gap in (1, 3):                                                        # an image stride that no plane stride explains
        buf = torch.full((N * (2 * H * W + gap) + 8,), layouts.SENTINEL[torch.float32])
        v = buf.as_strided((N, 2, H, W), (2 * H * W + gap, H * W, W, 1), 2)
        v.copy_(t)
        kept, *strides = dense_view(v)
        assert kept is v and strides == [2 * H * W + gap if N > 1 else 2 * H * W, H * W, W]       # the entries that take an image stride
        kept, plane, row = raft_video._strided(v)
        assert (plane, row) == (H * W, W) and torch.equal(_read(kept, (2 * plane, plane, row), v, 1), t)
        assert kept is v if N == 1 else _is_copy(kept, v)


def test_the_bindings_of_raft_video_return_the_flat_form():
    v = layouts.make(_source((3, 2, 5, 7), torch.float32), "crop")
    assert raft_video._rows(v)[0] is v and raft_video._rows(v)[1:] == dense_view(v)[1:] == (2 * 7 * 11, 7 * 11, 11)
    d = layouts.make(_source((3, 5, 7), torch.float32), "batch_slice")
    assert raft_video._planes(d)[0] is d and raft_video._planes(d)[1:] == (35, 7)
    f = layouts.make(_source((3, 5, 7, 3), torch.uint8), "chan_slice")
    assert raft_video._packed(f)[0] is f and raft_video._packed(f)[1:] == (7 * 7 * 3, 21)
