"""CPU checks of the layout tests' own ground: the view zoo of tests/layouts.py is what it claims to be (and a stride-blind reader
of every non-dense kind gets other values, so such a wrapper cannot pass the GPU tests), and every argument mismatch of the
ops / layers surface is refused before anything is allocated or launched (tensors that only claim to be on the GPU -- the
stand-in of test_raft_host_cpu.py -- and a library whose every attribute fails the test).  No device, no library."""
import pytest
import torch

import layouts
from test_raft_host_cpu import fake

CL = torch.channels_last


def _source(shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 200, shape, dtype=torch.uint8, generator=g)
    return torch.randn(shape, generator=g)


SHAPES = [(2, 2, 3, 3), (3, 4, 5, 7), (2, 1, 3, 5), (2, 4, 4), (3, 6), (6,), (2, 3, 1, 5)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_view_has_the_sources_values_and_its_own_memory_with_slack(shape, dtype):
    t = _source(shape, dtype)
    seen = []
    for kind, v in layouts.views(t):
        seen.append(kind)
        assert tuple(v.shape) == tuple(t.shape) and v.dtype == t.dtype and torch.equal(v, t), kind
        flat = layouts.storage_flat(v)
        assert flat.data_ptr() != t.data_ptr()
        assert flat.numel() - v.storage_offset() >= v.numel(), kind                  # the slack behind the first element
        covered = torch.zeros(flat.numel(), dtype=torch.bool)
        covered.as_strided(tuple(v.shape), v.stride(), v.storage_offset()).fill_(True)
        rest = flat[~covered]
        assert bool((rest == layouts.SENTINEL[dtype]).all()) and bool(torch.isfinite(rest.float()).all()), kind
        d = layouts.dense(v)
        assert torch.equal(d, t) and d.untyped_storage().data_ptr() != v.untyped_storage().data_ptr()
        assert d.storage_offset() == 0 and d.data_ptr() % 16 == 0
        if kind in layouts.CL_KINDS:
            assert d.is_contiguous(memory_format=CL), kind
        else:
            assert d.is_contiguous(), kind
    want = {"planar", "offset", "batch_slice"}
    if len(shape) == 4:
        want |= {"cl", "offset_cl", "chan_slice_cl"}
    if len(shape) >= 2:
        want |= {"chan_slice", "crop"}
        if shape[-1] > 1 and shape[-2] > 1:
            want.add("transposed")
    if 1 in shape:
        want.add("size1")
    assert set(seen) == want and len(seen) == len(want)


def test_the_kinds_report_what_the_table_says():
    t = _source((2, 2, 3, 3))
    v = dict(layouts.views(t))
    contiguity = lambda x: (x.is_contiguous(), x.is_contiguous(memory_format=CL), x.data_ptr() % 16)
    assert contiguity(v["planar"]) == (True, False, 0)
    assert contiguity(v["cl"]) == (False, True, 0)
    assert contiguity(v["offset"]) == (True, False, 4)                   # dense, one float into its storage
    assert contiguity(v["offset_cl"]) == (False, True, 4)
    assert contiguity(v["batch_slice"]) == (True, False, 8)              # big[1:3] of [4,2,3,3]: 18 floats in
    assert contiguity(v["chan_slice"])[:2] == (False, False)
    assert contiguity(v["chan_slice_cl"])[:2] == (False, False)          # a split of a channels_last tensor is neither
    assert layouts.is_cl(v["chan_slice_cl"]) and not layouts.is_cl(v["chan_slice"])
    assert contiguity(v["crop"])[:2] == (False, False) and v["crop"].stride(-2) == 3 + 4 and v["crop"].stride(-1) == 1
    assert contiguity(v["transposed"])[:2] == (False, False) and v["transposed"].stride()[-2:] == (1, 3)
    # what autograd hands the backward in front of a .sum(): every stride 0, and the zoo's `expanded` is that
    x = torch.randn(2, 2, 3, 3, requires_grad=True)
    g = torch.autograd.grad(x.sum(), x)[0]
    assert g.stride() == (0, 0, 0, 0)
    e = layouts.make(torch.full((2, 2, 3, 3), 0.25), "expanded")
    assert e.stride() == (0, 0, 0, 0) and contiguity(e)[:2] == (False, False) and bool((e == 0.25).all())
    rows = torch.arange(3.0).view(1, 1, 3, 1).expand(2, 2, 3, 3).contiguous()        # constant along N, C and W only
    e = layouts.make(rows, "expanded")
    assert e.stride() == (0, 0, 1, 0) and torch.equal(e, rows)
    assert layouts.make(t, "expanded") is None and layouts.make(t, "size1") is None
    # a size-1 dimension's stride is arbitrary and still reports contiguous
    s = layouts.make(_source((2, 1, 3, 5)), "size1")
    assert s.stride() == (15, layouts.SIZE1_STRIDE, 5, 1) and s.is_contiguous()
    s = layouts.make(_source((1, 2, 3, 1)), "size1")
    assert s.stride() == (layouts.SIZE1_STRIDE, 3, 1, layouts.SIZE1_STRIDE)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_a_stride_blind_reader_gets_other_values_from_every_kind_that_is_not_dense(dtype):
    """numel elements read densely from the view's first element -- what a wrapper that takes data_ptr() of a view it should have
    copied hands its kernel -- differ from the logical values, and come from the view's own allocation."""
    t = _source((3, 4, 5, 7), dtype)
    v = dict(layouts.views(t))
    for kind in ("chan_slice", "chan_slice_cl", "crop", "transposed"):
        assert kind in layouts.NOT_DENSE
        assert not torch.equal(layouts.read_as_dense(v[kind]), t.reshape(-1)), kind
    for kind in layouts.CL_KINDS:                                           # channels_last memory read as planar
        assert not torch.equal(layouts.read_as_dense(v[kind]), t.reshape(-1)), kind
    for kind in ("planar", "offset", "batch_slice"):                        # dense: the same values, whatever the offset
        assert torch.equal(layouts.read_as_dense(v[kind]), t.reshape(-1)), kind
    const = torch.full((3, 4, 5, 7), 3, dtype=dtype)
    e = layouts.make(const, "expanded")
    blind = layouts.read_as_dense(e)
    assert not torch.equal(blind, const.reshape(-1)) and bool((blind[1:] == layouts.SENTINEL[dtype]).all())


def test_relayout_hands_the_producer_a_gradient_of_the_chosen_kind():
    seen = {}

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2.0

        @staticmethod
        def backward(ctx, g):
            seen["g"] = g
            return g * 2.0

    cot = _source((2, 4, 3, 5), seed=1)
    for kind in ("planar", "cl", "offset", "offset_cl", "batch_slice", "chan_slice", "chan_slice_cl", "crop", "transposed"):
        x = _source((2, 4, 3, 5)).requires_grad_(True)
        y = layouts.relayout(Probe.apply(x), kind)
        assert torch.equal(y, x * 2.0)
        (y * cot).sum().backward()
        want = layouts.make(cot, kind)
        assert seen["g"].stride() == want.stride() and seen["g"].storage_offset() == want.storage_offset(), kind
        assert torch.equal(seen["g"], cot) and torch.equal(x.grad, 2.0 * cot)
    x = _source((2, 4, 3, 5)).requires_grad_(True)
    (layouts.relayout(Probe.apply(x), "expanded") * 0.5).sum().backward()
    assert seen["g"].stride() == (0, 0, 0, 0) and torch.equal(x.grad, torch.ones(2, 4, 3, 5))
    x = _source((2, 4, 3, 5)).requires_grad_(True)
    with pytest.raises(ValueError, match="does not apply"):
        (layouts.relayout(Probe.apply(x), "expanded") * cot).sum().backward()


def test_the_matrix_engine_on_a_plain_torch_operator():
    """The engine the GPU files share, run here on the CPU over an operator that handles every layout (torch's own), and over a
    stride-blind one, which it must catch in every kind that is not dense."""
    judge = lambda what, got, want: torch.testing.assert_close(got.double(), want, rtol=1e-6, atol=1e-6)
    inputs = {"x": _source((2, 4, 3, 5)), "k": _source((2, 4, 4), seed=2)}
    fn = lambda x, k: (x * x.flip(3), 2.0 * x[:, :, 1, :], k * k.transpose(1, 2))      # no reduction in either direction: exact
    good = {"mul": layouts.Case(fn, inputs, fn, judge, grads=("x", "k"))}
    cells = layouts.input_cells(good)
    assert ("mul", "x", "chan_slice_cl") in cells and ("mul", "k", "crop") in cells and ("mul", "k", "cl") not in cells
    for c, name, kind in cells:
        good[c].check_input("cpu", name, kind)
    cots = layouts.cotangent_cells(good)
    assert ("mul", "expanded") in cots and ("mul", "offset_cl") in cots and ("mul", "size1") not in cots
    for c, kind in cots:
        good[c].check_cotangent("cpu", kind)
    good["mul"].check_all_at_once("cpu")

    def blind(x, k):
        return fn(layouts.read_as_dense(x).view(x.shape), k)
    bad = layouts.Case(blind, inputs, fn, judge)
    for kind in bad.arg_kinds("x"):
        if kind in layouts.NOT_DENSE or kind in layouts.CL_KINDS:
            with pytest.raises(AssertionError):
                bad.check_input("cpu", "x", kind)
        else:
            bad.check_input("cpu", "x", kind)


# ---- argument refusals happen before any launch ---------------------------------------------------------------------------------
class Reached(Exception):
    """The stubbed library was asked for an entry point: the call got past every check."""


class _NoLibrary:
    def __getattr__(self, name):
        raise Reached(name)


@pytest.fixture
def no_library(monkeypatch):
    from deep_visual_slam_amd import _lib
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    monkeypatch.setattr(_lib, "stream", lambda: pytest.fail("a stream was asked for"))


B, H, W = 2, 17, 23


def _chain_args(**change):
    a = dict(target=fake(B, 3, H, W), src_l=fake(B, 3, H, W), src_r=fake(B, 3, H, W), K=fake(B, 4, 4), inv_K=fake(B, 4, 4),
             T_l=fake(B, 4, 4), T_r=fake(B, 4, 4), disps=[fake(B, 1, H, W), fake(B, 1, 9, 12)])
    a.update(change)
    return a


def _depth_args(**change):
    a = dict(pred_depths=[fake(B, 1, H, W), fake(B, 1, 9, 12)], gt_depth=fake(B, 1, H, W), rgb=fake(B, 3, H, W),
             valid_mask=fake(B, 1, H, W, dtype=torch.uint8))
    a.update(change)
    return a


def _mismatches():
    """(id, call, regex): the message starts with the operator's name and names the offending argument and both shapes."""
    from deep_visual_slam_amd import layers as L
    from deep_visual_slam_amd import ops
    sh = lambda *s: r"\(%s\)" % ", ".join(str(n) for n in s)
    x = sh(B, 3, H, W)
    return [
        ("ssim-broadcast-y", lambda: ops.ssim(fake(B, 3, H, W), fake(1, 3, H, W)), r"^ssim: y .*%s.*%s" % (x, sh(1, 3, H, W))),
        ("ssim-layer", lambda: L.SSIM()(fake(B, 3, H, W), fake(1, 3, H, W)), r"^ssim: y .*%s.*%s" % (x, sh(1, 3, H, W))),
        ("ssim-channels", lambda: ops.ssim(fake(B, 3, H, W), fake(B, 1, H, W)), r"^ssim: y .*%s.*%s" % (x, sh(B, 1, H, W))),
        ("ssim-rank", lambda: ops.ssim(fake(3, H, W), fake(3, H, W)), r"^ssim: x: \[B,C,H,W\].*%s" % sh(3, H, W)),
        ("ssim-one-row", lambda: ops.ssim(fake(B, 3, 1, W), fake(B, 3, 1, W)), r"^ssim: x: .*H, W >= 2.*%s" % sh(B, 3, 1, W)),
        ("backproject-4x4", lambda: ops.backproject(fake(B, 1, H, W), fake(4, 4)),
         r"^backproject: inv_K .*%s.*%s or %s, got %s" % (sh(B, 1, H, W), sh(B, 4, 4), sh(1, 4, 4), sh(4, 4))),
        ("backproject-3x3", lambda: ops.backproject(fake(B, 1, H, W), fake(B, 3, 3)), r"^backproject: inv_K .*%s.*got %s" % (sh(B, 4, 4), sh(B, 3, 3))),
        ("backproject-batch", lambda: ops.backproject(fake(B, 1, H, W), fake(3, 4, 4)), r"^backproject: inv_K .*%s.*got %s" % (sh(B, 4, 4), sh(3, 4, 4))),
        ("backproject-layer", lambda: L.BackprojectDepth(B, H, W)(fake(B, 1, H, W), fake(4, 4)), r"^backproject: inv_K .*got %s" % sh(4, 4)),
        ("backproject-depth", lambda: ops.backproject(fake(B, 3, H, W), fake(B, 4, 4)), r"^backproject: depth: \[B,1,H,W\].*got %s" % x),
        ("project-K-4x4", lambda: ops.project(fake(B, 4, H * W), fake(4, 4), fake(B, 4, 4), H, W),
         r"^project: K .*%s.*%s or %s, got %s" % (sh(B, 4, H * W), sh(B, 4, 4), sh(1, 4, 4), sh(4, 4))),
        ("project-T-3x3", lambda: ops.project(fake(B, 4, H * W), fake(B, 4, 4), fake(B, 3, 3), H, W), r"^project: T .*%s.*got %s" % (sh(B, 4, 4), sh(B, 3, 3))),
        ("project-T-batch", lambda: ops.project(fake(B, 4, H * W), fake(B, 4, 4), fake(3, 4, 4), H, W), r"^project: T .*%s.*got %s" % (sh(B, 4, 4), sh(3, 4, 4))),
        ("project-layer", lambda: L.Project3D(B, H, W)(fake(B, 4, H * W), fake(3, 4, 4), fake(B, 4, 4)), r"^project: K .*got %s" % sh(3, 4, 4)),
        ("project-HW", lambda: ops.project(fake(B, 4, H * W + 1), fake(B, 4, 4), fake(B, 4, 4), H, W),
         r"^project: points: \[B,4,H\*W\] with H=%d, W=%d.*got %s" % (H, W, sh(B, 4, H * W + 1))),
        ("project-rows", lambda: ops.project(fake(B, 3, H * W), fake(B, 4, 4), fake(B, 4, 4), H, W), r"^project: points: .*got %s" % sh(B, 3, H * W)),
        ("smooth-batch", lambda: ops.smooth_loss(fake(B, 1, H, W), fake(1, 3, H, W)), r"^smooth_loss: img: .*%s.*got %s" % (sh(B, 1, H, W), sh(1, 3, H, W))),
        ("smooth-height", lambda: ops.smooth_loss(fake(B, 1, H, W), fake(B, 3, H + 1, W)), r"^smooth_loss: img: .*%s.*got %s" % (sh(B, 1, H, W), sh(B, 3, H + 1, W))),
        ("smooth-width", lambda: L.get_smooth_loss(fake(B, 1, H, W), fake(B, 3, H, W - 1)), r"^smooth_loss: img: .*%s.*got %s" % (sh(B, 1, H, W), sh(B, 3, H, W - 1))),
        ("smooth-disp", lambda: ops.smooth_loss(fake(B, 2, H, W), fake(B, 3, H, W)), r"^smooth_loss: disp: \[B,1,H,W\].*got %s" % sh(B, 2, H, W)),
        ("pose-rows", lambda: ops.pose_to_mat(fake(2, 1, 3), fake(3, 1, 3)), r"^pose_to_mat: translation .*%s.*got %s" % (sh(2, 1, 3), sh(3, 1, 3))),
        ("pose-layer", lambda: L.transformation_from_parameters(fake(2, 1, 3), fake(2, 2, 3)), r"^pose_to_mat: translation .*%s.*got %s" % (sh(2, 1, 3), sh(2, 2, 3))),
        ("pose-not-3", lambda: ops.pose_to_mat(fake(2, 4), fake(2, 4)), r"^pose_to_mat: translation .*%s.*got %s" % (sh(2, 4), sh(2, 4))),
    ] + [
        ("chain-" + name, (lambda kw: lambda: ops.loss_chain(**_chain_args(**kw)))({name: bad}), r"^loss_chain: %s .*%s.*got %s" % (name, want, got))
        for name, bad, want, got in (
            ("src_l", fake(1, 3, H, W), x, sh(1, 3, H, W)), ("src_r", fake(B, 3, H, W + 1), x, sh(B, 3, H, W + 1)),
            ("K", fake(4, 4), sh(B, 4, 4), sh(4, 4)), ("K", fake(1, 4, 4), sh(B, 4, 4), sh(1, 4, 4)),
            ("inv_K", fake(B, 3, 3), sh(B, 4, 4), sh(B, 3, 3)), ("T_l", fake(3, 4, 4), sh(B, 4, 4), sh(3, 4, 4)),
            ("T_r", fake(1, 4, 4), sh(B, 4, 4), sh(1, 4, 4)))
    ] + [
        ("chain-target", lambda: ops.loss_chain(**_chain_args(target=fake(B, 1, H, W))), r"^loss_chain: target: \[B,3,H,W\].*got %s" % sh(B, 1, H, W)),
        ("chain-disp-batch", lambda: ops.loss_chain(**_chain_args(disps=[fake(B, 1, H, W), fake(1, 1, 9, 12)])),
         r"^loss_chain: disps\[1\]: \[B,1,h,w\] for target %s.*got %s" % (x, sh(1, 1, 9, 12))),
        ("chain-disp-channels", lambda: ops.loss_chain(**_chain_args(disps=[fake(B, 2, H, W)])), r"^loss_chain: disps\[0\]: .*%s.*got %s" % (x, sh(B, 2, H, W))),
        ("chain-noise", lambda: ops.loss_chain(noise=fake(1, B, 2, H, W), **_chain_args()), r"^loss_chain: noise .*%s.*got %s" % (sh(2, B, 2, H, W), sh(1, B, 2, H, W))),
        ("depth-gt", lambda: ops.depth_multiscale_losses(**_depth_args(gt_depth=fake(1, 1, H, W))),
         r"^depth_multiscale_losses: gt_depth .*%s.*%s.*got %s" % (x, sh(B, 1, H, W), sh(1, 1, H, W))),
        ("depth-mask", lambda: ops.depth_multiscale_losses(**_depth_args(valid_mask=fake(B, 1, H, W + 1, dtype=torch.uint8))),
         r"^depth_multiscale_losses: valid_mask .*%s.*got %s" % (sh(B, 1, H, W), sh(B, 1, H, W + 1))),
        ("depth-rgb", lambda: ops.depth_multiscale_losses(**_depth_args(rgb=fake(B, 1, H, W))), r"^depth_multiscale_losses: rgb: \[B,3,H,W\].*got %s" % sh(B, 1, H, W)),
        ("depth-pred-batch", lambda: ops.depth_multiscale_losses(**_depth_args(pred_depths=[fake(B, 1, H, W), fake(3, 1, 9, 12)])),
         r"^depth_multiscale_losses: pred_depths\[1\]: \[B,1,h,w\] for rgb %s.*got %s" % (x, sh(3, 1, 9, 12))),
    ]


def _mismatch_ids():
    return [m[0] + "#%d" % i for i, m in enumerate(_mismatches())]


@pytest.mark.parametrize("index", range(len(_mismatch_ids())), ids=_mismatch_ids())
def test_a_mismatched_call_is_refused_before_any_launch(no_library, index):
    from deep_visual_slam_amd._lib import DvsError
    _, call, regex = _mismatches()[index]
    with pytest.raises(DvsError, match=regex):
        call()


def test_matching_calls_and_the_1x4x4_broadcast_get_past_the_checks(no_library):
    """The other half: what the checks let through reaches the (stubbed) library, so a refusal above is the checks' own."""
    from deep_visual_slam_amd import layers as L
    from deep_visual_slam_amd import ops
    calls = [lambda: ops.ssim(fake(B, 3, H, W), fake(B, 3, H, W)),
             lambda: ops.backproject(fake(B, 1, H, W), fake(B, 4, 4)),
             lambda: L.BackprojectDepth(B, H, W)(fake(B, 1, H, W), fake(1, 4, 4)),
             lambda: L.Project3D(B, H, W)(fake(B, 4, H * W), fake(1, 4, 4), fake(B, 4, 4)),
             lambda: ops.project(fake(B, 4, H * W), fake(B, 4, 4), fake(1, 4, 4), H, W),
             lambda: ops.smooth_loss(fake(B, 1, H, W), fake(B, 3, H, W)),
             lambda: ops.pose_to_mat(fake(B, 1, 3), fake(B, 3)),
             lambda: ops.loss_chain(**_chain_args()),
             lambda: ops.depth_multiscale_losses(**_depth_args(gt_depth=fake(B, H, W)))]
    for i, call in enumerate(calls):
        with pytest.raises(Reached):
            call()


def test_aligned_copies_only_what_a_kernel_could_not_read_in_place():
    from deep_visual_slam_amd._host import aligned
    t = _source((3, 4, 3, 5))
    v = dict(layouts.views(t))
    assert aligned(v["planar"]) is v["planar"] and aligned(v["cl"], CL) is v["cl"]
    for kind, fmt in (("offset", torch.contiguous_format), ("offset_cl", CL),
                      ("crop", torch.contiguous_format), ("chan_slice_cl", CL), ("transposed", CL), ("cl", torch.contiguous_format)):
        a = aligned(v[kind], fmt)
        assert a is not v[kind] and torch.equal(a, t) and a.is_contiguous(memory_format=fmt) and a.data_ptr() % 16 == 0, kind
    odd = layouts.make(_source((3, 2, 3, 5)), "batch_slice")                # 30-float images: the slice starts 120 bytes in
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8 and aligned(odd).data_ptr() % 16 == 0


# ---- tensors a call writes are refused, not copied ---------------------------------------------------------------------------------
def _written(kind, *shape, dtype=torch.float32):
    """A stand-in GPU tensor of `kind` that a call would have to write through."""
    src = torch.zeros(*shape, dtype=dtype) if dtype == torch.uint8 else _source(shape)
    return layouts.make(src, kind).as_subclass(type(fake(1)))


def _refused():
    """(id, call, regex): a copy would not carry the result back, so these are the only layouts an operator may refuse."""
    from deep_visual_slam_amd import input_pipeline as P
    from deep_visual_slam_amd import pointcloud as PC
    frames = fake(2, 6, 8, 3, dtype=torch.uint8)
    depth, image, K = fake(2, 1, 6, 10), fake(2, 3, 6, 10), fake(2, 4, 4)
    cells = []
    for kind in ("crop", "chan_slice", "transposed", "cl"):
        cells.append(("color_jitter_-images-" + kind, lambda kind=kind: P.color_jitter_(_written(kind, 2, 3, 6, 8), [[0] * 8] * 2),
                      r"^color_jitter_: contiguous fp32 GPU tensor \[N,3,H,W\] expected"))
    for kind in ("crop", "chan_slice", "transposed", "cl", "offset"):
        cells.append(("u8_to_f32_planar-out-" + kind, lambda kind=kind: P.u8_to_f32_planar(frames, out=_written(kind, 2, 3, 6, 8)),
                      r"^u8_to_f32_planar: out is written in place and must be a contiguous, 16-byte aligned .*\[2,3,6,8\], got"))
    for kind in ("crop", "chan_slice", "transposed"):
        cells.append(("depth_to_cloud-out-" + kind, lambda kind=kind: PC.depth_to_cloud(depth, image, K, out=_written(kind, 2, 60, 4)),
                      r"^depth_to_cloud: out is written in place and must be contiguous, got \(2, 60, 4\)"))
    cells.append(("depth_to_cloud-index-transposed",
                  lambda: PC.depth_to_cloud(depth, image, K, index=torch.zeros(60, 2, dtype=torch.int32).t().as_subclass(type(fake(1)))),
                  r"^depth_to_cloud: index is written in place and must be contiguous, got \(2, 60\)"))
    cells.append(("depth_to_cloud-workspace-strided",
                  lambda: PC.depth_to_cloud(depth, image, K, z_range=(0.1, 5.0), workspace=torch.zeros(64, 2, dtype=torch.uint8)[:, 0].as_subclass(type(fake(1)))),
                  r"^depth_to_cloud: workspace is written in place and must be contiguous, got \(64,\)"))
    cells.append(("depth_to_cloud-count-strided",
                  lambda: PC.depth_to_cloud(depth, image, K, count=torch.zeros(2, 2, dtype=torch.int32)[:, 0].as_subclass(type(fake(1)))),
                  r"^depth_to_cloud: count is written in place and must be contiguous, got \(2,\)"))
    # PoseChain.step's outputs and the pose it advances
    chain = PC.PoseChain.__new__(PC.PoseChain)
    chain.left, chain.world = None, fake(4, 4)
    T = fake(3, 4, 4)
    for name, bad in (("poses", _written("crop", 3, 4, 4)), ("M", _written("transposed", 3, 4, 4)), ("tq", _written("chan_slice", 3, 7)),
                      ("world", _written("crop", 4, 4))):
        cells.append(("PoseChain.step-" + name, lambda name=name, bad=bad: chain.step(T, **{**dict(poses=fake(3, 4, 4), M=fake(3, 4, 4), tq=fake(3, 7), world=fake(4, 4)), name: bad}),
                      r"^PoseChain.step: %s is written in place and must be a contiguous fp32 GPU tensor \[.*\], got" % name))
    # the FusedAdam arena: dp.FlatParams always makes a dense one; an arena from elsewhere must be that too
    from types import SimpleNamespace
    from deep_visual_slam_amd import dp
    for name, bad in (("params", _written("crop", 8, 8)[:, 0]), ("grads", _written("offset", 64))):     # strided; misaligned
        arena = SimpleNamespace(params=fake(64), grads=fake(64), tensors=[])
        setattr(arena, name, bad)
        cells.append(("FusedAdam-arena-" + name, lambda arena=arena: dp.FusedAdam(arena),
                      r"^FusedAdam: the arena's %s are written in place and must be one contiguous, 16-byte aligned" % name))
    # the DA-V2 inference helpers that refuse: model-internal, handed only what the model made
    from deep_visual_slam_amd import depth_anything_v2 as D
    for kind in ("offset", "crop", "transposed", "batch_slice", "chan_slice"):
        cells.append(("layernorm-x2d-" + kind, lambda kind=kind: D.layernorm(_written(kind, 7, 62), fake(62), fake(62), 1e-6),
                      r"^layernorm: x2d must be contiguous and 16-byte aligned"))
        cells.append(("attention-qkv2d-" + kind, lambda kind=kind: D.attention(_written(kind, 6, 382), 2, 3, 2, 64),
                      r"^attention: qkv2d must be contiguous and 16-byte aligned"))
    for name in ("weight", "bias"):
        cells.append(("layernorm-%s-offset" % name, lambda name=name: D.layernorm(fake(7, 64), **{"weight": fake(64), "bias": fake(64),
                                                                                               name: _written("offset", 64)}, eps=1e-6),
                      r"^layernorm: %s must be contiguous and 16-byte aligned" % name))
    return cells


REFUSED = [c[0] for c in _refused()]


@pytest.mark.parametrize("index", range(len(REFUSED)), ids=REFUSED)
def test_a_written_tensor_that_is_not_dense_is_refused_before_any_launch(no_library, index):
    from deep_visual_slam_amd._lib import DvsError
    _, call, regex = _refused()[index]
    with pytest.raises(DvsError, match=regex):
        call()
