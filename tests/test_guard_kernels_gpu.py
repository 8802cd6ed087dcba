"""Guard-band cases per kernel family: does each kernel stay inside its buffers at ragged shapes?

Every case: inputs are built on the CPU and placed between POISON (quiet NaN) bands -- operands a kernel adds into
(gradient sinks, Adam's arrays) between CANARY bands -- the call runs inside guard.allocations(), so its outputs,
workspaces and weight packs are guarded too; after a synchronise every band must be untouched, the outputs finite, and
the values equal the fp64 torch reference at the tolerance the family's own value test uses.  Shapes sit on both sides of
each kernel's tile.  See tests/guard.py."""
import pytest
import torch
import torch.nn.functional as F

import guard

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def relmax(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    assert torch.isfinite(a).all(), "non-finite output: a guard value reached the arithmetic"
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cl(g, t, pattern=guard.POISON, grad=False):
    """A 4-D tensor placed in NHWC memory -- the layout the wrappers take without a copy -- between bands."""
    from deep_visual_slam_amd import conv as DC
    p = g.place(t.contiguous(memory_format=CL), pattern)
    assert DC._nhwc(p).data_ptr() == p.data_ptr()          # the kernel is handed the guarded pointer, not a fresh copy
    return p.requires_grad_(True) if grad else p


def _mods(*extra):
    from deep_visual_slam_amd import conv as DC, zeropool
    return (DC, zeropool) + extra


def _ref_conv(x, w, b, s, p, refl, act, xa=None):
    """fp64 reference: [upsample2x(xa) (+ concat x)] -> [reflect pad] -> conv -> act."""
    if xa is not None:
        up = F.interpolate(xa, scale_factor=2, mode="nearest")
        x = up if x is None else torch.cat([up, x], 1)
    xx = F.pad(x, (p,) * 4, mode="reflect") if refl else x
    y = F.conv2d(xx, w, b, s, 0 if refl else p)
    return {None: lambda v: v, "elu": F.elu, "relu": F.relu, "sigmoid": torch.sigmoid}[act](y)


def _autograd_case(dev, fn, B, ci, co, k, s, p, refl, H, W, act, has_b, c1=0, up=False, tol=(2e-5, 1e-4), seed=0, allocs=4, spec=None):
    """fn(x, w, b, xa) -> y on the GPU (an autograd wrapper); forward and all gradients against fp64.  c1 > 0: the decoder's
    upsample(+concat) gather -- xa [B,c1,H/2,W/2] is the coarse operand, x the skip tensor with ci - c1 channels (None when
    c1 == ci).  spec (bf16 mode): the operand rounding the forward is specified with; the forward is then compared with fp64 on
    the rounded operands, the gradients with fp64 on the unrounded ones."""
    gen = _gen(seed)
    xa = torch.randn(B, c1, H // 2, W // 2, generator=gen) if c1 else None
    x = torch.randn(B, ci - c1, H, W, generator=gen) if ci > c1 else None
    w = torch.randn(co, ci, k, k, generator=gen) * (2.0 / (ci * k * k)) ** 0.5
    b = torch.randn(co, generator=gen) * 0.1 if has_b else None
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in (x, xa, w, b)]
    y64 = _ref_conv(leaves[0], leaves[2], leaves[3], s, p, refl, act, leaves[1])
    cot = torch.randn(y64.shape, generator=gen)
    g64 = torch.autograd.grad(y64, [t for t in leaves if t is not None], cot.double())
    g = guard.Bands(dev)
    gx = _cl(g, x, grad=True) if x is not None else None
    gxa = _cl(g, xa, grad=True) if xa is not None else None
    gw = _cl(g, w, grad=True)
    gb = g.place(b).requires_grad_(True) if has_b else None
    gcot = _cl(g, cot)
    with guard.allocations(*_mods()) as rec:
        y = fn(gx, gw, gb, gxa)
        grads = torch.autograd.grad(y, [t for t in (gx, gxa, gw, gb) if t is not None], gcot)
        torch.cuda.synchronize()
    assert rec.count >= allocs, rec.count
    g.check()
    if spec is not None:
        rx, rxa, rw = (spec(t) if t is not None else None for t in (x, xa, w))
        y64 = _ref_conv(rx, rw, b.double() if has_b else None, s, p, refl, act, rxa)
    assert relmax(y, y64) < tol[0], relmax(y, y64)
    names = [n for n, t in zip(("dx", "dxa", "dw", "db"), (x, xa, w, b)) if t is not None]
    for nm, a, r in zip(names, grads, g64):
        assert relmax(a, r) < tol[1], (nm, relmax(a, r))


# ---- implicit GEMM forward / data gradient / weight gradient, split-K (conv_fwd.hip, conv_dma.h, conv_wgrad.hip) --------------
IGEMM = [
    # name, B, Cin, Cout, k, stride, pad, reflect, H, W, act, bias
    ("odd_tail_b1", 1, 20, 36, 3, 1, 1, False, 11, 17, None, True),
    ("odd_tail_b3", 3, 20, 36, 3, 1, 1, False, 11, 17, "relu", True),
    ("3x3_s2_odd", 3, 64, 128, 3, 2, 1, False, 15, 21, None, False),
    ("1x1_s2_odd", 1, 64, 128, 1, 2, 0, False, 15, 21, None, False),
    ("1x1_s2_odd_b3", 3, 64, 128, 1, 2, 0, False, 15, 21, "relu", True),
    ("split_k", 1, 256, 512, 3, 1, 1, False, 8, 12, None, False),
    ("split_k_s2_b3", 3, 256, 512, 3, 2, 1, False, 8, 12, None, False),
    ("reflect_3x5", 1, 64, 64, 3, 1, 1, True, 3, 5, "elu", True),
    ("reflect_3x5_b3", 3, 128, 64, 3, 1, 1, True, 3, 5, "elu", True),
    ("prime_13x31", 1, 36, 20, 3, 1, 1, False, 13, 31, None, True),
]


@pytest.fixture
def no_winograd():
    """The implicit-GEMM kernels themselves: Winograd dispatch off for the case."""
    from deep_visual_slam_amd import conv as DC
    old, DC._WINO = DC._WINO, False
    yield
    DC._WINO = old


@pytest.mark.parametrize("case", IGEMM, ids=[c[0] for c in IGEMM])
def test_igemm_conv(gpu_device, no_winograd, case):
    from deep_visual_slam_amd import conv as DC
    _, B, ci, co, k, s, p, refl, H, W, act, has_b = case
    w_probe = torch.empty(co, ci, k, k)
    assert DC.supported(torch.empty(B, ci, H, W), w_probe) and not DC.wino_eligible(w_probe, s, p, refl, act, None, False, None)
    assert not DC.head_supported(torch.empty(B, ci, H, W), w_probe, s, p if not refl else 0, p if refl else 0)
    _autograd_case(gpu_device, lambda x, w, b, xa: DC.conv2d(x, w, b, s, 0 if refl else p, p if refl else 0, act),
                   B, ci, co, k, s, p, refl, H, W, act, has_b)


@pytest.mark.parametrize("B,ci,co,k,s,p,H,W", [(1, 20, 36, 3, 1, 1, 11, 17), (3, 64, 128, 3, 2, 1, 15, 21), (1, 256, 512, 3, 1, 1, 8, 12),
                                               (3, 64, 128, 1, 2, 0, 15, 21)])
@pytest.mark.parametrize("ordered", [False, True], ids=["atomics", "ordered_ws"])
def test_igemm_wgrad_into_guarded_sinks(gpu_device, no_winograd, B, ci, co, k, s, p, H, W, ordered):
    """conv2d_wgrad adding into dw_out / db_out sinks that sit between canaries, as the gradient arena packs them; the ordered
    form additionally gets a workspace of exactly the size the library asks for (allocated inside the guarded context)."""
    from deep_visual_slam_amd import conv as DC
    gen = _gen(1)
    x = torch.randn(B, ci, H, W, generator=gen)
    Ho, Wo = DC.out_hw(H, W, k, k, s, p)
    dy = torch.randn(B, co, Ho, Wo, generator=gen)
    w64 = torch.zeros(co, ci, k, k, dtype=torch.float64, requires_grad=True)
    b64 = torch.zeros(co, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, b64, s, p).backward(dy.double())
    g = guard.Bands(gpu_device)
    gx, gdy = _cl(g, x), _cl(g, dy)
    sink = _cl(g, torch.full((co, ci, k, k), 0.5), guard.CANARY)
    bsink = g.place(torch.full((co,), 0.25), guard.CANARY)
    old, DC._WGRAD_ORDERED = DC._WGRAD_ORDERED, ordered
    try:
        with guard.allocations(*_mods()) as rec:
            got = DC.conv2d_wgrad(gx, gdy, (co, ci, k, k), s, p, False, True, dw_out=sink, db_out=bsink)
            dw, db = DC.conv2d_wgrad(gx, gdy, (co, ci, k, k), s, p, False, True)
            torch.cuda.synchronize()
    finally:
        DC._WGRAD_ORDERED = old
    assert got == (None, None) and rec.count >= (3 if ordered else 2), rec.count
    g.check()
    assert relmax(sink - 0.5, w64.grad) < 1e-4 and relmax(bsink - 0.25, b64.grad) < 1e-4
    assert relmax(dw, w64.grad) < 1e-4 and relmax(db, b64.grad) < 1e-4


# ---- Winograd forward / data gradient / weight gradient / decoder gather (conv_wino.hip) ---------------------------------
WINO_TOL = 3e-6          # tests/test_wino_gpu.py
WINO = [(1, 64, 64, 13, 27), (3, 64, 128, 5, 7), (1, 64, 64, 2, 2), (3, 128, 64, 2, 2), (1, 512, 512, 15, 20), (3, 80, 96, 5, 7),
        (1, 96, 80, 13, 27), (3, 64, 64, 1, 1), (1, 64, 192, 7, 1)]


@pytest.mark.parametrize("B,ci,co,h,w", WINO)
def test_wino_forward_stats_dgrad(gpu_device, B, ci, co, h, w):
    from deep_visual_slam_amd import conv as DC
    gen = _gen(2)
    x = torch.randn(B, ci, h, w, generator=gen)
    wt = torch.randn(co, ci, 3, 3, generator=gen) * (2.0 / (ci * 9)) ** 0.5
    dy = torch.randn(B, co, h, w, generator=gen)
    y64 = F.conv2d(x.double(), wt.double(), None, 1, 1)
    dx64 = F.conv_transpose2d(dy.double(), wt.double(), None, 1, 1)
    g = guard.Bands(gpu_device)
    gx, gw, gdy = _cl(g, x), _cl(g, wt), _cl(g, dy)
    assert DC.wino_eligible(gw, 1, 1, False, None, None, False, None)
    st = g.zeros((2, co), pattern=guard.CANARY)                      # statistics are atomically added
    slots = g.zeros((DC.STAT_SLOTS, 1, 2, co), pattern=guard.CANARY)
    with guard.allocations(*_mods()) as rec:
        y = DC.conv3x3_wino(gx, gw, st, 1)
        y2 = DC.conv3x3_wino(gx, gw, slots, 1, stat_slots=DC.STAT_SLOTS)
        dx = DC.conv3x3_wino(gdy, gw, flip=True)
        torch.cuda.synchronize()
    assert rec.count >= 5, rec.count                                  # 3 outputs + the two weight operands
    g.check()
    assert relmax(y, y64) < WINO_TOL and relmax(y2, y64) < WINO_TOL and relmax(dx, dx64) < WINO_TOL
    ref = torch.stack([y64.sum((0, 2, 3)), (y64 * y64).sum((0, 2, 3))])
    assert relmax(st, ref) < 2e-5 and relmax(slots.sum(0)[0], ref) < 2e-5


@pytest.mark.parametrize("B,ci,co,h,w", [(1, 64, 64, 13, 27), (3, 64, 128, 5, 7), (1, 64, 64, 2, 2), (1, 512, 512, 15, 20), (3, 96, 96, 5, 7),
                                         (3, 64, 64, 1, 1)])
@pytest.mark.parametrize("ordered", [False, True], ids=["atomics", "ordered_ws"])
def test_wino_wgrad_into_guarded_sink(gpu_device, B, ci, co, h, w, ordered):
    from deep_visual_slam_amd import conv as DC
    gen = _gen(3)
    x, dy = torch.randn(B, ci, h, w, generator=gen), torch.randn(B, co, h, w, generator=gen)
    w64 = torch.zeros(co, ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, None, 1, 1).backward(dy.double())
    assert DC.wino_wgrad_eligible((co, ci, 3, 3))
    g = guard.Bands(gpu_device)
    gx, gdy = _cl(g, x), _cl(g, dy)
    sink = _cl(g, torch.full((co, ci, 3, 3), 0.5), guard.CANARY)
    old, DC._WGRAD_ORDERED = DC._WGRAD_ORDERED, ordered
    try:
        with guard.allocations(*_mods()) as rec:
            assert DC.conv3x3_wino_wgrad(gx, gdy, (co, ci, 3, 3), dw_out=sink) is None
            dw = DC.conv3x3_wino_wgrad(gx, gdy, (co, ci, 3, 3))
            torch.cuda.synchronize()
    finally:
        DC._WGRAD_ORDERED = old
    assert rec.count >= (3 if ordered else 1), rec.count
    g.check()
    ref = w64.grad
    assert relmax(dw, ref) < WINO_TOL
    assert relmax(sink - 0.5, ref) < WINO_TOL + 1e-6 / float(ref.abs().max())


WINO_DEC = [
    # B, c1 (coarse / only source), c2 (skip), co, H, W, upsample
    (1, 64, 0, 64, 13, 27, False), (3, 80, 0, 64, 5, 7, False), (1, 64, 0, 64, 2, 2, False),
    (1, 64, 0, 64, 2, 2, True),                                                  # a 1x1 source, upsample only
    (3, 64, 64, 96, 6, 10, True), (1, 96, 32, 64, 2, 2, True),
]


@pytest.mark.parametrize("B,c1,c2,co,H,W,up", WINO_DEC)
def test_wino_decoder_gather(gpu_device, B, c1, c2, co, H, W, up):
    """ReflectionPad2d(1) + [nearest 2x upsample (+ concat)] + 3x3 + ELU on the Winograd gather, its padded-domain data
    gradient with the reflection fold, and the weight gradient of the gathers."""
    from deep_visual_slam_amd import conv as DC
    ci = c1 + c2
    xs = torch.empty(B, c1, H // 2 if up else H, W // 2 if up else W)
    x2 = torch.empty(B, c2, H, W) if c2 else (DC.UPSAMPLE_ONLY if up else None)
    assert DC.wino_dec_eligible(torch.empty(co, ci, 3, 3), 1, 1, True, "elu", xs, x2, False, None)
    old, DC._WINO_FORCE = DC._WINO_FORCE, True          # the cost model would send these small shapes elsewhere
    try:
        _autograd_case(gpu_device, lambda x, w, b, xa: DC.conv2d(xa if up else x, w, b, 1, 0, 1, "elu", x2=x if (up and c2) else None,
                                                                 upsample=up),
                       B, ci, co, 3, 1, 1, True, H, W, "elu", True, c1=c1 if up else 0, tol=(2e-5, 2e-5))
    finally:
        DC._WINO_FORCE = old


@pytest.mark.parametrize("B,c1,c2,co,H,W", [(3, 56, 72, 64, 4, 4), (1, 72, 56, 96, 10, 14), (1, 56, 72, 64, 6, 6)])
def test_wino_decoder_gather_uneven_channel_split(gpu_device, B, c1, c2, co, H, W):
    """Upsample + concat where the two sources split the channels at 56 / 72 -- multiples of 8 that are not multiples of 16, so a
    16-channel K chunk straddles the two tensors: the forward gather and the padded-domain data gradient with its reflection
    fold and 2x2 sum, through the family's own wrappers (the weight gradient of such a split runs elsewhere)."""
    from deep_visual_slam_amd import conv as DC
    ci = c1 + c2
    gen = _gen(c1)
    xa, skip = torch.randn(B, c1, H // 2, W // 2, generator=gen), torch.randn(B, c2, H, W, generator=gen)
    w = torch.randn(co, ci, 3, 3, generator=gen) * (2.0 / (ci * 9)) ** 0.5
    b = torch.randn(co, generator=gen) * 0.1
    dz = torch.randn(B, co, H, W, generator=gen)
    assert DC.wino_dec_eligible(w, 1, 1, True, "elu", xa, skip, False, None)
    xa64, sk64 = xa.double().requires_grad_(True), skip.double().requires_grad_(True)
    pre64 = _ref_conv(sk64, w.double(), b.double(), 1, 1, True, None, xa64)
    dxa64, dsk64 = torch.autograd.grad(pre64, [xa64, sk64], dz.double())
    g = guard.Bands(gpu_device)
    gxa, gsk, gw, gdz = _cl(g, xa), _cl(g, skip), _cl(g, w), _cl(g, dz)
    gb = g.place(b)
    with guard.allocations(*_mods()) as rec:
        y = DC.conv3x3_wino_gen(gxa, gsk, gw, gb, "elu", reflect=True)
        dxa, dsk = DC.conv2d_dgrad_padded(gdz, gw, (B, ci, H, W), split_c1=c1, wino=True)
        torch.cuda.synchronize()
    assert rec.count >= 6, rec.count                                  # y, two weight operands, padded gradient, d coarse, d skip
    g.check()
    assert relmax(y, F.elu(pre64)) < 2e-5                             # the decoder-gather tolerance of tests/test_wino_gpu.py
    assert relmax(dxa, dxa64) < 2e-5 and relmax(dsk, dsk64) < 2e-5


@pytest.mark.parametrize("B,ci,co,H,W,up", [(1, 64, 64, 2, 2, False), (3, 32, 32, 5, 2, False), (1, 64, 32, 2, 6, False), (3, 32, 64, 6, 3, False),
                                            (1, 32, 32, 7, 4, False), (1, 32, 32, 4, 5, False), (1, 32, 32, 2, 2, True), (3, 32, 64, 4, 2, True),
                                            (1, 64, 32, 2, 6, True)])
@pytest.mark.parametrize("act", [None, "elu"])
def test_wino_wgrad_gen_narrow_images(gpu_device, B, ci, co, H, W, up, act):
    """The weight gradient of ReflectionPad2d(1) [+ upsample] + 3x3 on images narrower than one pair of Winograd tiles.  The pad
    tile of a pair meets zero dY values, but 0 x (what it reads) must still be 0: at W == 2 the kernel used to read the pixel in
    front of each row -- for row 0 of image 0 the 128 bytes in front of the tensor -- and a NaN there made every dw of the channel
    block NaN."""
    from deep_visual_slam_amd import conv as DC
    gen = _gen(H * W)
    x = torch.randn(B, ci, H // 2 if up else H, W // 2 if up else W, generator=gen)
    w = torch.randn(co, ci, 3, 3, generator=gen) * (2.0 / (ci * 9)) ** 0.5
    b = torch.randn(co, generator=gen) * 0.1
    dy = torch.randn(B, co, H, W, generator=gen)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = _ref_conv(None if up else x.double(), w64, b64, 1, 1, True, act, x.double() if up else None)
    dw64, db64 = torch.autograd.grad(y64, [w64, b64], dy.double())
    g = guard.Bands(gpu_device)
    gx, gdy = _cl(g, x), _cl(g, dy)
    gy = _cl(g, y64.detach().float()) if act else None
    sink = _cl(g, torch.full((co, ci, 3, 3), 0.5), guard.CANARY)
    bsink = g.place(torch.full((co,), 0.25), guard.CANARY) if act else None
    x2 = DC.UPSAMPLE_ONLY if up else None
    assert DC.wino_dec_wgrad_eligible((co, ci, 3, 3), gx, x2)
    with guard.allocations(*_mods()) as rec:
        dw, db = DC.conv3x3_wino_wgrad_gen(gx, x2, gdy, (co, ci, 3, 3), y_out=gy, act=act, want_bias=bool(act))
        got = DC.conv3x3_wino_wgrad_gen(gx, x2, gdy, (co, ci, 3, 3), y_out=gy, act=act, dw_out=sink, db_out=bsink)
        torch.cuda.synchronize()
    assert got == (None, None) and rec.count >= (2 if act else 1), rec.count
    g.check()
    assert relmax(dw, dw64) < WINO_TOL and relmax(sink - 0.5, dw64) < WINO_TOL + 1e-6 / float(dw64.abs().max())
    if act:
        assert relmax(db, db64) < 1e-5 and relmax(bsink - 0.25, db64) < 1e-5


# ---- thin decoder layers and heads (conv_thin.hip, conv_head.hip) ---------------------------------------------------------
THIN = [(1, 32, 16, 9, 63), (3, 32, 16, 9, 64), (1, 64, 32, 9, 65), (1, 16, 16, 33, 47), (3, 16, 16, 5, 64), (1, 32, 32, 13, 128)]


@pytest.mark.parametrize("B,ci,co,H,W", THIN)
@pytest.mark.parametrize("bias_act", [(True, "elu"), (False, None)], ids=["elu_bias", "plain"])
def test_thin_decoder_conv(gpu_device, B, ci, co, H, W, bias_act):
    from deep_visual_slam_amd import conv as DC
    has_b, act = bias_act
    assert DC.supported(torch.empty(B, ci, H, W), torch.empty(co, ci, 3, 3))
    _autograd_case(gpu_device, lambda x, w, b, xa: DC.conv2d(x, w, b, 1, 0, 1, act), B, ci, co, 3, 1, 1, True, H, W, act, has_b)


@pytest.mark.parametrize("B,c1,c2,co,H,W", [(1, 32, 16, 16, 10, 66), (3, 32, 0, 16, 6, 126), (1, 32, 32, 32, 18, 62)])
def test_thin_decoder_upsample_concat(gpu_device, B, c1, c2, co, H, W):
    from deep_visual_slam_amd import conv as DC
    _autograd_case(gpu_device, lambda x, w, b, xa: DC.conv2d(xa, w, b, 1, 0, 1, "elu", x2=x, upsample=x is None),
                   B, c1 + c2, co, 3, 1, 1, True, H, W, "elu", True, c1=c1)


HEADS = [(1, 16, 1, 3, 2, 2), (3, 16, 1, 3, 3, 4), (1, 16, 1, 3, 70, 33), (1, 256, 1, 3, 3, 4), (3, 256, 2, 3, 2, 2), (1, 64, 1, 3, 70, 33),
         (3, 256, 6, 1, 2, 2), (1, 256, 6, 1, 3, 4), (1, 16, 8, 3, 5, 65)]


@pytest.mark.parametrize("B,ci,co,k,H,W", HEADS)
def test_head_conv(gpu_device, B, ci, co, k, H, W):
    """The disparity heads (reflect pad 1, 3x3, sigmoid) and PoseNet's 6-channel 1x1."""
    from deep_visual_slam_amd import conv as DC
    refl, act = (True, "sigmoid") if k == 3 else (False, None)
    p = k // 2
    assert DC.head_supported(torch.empty(B, ci, H, W), torch.empty(co, ci, k, k), 1, 0 if refl else p, p if refl else 0)
    _autograd_case(gpu_device, lambda x, w, b, xa: DC.head_conv2d(x, w, b, 0 if refl else p, p if refl else 0, act),
                   B, ci, co, k, 1, p, refl, H, W, act, True, allocs=3)


# ---- stem (conv_stem.hip): 7x7 stride 2 from the planar image with the input normalisation fused --------------------------
@pytest.mark.parametrize("B,cin,H,W", [(1, 3, 38, 50), (3, 6, 38, 50), (1, 6, 37, 259), (3, 3, 37, 259)])
def test_stem_conv(gpu_device, B, cin, H, W):
    from deep_visual_slam_amd import conv as DC
    gen = _gen(4)
    x = torch.rand(B, cin, H, W, generator=gen)
    w = torch.randn(64, cin, 7, 7, generator=gen) * 0.05
    w64 = w.double().requires_grad_(True)
    y64 = F.conv2d((x.double() - 0.45) / 0.225, w64, None, 2, 3)
    cot = torch.randn(y64.shape, generator=gen)
    (gw64,) = torch.autograd.grad(y64, [w64], cot.double())
    g = guard.Bands(gpu_device)
    gx = g.place(x)                                                 # planar NCHW, contiguous: taken as it is
    gw = g.place(w).requires_grad_(True)
    sc, sh = g.place(torch.full((cin,), 1 / 0.225)), g.place(torch.full((cin,), -0.45 / 0.225))
    gcot = _cl(g, cot)
    assert gx.is_contiguous() and DC.supported(gx, gw, planar=True)
    with guard.allocations(*_mods()) as rec:
        y = DC.conv2d(gx, gw, None, 2, 3, 0, None, planar_norm=(sc, sh))
        (gwg,) = torch.autograd.grad(y, [gw], gcot)
        torch.cuda.synchronize()
    assert rec.count >= 2, rec.count
    g.check()
    assert relmax(y, y64) < 2e-5 and relmax(gwg, gw64) < 1e-4


# ---- max-pool (uint8 argmax buffer), upsample2x (pool.hip) -------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W", [(1, 16, 7, 9), (3, 64, 10, 5), (1, 4, 3, 5), (3, 12, 1, 1), (1, 64, 15, 21)])
def test_max_pool_and_upsample(gpu_device, B, C, H, W):
    from deep_visual_slam_amd import nn_ops
    gen = _gen(5)
    x = torch.randn(B, C, H, W, generator=gen)
    x64 = x.double().requires_grad_(True)
    y64 = F.max_pool2d(x64, 3, 2, 1)
    cot = torch.randn(y64.shape, generator=gen)
    (dx64,) = torch.autograd.grad(y64, [x64], cot.double())
    u64 = F.interpolate(x64, scale_factor=2, mode="nearest")
    ucot = torch.randn(u64.shape, generator=gen)
    (du64,) = torch.autograd.grad(u64, [x64], ucot.double())
    g = guard.Bands(gpu_device)
    gx, gcot, gucot = _cl(g, x, grad=True), _cl(g, cot), _cl(g, ucot)
    with guard.allocations(*_mods(nn_ops)) as rec:
        y = nn_ops.max_pool_3x3_s2(gx)
        (dx,) = torch.autograd.grad(y, [gx], gcot)
        u = nn_ops.upsample_nearest2x(gx)
        (du,) = torch.autograd.grad(u, [gx], gucot)
        torch.cuda.synchronize()
    assert rec.count >= 5, rec.count                                 # y, the uint8 index, dx, u, du
    assert any(b.nbytes == y.numel() for b in rec.bands)       # the one-byte-per-element index
    g.check()
    assert relmax(y, y64) == 0.0 and relmax(u, u64) == 0.0
    assert relmax(dx, dx64) < 1e-6 and relmax(du, du64) < 1e-6


# ---- ViT kernels (vit.hip) ------------------------------------------------------------------------------------------------
def _attn_err(got, want, i):
    """relmax of component i (dq, dk, dv) of d qkv.  With a single key the softmax is constant and dq is exactly zero: that
    component is then judged against the scale of the whole gradient (a relative error against 0 has no meaning)."""
    scale = want[:, :, i].abs().max()
    scale = scale if float(scale) > 0.0 else want.abs().max()
    g = got[:, :, i].detach().double().cpu()
    assert torch.isfinite(g).all(), "non-finite output: a guard value reached the arithmetic"
    return float((g - want[:, :, i].detach()).abs().max() / scale)


def _attn_ref(qkv):
    B, N, _, heads, _ = qkv.shape
    q, k, v = qkv.permute(2, 0, 3, 1, 4)
    return (((q * 0.125) @ k.transpose(-2, -1)).softmax(-1) @ v).transpose(1, 2).reshape(B * N, heads * 64)


@pytest.mark.parametrize("B,N,heads", [(1, 1, 2), (3, 1, 6), (3, 31, 6), (1, 32, 12), (3, 32, 2), (3, 33, 2), (1, 33, 6), (1, 64, 6), (3, 64, 12),
                                       (3, 257, 2), (1, 257, 12), (1, 1370, 6)])
def test_attention_fwd_bwd(gpu_device, B, N, heads):
    """The 32-token tile: shorter than a tile, exactly one / two tiles, one key in the last tile (33, 257), 1370 = 42 tiles + 26."""
    from deep_visual_slam_amd import depth_anything_v2 as DA
    gen = _gen(N + heads)
    qkv = torch.randn(B, N, 3, heads, 64, generator=gen) * 1.2
    cot = torch.randn(B * N, heads * 64, generator=gen)
    q64 = qkv.double().requires_grad_(True)
    ref = _attn_ref(q64)
    (dq64,) = torch.autograd.grad(ref, [q64], cot.double())
    g = guard.Bands(gpu_device)
    x = g.place(qkv.reshape(B * N, -1)).requires_grad_(True)
    gcot = g.place(cot)
    with guard.allocations(DA) as rec:
        inf = DA.attention(x.detach(), B, N, heads, 64)
        out = DA._AttentionF.apply(x, B, N, heads, 64)
        (dqkv,) = torch.autograd.grad(out, [x], gcot)
        torch.cuda.synchronize()
    assert rec.count >= 5, rec.count                                 # out (twice), lse, delta, d_qkv
    g.check()
    assert relmax(inf, ref) < 2e-5 and relmax(out, ref) < 2e-5
    got, want = dqkv.reshape(B, N, 3, heads, 64), dq64
    for i, name in enumerate(("dq", "dk", "dv")):
        e = _attn_err(got, want, i)
        assert e < 5e-5, (name, e)


@pytest.mark.parametrize("N", [1, 31, 33, 64])
def test_attention_does_not_read_the_neighbouring_image(gpu_device, N):
    """In a batch, image b's tail sits directly in front of image b+1's tokens: with images 0 and 2 all NaN, image 1 must come
    out as if it were alone, forward and backward."""
    from deep_visual_slam_amd import depth_anything_v2 as DA
    heads = 2
    gen = _gen(N)
    qkv = torch.randn(3, N, 3, heads, 64, generator=gen) * 1.2
    cot = torch.randn(3 * N, heads * 64, generator=gen)
    q64 = qkv[1:2].double().requires_grad_(True)
    ref = _attn_ref(q64)
    (dq64,) = torch.autograd.grad(ref, [q64], cot[N:2 * N].double())
    qkv[0], qkv[2] = float("nan"), float("nan")
    cot[:N], cot[2 * N:] = float("nan"), float("nan")
    g = guard.Bands(gpu_device)
    x = g.place(qkv.reshape(3 * N, -1)).requires_grad_(True)
    gcot = g.place(cot)
    with guard.allocations(DA) as rec:
        out = DA._AttentionF.apply(x, 3, N, heads, 64)
        (dqkv,) = torch.autograd.grad(out, [x], gcot)
        torch.cuda.synchronize()
    assert rec.count >= 4
    g.check()
    assert relmax(out[N:2 * N], ref) < 2e-5
    for i, name in enumerate(("dq", "dk", "dv")):
        e = _attn_err(dqkv[N:2 * N].reshape(1, N, 3, heads, 64), dq64, i)
        assert e < 5e-5, (name, e)


@pytest.mark.parametrize("M", [1, 5, 700])
@pytest.mark.parametrize("C", [64, 384, 1024])
def test_layernorm_fwd_bwd(gpu_device, M, C):
    from deep_visual_slam_amd import depth_anything_v2 as DA
    gen = _gen(C + M)
    x, w, b = torch.randn(M, C, generator=gen) * 2 + 0.3, torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    cot = torch.randn(M, C, generator=gen)
    l64 = [t.double().requires_grad_(True) for t in (x, w, b)]
    y64 = F.layer_norm(l64[0], (C,), l64[1], l64[2], 1e-6)
    g64 = torch.autograd.grad(y64, l64, cot.double())
    g = guard.Bands(gpu_device)
    gx, gw, gb = (g.place(t).requires_grad_(True) for t in (x, w, b))
    gcot = g.place(cot)
    with guard.allocations(DA) as rec:
        y = DA._LayerNormF.apply(gx, gw, gb, 1e-6)
        grads = torch.autograd.grad(y, [gx, gw, gb], gcot)
        torch.cuda.synchronize()
    assert rec.count >= 4, rec.count                                 # y, dx, dgamma, dbeta
    g.check()
    assert relmax(y, y64) < 2e-5
    for nm, a, r in zip(("dx", "dgamma", "dbeta"), grads, g64):
        assert relmax(a, r) < 5e-5, (nm, relmax(a, r))


@pytest.mark.parametrize("B,C,h,w,H,W", [(1, 32, 9, 12, 19, 25), (3, 64, 5, 7, 5, 7), (1, 4, 1, 3, 7, 2), (3, 32, 19, 19, 37, 38)])
def test_resize_bilinear_fwd_bwd(gpu_device, B, C, h, w, H, W):
    from deep_visual_slam_amd import depth_anything_v2 as DA
    gen = _gen(6)
    x = torch.randn(B, C, h, w, generator=gen)
    x64 = x.double().requires_grad_(True)
    y64 = F.interpolate(x64, (H, W), mode="bilinear", align_corners=True)
    cot = torch.randn(y64.shape, generator=gen)
    (dx64,) = torch.autograd.grad(y64, [x64], cot.double())
    g = guard.Bands(gpu_device)
    gx, gcot = _cl(g, x, grad=True), _cl(g, cot)
    with guard.allocations(DA) as rec:
        y = DA._ResizeF.apply(gx, H, W)
        (dx,) = torch.autograd.grad(y, [gx], gcot)
        torch.cuda.synchronize()
    assert rec.count >= 2
    g.check()
    assert relmax(y, y64) < 2e-6 and relmax(dx, dx64) < 2e-5


@pytest.mark.parametrize("B,k,co,h,w", [(1, 2, 8, 5, 6), (3, 4, 12, 3, 7), (1, 2, 96, 7, 9)])
def test_deconv_shuffle_and_unshuffle(gpu_device, B, k, co, h, w):
    from deep_visual_slam_amd import depth_anything_v2 as DA
    gen = _gen(7)
    src = torch.randn(B, k * k * co, h, w, generator=gen)
    # [B, (ky, kx, co), h, w] -> [B, co, h*k, w*k]
    ref = src.view(B, k, k, co, h, w).permute(0, 3, 4, 1, 5, 2).reshape(B, co, h * k, w * k)
    cot = torch.randn(ref.shape, generator=gen)
    dref = cot.view(B, co, h, k, w, k).permute(0, 3, 5, 1, 2, 4).reshape(B, k * k * co, h, w)
    g = guard.Bands(gpu_device)
    gs, gcot = _cl(g, src, grad=True), _cl(g, cot)
    with guard.allocations(DA) as rec:
        y = DA._ShuffleF.apply(gs, k, co)
        (dg,) = torch.autograd.grad(y, [gs], gcot)
        torch.cuda.synchronize()
    assert rec.count >= 2
    g.check()
    assert relmax(y, ref) == 0.0 and relmax(dg, dref) == 0.0


# ---- fused Adam (optim.hip) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 1001, 3 * 2 ** 20 + 3])
def test_fused_adam_stays_inside_its_four_arrays(gpu_device, n):
    """n = 3 * 2^20 + 3 crosses the 2048-block grid-stride cap and ends in a 3-element scalar tail next to 16-byte vector
    stores.  Against torch.optim.Adam, three steps, at tests/test_optim_gpu.py's tolerance."""
    from deep_visual_slam_amd import _lib
    gen = _gen(n % 1000)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * s for s in (1.0, 0.1, 3.0)]
    ref = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.Adam([ref], lr=1e-3)
    g = guard.Bands(gpu_device)
    p, gr, m, v = (g.place(t, guard.CANARY) for t in (p0, grads[0], torch.zeros(n), torch.zeros(n)))
    for step, gstep in enumerate(grads, 1):
        ref.grad = gstep.clone().double()
        opt.step()
        gr.copy_(gstep)
        _lib.check(_lib.lib().dvs_adam_step(_lib.ptr(p), _lib.ptr(gr), _lib.ptr(m), _lib.ptr(v), n, 1e-3, 0.9, 0.999, 1e-8, step, 1.0,
                                            int(step == 3), _lib.stream()), "dvs_adam_step")
    g.check()
    assert len(g) == 4
    assert torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(v).all()
    assert torch.allclose(p.cpu().double(), ref.detach(), atol=1e-6, rtol=1e-5)
    assert float(gr.abs().max()) == 0.0                              # zero_grad fused into the last pass, tail included


# ---- BatchNorm forward / backward, stem tail (norm.hip) ------------------------------------------------------------------------
def _guarded_bn(g, C, gen):
    """nn.BatchNorm2d whose affine parameters sit between NaN bands (they are read) and whose running statistics and step
    counter sit between canaries (they are updated in place)."""
    bn = torch.nn.BatchNorm2d(C).train()
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.rand(C, generator=gen) * 0.6 - 0.3
    rm, rv = torch.randn(C, generator=gen) * 0.1, torch.rand(C, generator=gen) + 0.5
    bn.weight = torch.nn.Parameter(g.place(gamma))
    bn.bias = torch.nn.Parameter(g.place(beta))
    bn._buffers["running_mean"] = g.place(rm, guard.CANARY)
    bn._buffers["running_var"] = g.place(rv, guard.CANARY)
    bn._buffers["num_batches_tracked"] = g.place(torch.zeros((), dtype=torch.int64), guard.CANARY)
    return bn, gamma, beta, rm, rv


def _bn_ref(y, gamma, beta, rm, rv, groups, eps=1e-5, momentum=0.1):
    """fp64 training-mode BatchNorm per sub-batch, running statistics updated group after group."""
    outs = []
    rm, rv = rm.double().clone(), rv.double().clone()
    for part in y.chunk(groups, 0):
        outs.append(F.batch_norm(part, None, None, gamma, beta, True, 0.0, eps))
        n = part.numel() // part.shape[1]
        mean, var = part.detach().mean((0, 2, 3)), part.detach().var((0, 2, 3), unbiased=False)
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * n / max(n - 1, 1)
    return torch.cat(outs, 0), rm, rv


def _stats(y, groups, slots=1):
    """[G][2][C] sum / sum of squares per sub-batch as the conv epilogue leaves them; slots > 1: [slots][G][2][C] whose sum is that."""
    st = torch.stack([torch.stack([p.sum((0, 2, 3)), (p * p).sum((0, 2, 3))]) for p in y.double().chunk(groups, 0)])
    if slots > 1:
        share = torch.linspace(0.5, 1.5, slots, dtype=torch.float64)
        return (st[None] * (share / share.sum())[:, None, None, None]).float()
    return (st if groups > 1 else st[0]).float()


BN = [
    # B, C, H, W, groups, slots, mode
    (1, 16, 15, 21, 1, 1, "relu"), (3, 64, 9, 10, 1, 1, "relu"), (2, 512, 3, 5, 2, 1, "relu"), (2, 64, 15, 21, 2, 4, "relu"),
    (3, 16, 3, 5, 1, 16, "residual"), (2, 64, 9, 10, 2, 1, "residual"), (1, 512, 15, 21, 1, 1, "residual"), (3, 64, 15, 21, 1, 1, "plain"),
]


@pytest.mark.parametrize("B,C,H,W,groups,slots,mode", BN)
@pytest.mark.parametrize("fused_bwd", [True, False], ids=["fused_bwd", "two_pass_bwd"])
def test_batchnorm_fwd_bwd(gpu_device, B, C, H, W, groups, slots, mode, fused_bwd):
    from deep_visual_slam_amd import bn as DB
    gen = _gen(C + H)
    y = torch.randn(B, C, H, W, generator=gen) * 1.5 + 0.3
    res = torch.randn(B, C, H, W, generator=gen) if mode == "residual" else None
    cot = torch.randn(B, C, H, W, generator=gen)
    g = guard.Bands(gpu_device)
    bn, gamma, beta, rm, rv = _guarded_bn(g, C, gen)
    assert DB.supported_c(C, bn)
    l64 = [t.double().requires_grad_(True) if t is not None else None for t in (y, gamma, beta, res)]
    z64, rm64, rv64 = _bn_ref(l64[0], l64[1], l64[2], rm, rv, groups)
    z64 = z64 + l64[3] if res is not None else z64
    z64 = F.relu(z64) if mode != "plain" else z64
    g64 = torch.autograd.grad(z64, [t for t in l64 if t is not None], cot.double())
    gy = _cl(g, y, grad=True)
    gres = _cl(g, res, grad=True) if res is not None else None
    gst, gcot = g.place(_stats(y, groups, slots)), _cl(g, cot)
    old, DB._BWD_FUSED = DB._BWD_FUSED, fused_bwd
    try:
        with guard.allocations(*_mods(DB)) as rec:
            z = DB.bn_act(gy, bn, gst, relu=mode != "plain", residual=gres, groups=groups)
            grads = torch.autograd.grad(z, [t for t in (gy, bn.weight, bn.bias, gres) if t is not None], gcot)
            torch.cuda.synchronize()
    finally:
        DB._BWD_FUSED = old
    assert rec.count >= 5, rec.count                                  # z, the [G][4][C] table, dy, the channel sums, the slot table
    g.check()
    assert relmax(z, z64) < 5e-5
    assert relmax(bn.running_mean, rm64) < 1e-4 and relmax(bn.running_var, rv64) < 1e-4 and int(bn.num_batches_tracked) == groups
    for nm, a, r in zip([n for n, t in zip(("dy", "dgamma", "dbeta", "dres"), l64) if t is not None], grads, g64):
        assert relmax(a, r) < 5e-4, (nm, relmax(a, r))


@pytest.mark.parametrize("B,C,H,W,groups,need_z", [(1, 64, 15, 21, 1, True), (2, 16, 9, 10, 2, True), (3, 64, 3, 5, 1, False), (2, 64, 7, 9, 2, False)])
def test_stem_tail_bn_relu_maxpool(gpu_device, B, C, H, W, groups, need_z):
    """relu(bn1(y)) -> MaxPool2d(3, 2, 1) in one pass, with the uint8 argmax buffer, forward and backward."""
    from deep_visual_slam_amd import bn as DB
    gen = _gen(C + W)
    y = torch.randn(B, C, H, W, generator=gen) * 1.5 + 0.3
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    cot_p, cot_z = torch.randn(B, C, Ho, Wo, generator=gen), torch.randn(B, C, H, W, generator=gen)
    g = guard.Bands(gpu_device)
    bn, gamma, beta, rm, rv = _guarded_bn(g, C, gen)
    l64 = [t.double().requires_grad_(True) for t in (y, gamma, beta)]
    z64 = F.relu(_bn_ref(l64[0], l64[1], l64[2], rm, rv, groups)[0])
    p64 = F.max_pool2d(z64, 3, 2, 1)
    loss64 = (p64 * cot_p.double()).sum() + ((z64 * cot_z.double()).sum() if need_z else 0.0)
    g64 = torch.autograd.grad(loss64, l64)
    gy, gst, gcp, gcz = _cl(g, y, grad=True), g.place(_stats(y, groups)), _cl(g, cot_p), _cl(g, cot_z)
    with guard.allocations(*_mods(DB)) as rec:
        z, p = DB.bn_relu_pool(gy, bn, gst, groups=groups, need_z=need_z)
        outs, cots = ([p, z], [gcp, gcz]) if need_z else ([p], [gcp])
        grads = torch.autograd.grad(outs, [gy, bn.weight, bn.bias], cots)
        torch.cuda.synchronize()
    assert rec.count >= 6, rec.count                                  # table, pooled, uint8 index, dy, sums, slot table (+ z)
    g.check()
    assert relmax(p, p64) < 5e-5 and (not need_z or relmax(z, z64) < 5e-5)
    for nm, a, r in zip(("dy", "dgamma", "dbeta"), grads, g64):
        assert relmax(a, r) < 5e-4, (nm, relmax(a, r))


# ---- loss chain, pose, stand-alone operators (loss_chain.hip, pose.hip, standalone.hip) -------------------------------------------
def _chain_case(dev, sample, disps, poses, noise, ns, auto_mask=True, materialize=False):
    from deep_visual_slam_amd import ops
    g = guard.Bands(dev)
    P = lambda t: g.place(t.contiguous())
    d_disps = [P(d).requires_grad_(True) for d in disps[:ns]]
    d_poses = [P(p).requires_grad_(True) for p in poses]
    nz = P(torch.stack(noise)) if noise is not None else None
    ins = [P(sample[(k, 0)]) for k in ("target_image", "source_left", "source_right", "K", "inv_K")]
    with guard.allocations(ops) as rec:
        T_l = ops.pose_to_mat(d_poses[0][:, 0], d_poses[1][:, 0], invert=True)
        T_r = ops.pose_to_mat(d_poses[2][:, 0], d_poses[3][:, 0], invert=False)
        losses, sel, extras = ops.loss_chain(*ins, T_l, T_r, d_disps, noise=nz, materialize=materialize, auto_mask=auto_mask)
        total = losses.mean()
        grads = torch.autograd.grad(total, d_disps + d_poses)
        torch.cuda.synchronize()
    # 2 pose matrices; partial sums, the uint8 selection, statistics, losses; d disp per scale, 2 d T, backward partial sums; 2 x (d aa, d t)
    assert rec.count >= 2 + 4 + ns + 3 + 4 + (6 * ns if materialize else 0), rec.count
    assert any(b.nbytes == sel.numel() for b in rec.bands)
    g.check()
    for t in [losses, T_l, T_r] + list(grads) + [v for e in extras for k in ("disp_up", "depth") for v in (e[k],)]:
        assert torch.isfinite(t).all()
    return dict(losses=losses, total=total, sel=sel, extras=extras, T=(T_l, T_r), d_disp=grads[:ns], d_pose=grads[ns:])


@pytest.mark.parametrize("B,H,W,ns", [(1, 50, 70, 1), (3, 80, 200, 4), (2, 48, 64, 4), (1, 48, 64, 4)])
def test_loss_chain_vs_oracle(gpu_device, B, H, W, ns):
    """Sizes around the 64 x 16 tile, one and four scales, against the CPU oracle at tests/test_chain_gpu.py's tolerances."""
    from test_chain_gpu import close, close_frac, close_pose
    from deep_visual_slam_amd import synth
    from oracle import loss_chain as O
    sample = synth.parity_sample(B, H, W, seed=77)
    disps = synth.parity_disps(B, H, W, seed=3)[:ns]
    poses = synth.parity_poses(B, seed=5)
    gen = _gen(7)
    noise = [torch.randn(B, 2, H, W, generator=gen) for _ in range(ns)]
    _, ref_losses, ref_grads = O.loss_chain_with_grads(sample, disps, poses, noise, num_scales=ns, auto_mask=True)
    out = _chain_case(gpu_device, sample, disps, poses, noise, ns, materialize=(H == 48))
    close(out["total"], ref_losses["loss"], 1e-7, 1e-5)
    for s in range(ns):
        close(out["losses"][s], ref_losses["loss/%d" % s], 1e-7, 1e-5)
        close_frac(out["d_disp"][s], ref_grads["disp"][s], atol=2e-8, rtol=2e-3)
    for i in range(4):
        close_pose(out["d_pose"][i], ref_grads["pose"][i], B * H * W)


def test_loss_chain_out_of_image_poses(gpu_device):
    """The golden case whose poses push >= 10 % of the samples over each image border: the bilinear fetch clamps, it must not read
    the rows and columns beyond the source images."""
    from conftest import golden_chain_inputs, load_golden
    from test_chain_gpu import close, close_frac, close_pose
    rec = load_golden("chain_b2_48x64_oob.npz")
    sample, disps, poses, noise, ns = golden_chain_inputs(rec)
    out = _chain_case(gpu_device, sample, disps, poses, noise, ns, materialize=True)
    close(out["total"], rec["loss"], 1e-7, 1e-5)
    for s in range(ns):
        close(out["losses"][s], rec["loss/%d" % s], 1e-7, 1e-5)
        close_frac(out["d_disp"][s], rec["grad/disp%d" % s], atol=2e-8, rtol=2e-3)
        for f, nm in ((0, "m1"), (1, "p1")):
            close(out["extras"][s]["color"][f], rec["out/color_%s_%d" % (nm, s)], 2e-5, 2e-5)
    for i, n in enumerate(("aa_left", "t_left", "aa_right", "t_right")):
        close_pose(out["d_pose"][i], rec["grad/" + n], sample[("target_image", 0)][:, 0].numel())


@pytest.mark.parametrize("B,H,W", [(1, 50, 70), (3, 24, 40), (2, 17, 65)])
def test_standalone_operators(gpu_device, B, H, W):
    """SSIM, edge-aware smoothness, back-projection and projection as their own launches, against the fp64 oracle restatements
    at tests/test_ops_gpu.py's tolerances."""
    import numpy as np
    from deep_visual_slam_amd import ops, synth
    from oracle import loss_chain as O
    gen = _gen(H)
    x, yv = torch.rand(B, 3, H, W, generator=gen), torch.rand(B, 3, H, W, generator=gen)
    disp = torch.rand(B, 1, H, W, generator=gen) * 0.8 + 0.1
    depth = torch.rand(B, 1, H, W, generator=gen) * 5 + 0.5
    cot_s = torch.randn(B, 3, H, W, generator=gen)
    cot_g = torch.randn(B, H, W, 2, generator=gen)
    intr = synth.intrinsics(B, H, W)
    K, inv_K = intr[("K", 0)], intr[("inv_K", 0)]
    aa, tr = synth.parity_poses(B, seed=5)[:2]
    T = O.transformation_from_parameters(aa[:, 0], tr[:, 0]).detach()

    def close(a, b, atol, rtol):
        a = a.detach().cpu()
        assert torch.isfinite(a).all()
        np.testing.assert_allclose(a.numpy(), b.detach().float().numpy(), atol=atol, rtol=rtol)

    x64, d64, z64, T64 = (t.double().requires_grad_(True) for t in (x, disp, depth, T))
    s64 = O.ssim(x64, yv.double())
    (dx64,) = torch.autograd.grad(s64, [x64], cot_s.double())
    sm64 = O.smooth_loss(d64, x.double())
    (dd64,) = torch.autograd.grad(sm64, [d64])
    cam64 = O.backproject(z64, inv_K.double())
    grid64 = O.project(cam64, K.double(), T64, H, W)
    dz64, dT64 = torch.autograd.grad(grid64, [z64, T64], cot_g.double())
    g = guard.Bands(gpu_device)
    gx, gd, gz, gT = (g.place(t).requires_grad_(True) for t in (x, disp, depth, T))
    gy, gK, giK, gcs, gcg = (g.place(t.contiguous()) for t in (yv, K, inv_K, cot_s, cot_g))
    with guard.allocations(ops) as rec:
        s = ops.ssim(gx, gy)
        (dx,) = torch.autograd.grad(s, [gx], gcs)
        sm = ops.smooth_loss(gd, gx.detach())
        (dd,) = torch.autograd.grad(sm, [gd])
        cam = ops.backproject(gz, giK)
        grid = ops.project(cam, gK, gT, H, W)
        dz, dT = torch.autograd.grad(grid, [gz, gT], gcg)
        torch.cuda.synchronize()
    assert rec.count >= 11, rec.count
    g.check()
    close(s, s64, 5e-5, 1e-5)
    close(dx, dx64, 2e-3, 2e-3)
    close(sm, sm64, 1e-8, 1e-5)
    close(dd, dd64, 1e-7, 1e-3)
    close(cam, cam64, 2e-6, 2e-5)
    close(grid, grid64, 1e-5, 1e-5)
    close(dz, dz64, 5e-3, 5e-3)
    close(dT, dT64, 5e-2, 5e-3)


# ---- supervised depth loss (depth_loss.hip), input side (preprocess.hip) ------------------------------------------------------
@pytest.mark.parametrize("B,H,W,valid", [(2, 50, 70, "column"), (1, 24, 40, "all"), (3, 24, 40, "random")])
def test_depth_loss(gpu_device, B, H, W, valid):
    from deep_visual_slam_amd import ops
    from oracle import depth_loss as OD
    gen = _gen(11)
    sizes = [(H, W), (H // 2, W // 2), (H // 4, W // 4), (H // 8, W // 8)]
    preds = [(torch.rand(B, 1, h, w, generator=gen) * 5 + 0.2) for h, w in sizes]
    rgb, gt = torch.rand(B, 3, H, W, generator=gen), torch.rand(B, 1, H, W, generator=gen) * 8 + 0.2
    if valid == "all":
        mask = torch.ones(B, 1, H, W, dtype=torch.bool)
    elif valid == "column":
        mask = torch.zeros(B, 1, H, W, dtype=torch.bool)
        mask[:, :, :, 3] = True
    else:
        mask = torch.rand(B, 1, H, W, generator=gen) < 0.7
    # the learner's own weighting of the per-scale terms (depth/depth_learner.py:97-117), so the gradients have the scale
    # tests/test_depth_learner_gpu.py's tolerance was written for
    ref_in = [p.double().requires_grad_(True) for p in preds]
    tot, _, _, silog_r, smooth_r = OD.multi_scale_loss(ref_in, gt.double(), rgb.double(), mask)
    g64 = torch.autograd.grad(tot, ref_in)
    g = guard.Bands(gpu_device)
    gp = [g.place(p).requires_grad_(True) for p in preds]
    ggt, grgb = g.place(gt), g.place(rgb)
    gmask = g.place(mask.to(torch.uint8))
    with guard.allocations(ops) as rec:
        silog, smooth = ops.depth_multiscale_losses(gp, ggt, grgb, gmask)
        alphas = torch.tensor(OD.ALPHAS, device=gpu_device)
        total = (silog * alphas).sum() + 0.1 * (smooth * alphas).sum()
        grads = torch.autograd.grad(total, gp)
        torch.cuda.synchronize()
    assert rec.count >= 2 + 4, rec.count                              # workspace, the 2 S results, one gradient per scale
    g.check()
    for s in range(4):
        assert abs(float(silog[s].detach()) - float(silog_r[s].detach())) < 1e-5 * abs(float(silog_r[s].detach())), s
        assert abs(float(smooth[s].detach()) - float(smooth_r[s].detach())) < 1e-5 * abs(float(smooth_r[s].detach())), s
        a, r = grads[s].detach().cpu().double(), g64[s]
        assert torch.isfinite(a).all()
        bad = (a - r).abs() > 2e-7 + 2e-3 * r.abs()
        assert float(bad.double().mean()) <= 2e-3, (s, float(bad.double().mean()))


@pytest.mark.parametrize("N,h,w,oh,ow", [(1, 37, 53, 24, 40), (3, 11, 7, 24, 40), (2, 50, 70, 50, 33), (1, 5, 9, 13, 9)])
def test_preprocess_resize_and_to_float(gpu_device, N, h, w, oh, ow):
    """PIL-bilinear resize from odd source sizes (both passes, uint8 in and out) and the uint8 -> planar fp32 conversion."""
    import numpy as np
    from deep_visual_slam_amd import input_pipeline as IP
    from oracle import input_pipeline as OI
    rng = np.random.default_rng(h * w)
    u8 = rng.integers(0, 256, size=(N, h, w, 3), dtype=np.uint8)
    ref = np.stack([OI.pil_resize_bilinear(f, oh, ow) for f in u8])
    g = guard.Bands(gpu_device)
    gu8 = g.place(torch.from_numpy(u8))
    keys = []
    for n_in, n_out in ((w, ow), (h, oh)):                             # the coefficient tables the kernel reads, guarded too
        if n_in != n_out:
            b, c = IP.pil_bilinear_tables(n_in, n_out)
            keys.append((n_in, n_out, gu8.device))
            IP._resize_tables[keys[-1]] = (g.place(torch.from_numpy(b)), g.place(torch.from_numpy(c)))
    try:
        with guard.allocations(IP) as rec:
            got = IP.resize_u8(gu8, oh, ow)
            f32 = IP.u8_to_f32_planar(got) if oh * ow % 4 == 0 else None      # (the conversion takes H*W % 4 == 0 only, and says so)
            torch.cuda.synchronize()
    finally:
        for k in keys:
            IP._resize_tables.pop(k, None)
    assert rec.count >= int(f32 is not None) + int(h != oh) + int(w != ow), rec.count
    g.check()
    assert np.array_equal(got.cpu().numpy(), ref)                       # every byte, as tests/test_pipeline_gpu.py asks
    assert f32 is None or float((f32.cpu() - OI.to_tensor(ref)).abs().max()) <= 6e-8


# ---- bf16 patch kernels and their weight packs (conv_p16.hip), in the bf16 mode ---------------------------------------------------
def r16(t):
    return t.detach().to(torch.bfloat16).to(torch.float64)


@pytest.fixture
def bf16_mode():
    from deep_visual_slam_amd import _lib
    _lib.set_precision("bf16")
    try:
        yield
    finally:
        _lib.set_precision("fp32")


@pytest.mark.parametrize("B,ci,co,H,W,groups,slots", [(1, 64, 64, 15, 20, 1, 1), (3, 128, 64, 9, 13, 1, 4), (2, 64, 128, 17, 45, 2, 16),
                                                     (1, 64, 64, 7, 15, 1, 1), (3, 64, 64, 8, 16, 1, 1), (1, 64, 64, 9, 17, 1, 16)])
def test_p16_patch_kernel(gpu_device, bf16_mode, B, ci, co, H, W, groups, slots):
    """Forward with the statistics epilogue, data gradient with a residual, weight gradient (fresh and into a guarded sink) at
    sizes on both sides of the 8 x 16 patch; the bf16 weight packs are allocated inside the context.  Against the mode's
    specification (bf16-rounded operands, fp64) at tests/test_bf16_gpu.py's tolerances."""
    from deep_visual_slam_amd import conv as DC
    gen = _gen(4)
    x = torch.randn(B, ci, H, W, generator=gen)
    w = torch.randn(co, ci, 3, 3, generator=gen) * (2.0 / (ci * 9)) ** 0.5
    dy, res = torch.randn(B, co, H, W, generator=gen), torch.randn(B, ci, H, W, generator=gen)
    yr = F.conv2d(r16(x), r16(w), None, 1, 1)
    dxr = F.conv_transpose2d(r16(dy), r16(w), None, 1, 1) + res.double()
    wv = r16(w).requires_grad_(True)
    (dwr,) = torch.autograd.grad(F.conv2d(r16(x), wv, None, 1, 1), [wv], r16(dy))
    g = guard.Bands(gpu_device)
    gx, gw, gdy, gres = _cl(g, x), _cl(g, w), _cl(g, dy), _cl(g, res)
    assert DC.p16_eligible(gw, 1, 1, False, None, None, False, None)
    stats = g.zeros((slots, groups, 2, co) if slots > 1 else ((groups, 2, co) if groups == 2 else (2, co)), pattern=guard.CANARY)
    sink = _cl(g, torch.full((co, ci, 3, 3), 0.5), guard.CANARY)
    with guard.allocations(*_mods()) as rec:
        y = DC.conv3x3_p16(gx, gw, stats, groups, stat_slots=slots)
        dx = DC.conv3x3_p16(gdy, gw, flip=True, residual=gres)
        dw = DC.conv3x3_p16_wgrad(gx, gdy, (co, ci, 3, 3))
        assert DC.conv3x3_p16_wgrad(gx, gdy, (co, ci, 3, 3), dw_out=sink) is None
        torch.cuda.synchronize()
    assert rec.count >= 5, rec.count                                  # y, dx, dw and the two bf16 packs
    assert sum(b.buf.dtype == torch.uint8 and b.nbytes == 2 * 9 * ci * co for b in rec.bands) >= 2
    g.check()
    assert relmax(y, yr) < 2e-5 and relmax(dx, dxr) < 1e-4
    assert relmax(dw, dwr) < 1e-4 and relmax(sink - 0.5, dwr) < 1e-4
    st = (stats.double().sum(0) if slots > 1 else stats.double()).reshape(groups, 2, co).cpu()
    for i in range(groups):
        yy = y.double().cpu()[i * B // groups:(i + 1) * B // groups]
        assert relmax(st[i, 0], yy.sum((0, 2, 3))) < 1e-5 and relmax(st[i, 1], (yy ** 2).sum((0, 2, 3))) < 1e-5


P16_DEC = [
    # B, c1, c2 (None: no upsample; 0: upsample only), co, H, W (of the output), act
    (1, 64, None, 32, 15, 20, "elu"), (3, 32, None, 16, 17, 45, "elu"), (1, 48, None, 32, 9, 13, None), (1, 16, 0, 16, 18, 26, "elu"),
    (3, 32, 64, 32, 10, 26, "elu"), (1, 128, None, 64, 9, 13, "elu"), (1, 64, 64, 64, 18, 30, "elu"),
    (1, 64, None, 64, 3, 5, "elu"), (3, 32, None, 16, 3, 3, "elu"),
]


@pytest.mark.parametrize("B,c1,c2,co,H,W,act", P16_DEC)
def test_p16_decoder_layers(gpu_device, bf16_mode, B, c1, c2, co, H, W, act):
    """The decoder's Conv3x3 layers on the patch kernels' general gather (reflect pad, upsample, concat), wide and thin
    (16 / 32 channels): forward against the bf16 specification, gradients against fp64 at the mode's 1e-2."""
    from deep_visual_slam_amd import conv as DC
    up = c2 is not None
    ci = c1 + (c2 or 0)
    xs = torch.empty(B, c1, H // 2 if up else H, W // 2 if up else W)
    x2 = torch.empty(B, c2, H, W) if c2 else (DC.UPSAMPLE_ONLY if up else None)
    assert DC.p16_dec_eligible(torch.empty(co, ci, 3, 3), 1, 1, True, act, xs, x2, False, None)
    _autograd_case(gpu_device, lambda x, w, b, xa: DC.conv2d(xa if up else x, w, b, 1, 0, 1, act, x2=x if (up and c2) else None, upsample=up),
                   B, ci, co, 3, 1, 1, True, H, W, act, True, c1=c1 if up else 0, tol=(2e-5, 1e-2), spec=r16)


@pytest.mark.parametrize("B,H,W,C", [(1, 28, 42, 64), (3, 14, 70, 384), (1, 42, 14, 1024)])
def test_vit_patchify_and_assemble(gpu_device, B, H, W, C):
    """The token front end at non-square sizes, through the C ABI with guarded pointers (no stand-alone wrapper exists): patch rows
    [B*Np][Kp] in (channel, ky, kx) order, zero-padded from 588 to 608 columns, and cls / position-embedding assembly."""
    from deep_visual_slam_amd import _lib
    P, K, Kp = 14, 3 * 14 * 14, 608
    Np = (H // P) * (W // P)
    gen = _gen(H + W)
    img = torch.randn(B, 3, H, W, generator=gen)
    tok, cls, pos = torch.randn(B * Np, C, generator=gen), torch.randn(C, generator=gen), torch.randn(Np + 1, C, generator=gen)
    rows_ref = F.pad(F.unfold(img, P, stride=P).transpose(1, 2).reshape(B * Np, K), (0, Kp - K))
    x_ref = (torch.cat([cls.expand(B, 1, C), tok.view(B, Np, C)], 1).double() + pos.double()).reshape(B * (Np + 1), C)
    g = guard.Bands(gpu_device)
    gimg, gtok, gcls, gpos = (g.place(t) for t in (img, tok, cls, pos))
    rows, x = g.empty((B * Np, Kp)), g.empty((B * (Np + 1), C))
    l = _lib.lib()
    _lib.check(l.dvs_vit_patchify(_lib.ptr(gimg), _lib.ptr(rows), B, H, W, P, Kp, _lib.stream()), "dvs_vit_patchify")
    _lib.check(l.dvs_vit_assemble(_lib.ptr(gtok), _lib.ptr(gcls), _lib.ptr(gpos), _lib.ptr(x), B, Np, C, _lib.stream()), "dvs_vit_assemble")
    assert len(g) == 6
    g.check()
    assert torch.equal(rows.cpu(), rows_ref)
    assert relmax(x, x_ref) < 1e-6                                    # one fp32 rounding of the sum
