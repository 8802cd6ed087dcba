"""Winograd F(2x2,3x3) kernel (csrc/conv_wino.hip; torchvision BasicBlock conv1/conv2 as used by model/resnet_encoder.py:94-111)
against F.conv2d in fp64: forward with the BatchNorm statistics epilogue, the data gradient through the rotated filter, the
batched weight transform, odd / tiny images and ragged channel blocks, and the autograd path of conv.conv2d that selects it."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CL = torch.channels_last


@pytest.fixture(autouse=True)
def _always_winograd():
    """The product picks the Winograd kernels by a cost model (conv.wino_pays: enough tiles to fill the chip); these tests
    exercise the kernels at every size."""
    from deep_visual_slam_amd import conv as DC
    old, DC._WINO_FORCE = DC._WINO_FORCE, True
    yield
    DC._WINO_FORCE = old


def test_cost_model_keeps_small_problems_on_the_direct_kernels():
    from deep_visual_slam_amd import conv as DC
    DC._WINO_FORCE = False
    # layer 1 .. 4 of the encoder at 480x640 (input of the 3x3 layers): batch 12 and 24 all Winograd, batch 1 only layer 1
    shapes = [(64, 120, 160), (128, 60, 80), (256, 30, 40), (512, 15, 20)]
    assert all(DC.wino_pays(12, h, w, c, c) and DC.wino_pays(24, h, w, c, c) for c, h, w in shapes)
    assert [DC.wino_pays(1, h, w, c, c) for c, h, w in shapes] == [True, False, False, False]
    assert not DC.wino_pays(2, 15, 20, 512, 512)          # 20 workgroups of 132 us against 42 us (tools/wino_bench.py, batch 2)
TOL = 3e-6        # max |err| / max |ref|; the direct kernel and MIOpen sit at 1-4e-6 on the same shapes (tools/wino_bench.py)


def _mk(B, ci, co, h, w, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, ci, h, w, device="cuda", generator=g).contiguous(memory_format=CL)
    wt = (torch.randn(co, ci, 3, 3, device="cuda", generator=g) * (2.0 / (ci * 9)) ** 0.5).contiguous(memory_format=CL)
    return x, wt


def _rel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


SHAPES = [(2, 64, 64, 120, 160), (2, 128, 128, 60, 80), (2, 256, 256, 30, 40), (2, 512, 512, 15, 20), (12, 512, 512, 15, 20),      # encoder, 480x640 (the 512-channel ones take the K split)
          (4, 64, 128, 13, 27), (2, 128, 64, 1, 5), (2, 64, 192, 7, 1), (6, 80, 96, 6, 6), (1, 64, 64, 2, 2)]


@pytest.mark.parametrize("B,ci,co,h,w", SHAPES)
def test_forward_stats_and_data_gradient(B, ci, co, h, w):
    from deep_visual_slam_amd import conv as DC
    x, wt = _mk(B, ci, co, h, w)
    y64 = F.conv2d(x.double(), wt.double(), None, 1, 1)
    for groups in (1, 2) if B % 2 == 0 else (1,):
        st = torch.zeros((2, co) if groups == 1 else (2, 2, co), device="cuda")
        y = DC.conv3x3_wino(x, wt, st, groups)
        assert y.shape == y64.shape and y.is_contiguous(memory_format=CL)
        assert _rel(y, y64) < TOL
        parts = [y64] if groups == 1 else [y64[: B // 2], y64[B // 2:]]
        ref = torch.stack([torch.stack([p.sum((0, 2, 3)), (p * p).sum((0, 2, 3))]) for p in parts])
        ref = ref[0] if groups == 1 else ref
        assert float((st.double() - ref).abs().max() / ref.abs().max()) < 2e-5
    dy = torch.randn(B, co, h, w, device="cuda").contiguous(memory_format=CL)
    dx64 = F.conv_transpose2d(dy.double(), wt.double(), None, 1, 1)
    dx = DC.conv3x3_wino(dy, wt, flip=True)
    assert dx.shape == x.shape and _rel(dx, dx64) < TOL


WSHAPES = [(2, 64, 64, 120, 160), (2, 128, 128, 60, 80), (2, 256, 256, 30, 40), (2, 512, 512, 15, 20), (12, 512, 512, 15, 20),
           (4, 64, 128, 13, 27), (2, 128, 64, 1, 5), (2, 64, 192, 7, 1), (6, 96, 96, 6, 6), (1, 64, 64, 2, 2)]


@pytest.mark.parametrize("B,ci,co,h,w", WSHAPES)
def test_weight_gradient(B, ci, co, h, w):
    """dW against fp64 autograd; into a fresh tensor and accumulated into a gradient sink that already holds values; with the
    tile range split over many workgroups (atomics) and owned by one (plain adds)."""
    from deep_visual_slam_amd import conv as DC
    x, _ = _mk(B, ci, co, h, w, seed=3)
    dy = torch.randn(B, co, h, w, device="cuda").contiguous(memory_format=CL)
    w64 = torch.zeros(co, ci, 3, 3, device="cuda", dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, None, 1, 1).backward(dy.double())
    ref = w64.grad
    for wgs in (0, 1, 4096):
        old, DC._WINO_WGS = DC._WINO_WGS, wgs
        try:
            dw = DC.conv3x3_wino_wgrad(x, dy, (co, ci, 3, 3))
            assert dw.shape == ref.shape and dw.permute(0, 2, 3, 1).is_contiguous()
            assert _rel(dw, ref) < 3e-6, wgs
            sink = torch.full((co, ci, 3, 3), 0.5, device="cuda").contiguous(memory_format=CL)
            assert DC.conv3x3_wino_wgrad(x, dy, (co, ci, 3, 3), dw_out=sink) is None
            assert _rel(sink - 0.5, ref) < 3e-6 + 1e-6 / float(ref.abs().max()), wgs
        finally:
            DC._WINO_WGS = old


def test_batched_weight_transform_matches_the_single_launches():
    from deep_visual_slam_amd import conv as DC
    ws = [_mk(1, ci, co, 2, 2, seed=s)[1] for s, (ci, co) in enumerate([(64, 64), (64, 128), (128, 128), (512, 256)])]
    ws.append(torch.randn(32, 16, 3, 3, device="cuda").contiguous(memory_format=CL))          # not eligible: left alone
    ref = [(DC._wino_weight(w, w, False).clone(), DC._wino_weight(w, w, True).clone()) for w in ws[:4]]
    DC._wino_packed.clear()
    pk = DC.PackedWeights(ws)
    assert len(pk.wino) == 4
    pk.repack()
    try:
        for w, (u, uf) in zip(ws[:4], ref):
            ent = DC._wino_packed[w.data_ptr()]
            assert torch.equal(ent[0], u) and torch.equal(ent[1], uf)
            assert DC._wino_weight(w, w, False) is ent[0]
    finally:
        pk.release()
    assert not DC._wino_packed


def test_operand_follows_the_weight():
    """An in-place weight update (any optimiser) bumps the version counter: the cached operand must not be served again."""
    from deep_visual_slam_amd import conv as DC
    x, wt = _mk(2, 64, 64, 8, 8)
    y0 = DC.conv3x3_wino(x, wt)
    with torch.no_grad():
        wt.mul_(2.0)
    y1 = DC.conv3x3_wino(x, wt)
    assert _rel(y1, 2.0 * y0.double()) < 1e-6


def test_same_shaped_weights_in_standard_layout_do_not_share_an_operand():
    """Weights that are not stored channels-last are copied to NHWC per call; the copies of two different weights can get the
    same address from the allocator, so the operand cache must be keyed by the weight itself."""
    from deep_visual_slam_amd import conv as DC
    x, _ = _mk(2, 64, 64, 8, 8)
    ws = [torch.randn(64, 64, 3, 3, device="cuda") * 0.05 for _ in range(4)]          # standard (NCHW-contiguous) layout
    for w in ws:
        y = DC.conv3x3_wino(x, w)
        assert _rel(y, F.conv2d(x.double(), w.double(), None, 1, 1)) < TOL


def test_operand_cache_is_pinned_to_the_weight_object():
    """A live parameter whose storage moved (an arena, .to()) leaves its old address to the allocator; an entry filed under
    that address for the OLD owner must not serve the new tenant even when version counter and shape agree."""
    import weakref
    from deep_visual_slam_amd import conv as DC
    x, wa = _mk(2, 64, 64, 8, 8, seed=1)
    _, wb = _mk(2, 64, 64, 8, 8, seed=2)
    ua = DC._wino_weight(wa, wa, False)
    DC._wino_packed[wb.data_ptr()] = [ua, None, wb._version, tuple(wb.shape), weakref.ref(wa)]     # what a moved `wa` leaves behind
    y = DC.conv3x3_wino(x, wb)
    assert _rel(y, F.conv2d(x.double(), wb.double(), None, 1, 1)) < TOL


def test_autograd_path_selects_it_and_matches_torch():
    from deep_visual_slam_amd import conv as DC
    x, wt = _mk(4, 64, 128, 24, 32)
    x.requires_grad_(True)
    wt.requires_grad_(True)
    assert DC.wino_eligible(wt, 1, 1, False, None, None, False, None) and DC.wino_pays(4, 24, 32, 64, 128)
    y, st = DC.conv2d(x, wt, None, 1, 1, want_stats=1)
    gy = torch.randn_like(y)
    y.backward(gy)
    x64, w64 = x.detach().double().requires_grad_(True), wt.detach().double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, 1, 1)
    y64.backward(gy.double())
    assert _rel(y, y64.detach()) < TOL and _rel(x.grad, x64.grad) < TOL and _rel(wt.grad, w64.grad) < 2e-5
    assert float((st[0].double() - y64.detach().sum((0, 2, 3))).abs().max() / y64.detach().sum((0, 2, 3)).abs().max()) < 2e-5
    # the switch: DVS_WINOGRAD=0 keeps every convolution on the direct kernels
    old, DC._WINO = DC._WINO, False
    try:
        assert not DC.wino_eligible(wt, 1, 1, False, None, None, False, None)
        y2 = DC.conv2d(x.detach(), wt.detach(), None, 1, 1)
    finally:
        DC._WINO = old
    assert _rel(y2, y64.detach()) < 6e-6


def test_rejects_what_it_does_not_cover():
    from deep_visual_slam_amd import _lib, conv as DC
    x, wt = _mk(1, 24, 64, 4, 4)
    with pytest.raises(_lib.DvsError):
        DC.conv3x3_wino(x, wt)                         # Cin % 16 != 0
    x, wt = _mk(1, 64, 64, 4, 4)
    with pytest.raises(_lib.DvsError):
        DC.conv3x3_wino(x[:, :32], wt)                 # channel mismatch


DEC = [  # B, C1, C2 (skip channels; -1: no upsample, 0: upsample only), Cout, h, w of x
    (2, 512, -1, 256, 15, 20), (2, 256, 256, 256, 15, 20), (2, 256, -1, 128, 30, 40), (2, 128, 128, 128, 30, 40),
    (2, 128, -1, 64, 60, 80), (2, 64, 64, 64, 60, 80), (1, 64, 0, 64, 5, 7), (3, 72, 56, 80, 3, 2), (1, 64, -1, 64, 2, 2)]


def _dec_ref(x, skip, up, wt, bias, act):
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    if skip is not None:
        xin = torch.cat([xin, skip], 1)
    y = F.conv2d(F.pad(xin, (1, 1, 1, 1), mode="reflect"), wt, bias)
    return F.elu(y) if act == "elu" else y


@pytest.mark.parametrize("B,c1,c2,co,h,w", DEC)
def test_decoder_gather_forward_and_padded_data_gradient(B, c1, c2, co, h, w):
    """ReflectionPad2d(1) + [upsample (+ concat)] + 3x3 + bias + ELU (model/layers.py:26-41, model/depth_decoder.py:52-62) and
    the full correlation of the padded-domain data gradient, against fp64 torch."""
    from deep_visual_slam_amd import conv as DC
    g = torch.Generator(device="cuda").manual_seed(5)
    up = c2 >= 0
    H, W = (2 * h, 2 * w) if up else (h, w)
    x = torch.randn(B, c1, h, w, device="cuda", generator=g).contiguous(memory_format=CL)
    skip = torch.randn(B, c2, H, W, device="cuda", generator=g).contiguous(memory_format=CL) if c2 > 0 else None
    ci = c1 + max(c2, 0)
    wt = (torch.randn(co, ci, 3, 3, device="cuda", generator=g) * (2.0 / (ci * 9)) ** 0.5).contiguous(memory_format=CL)
    bias = torch.randn(co, device="cuda", generator=g) * 0.1
    x2 = skip if skip is not None else (DC.UPSAMPLE_ONLY if up else None)
    for act in ("elu", None):
        y = DC.conv3x3_wino_gen(x, x2, wt, bias, act, reflect=True)
        ref = _dec_ref(x.double(), None if skip is None else skip.double(), up, wt.double(), bias.double(), act)
        assert y.shape == ref.shape and _rel(y, ref) < TOL, act
    dz = torch.randn(B, co, H, W, device="cuda", generator=g).contiguous(memory_format=CL)
    gp = DC.conv3x3_wino_gen(dz, None, wt, reflect=False, full=True, flip=True)
    ref = F.conv_transpose2d(dz.double(), wt.double())           # [B, ci, H+2, W+2]: gradient w.r.t. the padded input
    assert gp.shape == ref.shape and _rel(gp, ref) < TOL


DEC_W = [  # B, C1, C2 (-1: no upsample, 0: upsample only), Cout, h, w of x -- channel counts in 32-blocks, odd sizes without upsample
    (2, 512, -1, 256, 15, 20), (2, 256, 256, 256, 15, 20), (2, 256, -1, 128, 30, 40), (2, 128, 128, 128, 30, 40),
    (2, 128, -1, 64, 60, 80), (2, 64, 64, 64, 60, 80), (1, 64, 0, 64, 5, 7), (3, 96, 32, 64, 3, 2), (1, 64, -1, 64, 2, 2),
    (2, 64, -1, 32, 7, 5), (2, 32, -1, 64, 3, 9), (5, 32, 64, 32, 1, 1), (2, 64, -1, 64, 2, 3)]


@pytest.mark.parametrize("B,c1,c2,co,h,w", DEC_W)
def test_decoder_weight_gradient(B, c1, c2, co, h, w):
    """dW of ReflectionPad2d(1) + [upsample (+ concat)] + 3x3 (model/layers.py:26-41, model/depth_decoder.py:52-62) on the Winograd
    kernel's reflect / upsample gathers against fp64 autograd: fresh tensor, gradient sink, tile range split or owned."""
    from deep_visual_slam_amd import conv as DC
    g = torch.Generator(device="cuda").manual_seed(11)
    up = c2 >= 0
    H, W = (2 * h, 2 * w) if up else (h, w)
    x = torch.randn(B, c1, h, w, device="cuda", generator=g).contiguous(memory_format=CL)
    skip = torch.randn(B, c2, H, W, device="cuda", generator=g).contiguous(memory_format=CL) if c2 > 0 else None
    ci = c1 + max(c2, 0)
    x2 = skip if skip is not None else (DC.UPSAMPLE_ONLY if up else None)
    assert DC.wino_dec_wgrad_eligible((co, ci, 3, 3), x, x2)
    dz = torch.randn(B, co, H, W, device="cuda", generator=g).contiguous(memory_format=CL)
    w64 = torch.zeros(co, ci, 3, 3, device="cuda", dtype=torch.float64, requires_grad=True)
    _dec_ref(x.double(), None if skip is None else skip.double(), up, w64, None, None).backward(dz.double())
    ref = w64.grad
    for wgs in (0, 1, 4096):
        old, DC._WINO_WGS = DC._WINO_WGS, wgs
        try:
            dw, db = DC.conv3x3_wino_wgrad_gen(x, x2, dz, (co, ci, 3, 3))
            assert db is None and dw.shape == ref.shape and dw.permute(0, 2, 3, 1).is_contiguous()
            assert _rel(dw, ref) < 3e-6, wgs
            sink = torch.full((co, ci, 3, 3), 0.5, device="cuda").contiguous(memory_format=CL)
            assert DC.conv3x3_wino_wgrad_gen(x, x2, dz, (co, ci, 3, 3), dw_out=sink) == (None, None)
            assert _rel(sink - 0.5, ref) < 3e-6 + 1e-6 / float(ref.abs().max()), wgs
        finally:
            DC._WINO_WGS = old
    # the thin layers' form: dY times the activation derivative of the forward output on load, bias gradient on the way
    yo = torch.randn(B, co, H, W, device="cuda", generator=g).contiguous(memory_format=CL)
    for act in ("elu", "relu"):
        dact = (1.0 + yo.double().clamp(max=0.0)) if act == "elu" else (yo > 0).double()
        w64 = torch.zeros(co, ci, 3, 3, device="cuda", dtype=torch.float64, requires_grad=True)
        _dec_ref(x.double(), None if skip is None else skip.double(), up, w64, None, None).backward(dz.double() * dact)
        bref = (dz.double() * dact).sum((0, 2, 3))
        for wgs in (0, 4096):
            old, DC._WINO_WGS = DC._WINO_WGS, wgs
            try:
                dw, db = DC.conv3x3_wino_wgrad_gen(x, x2, dz, (co, ci, 3, 3), y_out=yo, act=act, want_bias=True)
                assert _rel(dw, w64.grad) < 3e-6 and _rel(db, bref) < 1e-5, (act, wgs)
                sink, bsink = torch.full((co, ci, 3, 3), 0.5, device="cuda").contiguous(memory_format=CL), torch.full((co,), 0.25, device="cuda")
                assert DC.conv3x3_wino_wgrad_gen(x, x2, dz, (co, ci, 3, 3), dw_out=sink, y_out=yo, act=act, db_out=bsink) == (None, None)
                assert _rel(sink - 0.5, w64.grad) < 3e-6 + 1e-6 / float(w64.grad.abs().max()) and _rel(bsink - 0.25, bref) < 1e-5, (act, wgs)
                dw2, none = DC.conv3x3_wino_wgrad_gen(x, x2, dz, (co, ci, 3, 3), y_out=yo, act=act)
                assert none is None and _rel(dw2, w64.grad) < 3e-6
            finally:
                DC._WINO_WGS = old


def test_decoder_weight_gradient_rejects_what_it_does_not_cover():
    from deep_visual_slam_amd import _lib, conv as DC
    x = torch.randn(1, 48, 4, 4, device="cuda").contiguous(memory_format=CL)
    assert not DC.wino_dec_wgrad_eligible((64, 48, 3, 3), x, None)
    with pytest.raises(_lib.DvsError):
        DC.conv3x3_wino_wgrad_gen(x, None, torch.randn(1, 64, 4, 4, device="cuda").contiguous(memory_format=CL), (64, 48, 3, 3))
    x = torch.randn(1, 64, 1, 4, device="cuda").contiguous(memory_format=CL)
    with pytest.raises(_lib.DvsError):          # ReflectionPad2d(1) needs two rows
        DC.conv3x3_wino_wgrad_gen(x, None, torch.randn(1, 64, 1, 4, device="cuda").contiguous(memory_format=CL), (64, 64, 3, 3))
    x = torch.randn(1, 64, 4, 4, device="cuda").contiguous(memory_format=CL)
    with pytest.raises(_lib.DvsError):          # a bias gradient without the activation path
        DC.conv3x3_wino_wgrad_gen(x, None, torch.randn(1, 64, 4, 4, device="cuda").contiguous(memory_format=CL), (64, 64, 3, 3), want_bias=True)


@pytest.mark.parametrize("mode,co,c1,c2", [("skip", 32, 32, 64), ("plain", 32, 64, 0), ("skip", 64, 64, 64), ("plain", 128, 64, 0)])
def test_decoder_layer_autograd_takes_the_winograd_weight_gradient(mode, co, c1, c2, monkeypatch):
    """A decoder ConvBlock through conv.conv2d with the weight gradient on the Winograd gathers: thin layers (32 outputs) with the
    ELU derivative and the bias gradient fused into it, wide ones behind the pre-activation pass; against fp64 autograd."""
    from deep_visual_slam_amd import conv as DC
    g = torch.Generator(device="cuda").manual_seed(13)
    B, h, w = 2, 16, 32
    up = mode != "plain"
    H, W = (2 * h, 2 * w) if up else (h, w)
    x = torch.randn(B, c1, h, w, device="cuda", generator=g).contiguous(memory_format=CL).requires_grad_(True)
    skip = torch.randn(B, c2, H, W, device="cuda", generator=g).contiguous(memory_format=CL).requires_grad_(True) if c2 else None
    wt = (torch.randn(co, c1 + c2, 3, 3, device="cuda", generator=g) * 0.05).contiguous(memory_format=CL).requires_grad_(True)
    bias = (torch.randn(co, device="cuda", generator=g) * 0.1).requires_grad_(True)
    calls = []
    real = DC.conv3x3_wino_wgrad_gen
    monkeypatch.setattr(DC, "conv3x3_wino_wgrad_gen", lambda *a, **k: (calls.append(k.get("act")), real(*a, **k))[1])
    monkeypatch.setattr(DC, "wino_dec_wgrad_pays", lambda *a: True)
    y = DC.conv2d(x, wt, bias, 1, 0, reflect_pad=1, act="elu", x2=skip, upsample=up)
    cot = torch.randn(y.shape, device="cuda", generator=g).contiguous(memory_format=CL)
    ins = [x, wt, bias] + ([skip] if skip is not None else [])
    got = torch.autograd.grad(y, ins, cot)
    assert calls == (["elu"] if co == 32 else [None])          # fused derivative for the thin layer, pre-activation pass for the wide one
    d = [t.detach().double().requires_grad_(True) for t in ins]
    ref = _dec_ref(d[0], d[3] if skip is not None else None, up, d[1], d[2], "elu")
    want = torch.autograd.grad(ref, d, cot.double())
    assert _rel(y, ref.detach()) < TOL
    for a, b in zip(got, want):
        assert _rel(a, b) < 2e-5


@pytest.mark.parametrize("mode", ["plain", "skip", "up"])
def test_decoder_layer_autograd_matches_torch(mode):
    from deep_visual_slam_amd import conv as DC
    g = torch.Generator(device="cuda").manual_seed(9)
    B, c1, co, h, w = 2, 64, 64, 6, 8
    up = mode != "plain"
    c2 = 64 if mode == "skip" else 0
    H, W = (2 * h, 2 * w) if up else (h, w)
    x = torch.randn(B, c1, h, w, device="cuda", generator=g).contiguous(memory_format=CL).requires_grad_(True)
    skip = torch.randn(B, c2, H, W, device="cuda", generator=g).contiguous(memory_format=CL).requires_grad_(True) if c2 else None
    wt = (torch.randn(co, c1 + c2, 3, 3, device="cuda", generator=g) * 0.05).contiguous(memory_format=CL).requires_grad_(True)
    bias = (torch.randn(co, device="cuda", generator=g) * 0.1).requires_grad_(True)
    assert DC.wino_dec_eligible(wt, 1, 1, True, "elu", x, skip if skip is not None else (DC.UPSAMPLE_ONLY if up else None), False, None)
    y = DC.conv2d(x, wt, bias, 1, 0, reflect_pad=1, act="elu", x2=skip, upsample=up)
    cot = torch.randn_like(y)
    ins = [x, wt, bias] + ([skip] if skip is not None else [])
    got = torch.autograd.grad(y, ins, cot)
    d = [t.detach().double().requires_grad_(True) for t in ins]
    ref = _dec_ref(d[0], d[3] if skip is not None else None, up, d[1], d[2], "elu")
    want = torch.autograd.grad(ref, d, cot.double())
    assert _rel(y, ref.detach()) < TOL
    for a, b, tol in zip(got, want, (2e-5, 2e-5, 2e-5, 2e-5)):
        assert _rel(a, b) < tol


@pytest.mark.parametrize("B,ci,co,h,w", [(2, 64, 64, 120, 160), (3, 128, 64, 13, 27), (2, 512, 512, 15, 20)])
def test_residual_in_the_epilogue(B, ci, co, h, w):
    from deep_visual_slam_amd import conv as DC
    x, wt = _mk(B, ci, co, h, w, seed=7)
    r = torch.randn(B, co, h, w, device="cuda").contiguous(memory_format=CL)
    y = DC.conv3x3_wino(x, wt, residual=r)
    assert _rel(y, F.conv2d(x.double(), wt.double(), None, 1, 1) + r.double()) < TOL


def test_identity_passthrough_adds_the_skip_gradient_in_the_data_gradient():
    """conv2d(..., passthrough=True) hands x back as an output of the same autograd node (nn_ops.conv_bn_relu_with_identity):
    the gradient of everything that consumes that alias is added in the data-gradient epilogue, and the total must equal what
    autograd computes for a tensor used twice."""
    from deep_visual_slam_amd import conv as DC
    x, wt = _mk(2, 64, 64, 12, 20, seed=8)
    x.requires_grad_(True)
    wt.requires_grad_(True)
    y, st, xa = DC.conv2d(x, wt, None, 1, 1, want_stats=1, passthrough=True)
    assert xa.data_ptr() == x.data_ptr() and not st.requires_grad
    cot_y, cot_s = torch.randn_like(y), torch.randn_like(x)
    ((y * cot_y).sum() + (torch.tanh(xa) * cot_s).sum()).backward()
    x64, w64 = x.detach().double().requires_grad_(True), wt.detach().double().requires_grad_(True)
    ((F.conv2d(x64, w64, None, 1, 1) * cot_y.double()).sum() + (torch.tanh(x64) * cot_s.double()).sum()).backward()
    assert _rel(x.grad, x64.grad) < TOL and _rel(wt.grad, w64.grad) < 2e-5
    # only the alias is used: the convolution's own branch gets no gradient
    x2 = x.detach().clone().requires_grad_(True)
    _, xa2 = DC.conv2d(x2, wt.detach(), None, 1, 1, passthrough=True)
    (xa2 * cot_s).sum().backward()
    assert torch.equal(x2.grad, cot_s)


@pytest.mark.parametrize("B,c,h,w", [(24, 256, 15, 20), (2, 256, 15, 20), (3, 64, 9, 11)])
def test_bias_relu_layer_autograd_matches_torch(B, c, h, w):
    """PoseNet's decoder convolutions (Conv2d(256, 256, 3, 1, 1) + ReLU, model/posenet_single.py:160-164, 189-197): bias and ReLU
    in the Winograd epilogue, dZ = dY * [Y > 0] and the bias gradient from one pre-activation pass, data and weight gradient on
    the Winograd kernels."""
    from deep_visual_slam_amd import conv as DC
    x, wt = _mk(B, c, c, h, w, seed=5)
    g = torch.Generator(device="cuda").manual_seed(6)
    b = (torch.randn(c, device="cuda", generator=g) * 0.3)
    x.requires_grad_(True); wt.requires_grad_(True); b.requires_grad_(True)
    y = DC.conv2d(x, wt, b, 1, 1, act="relu")
    assert y.grad_fn is not None and y.is_contiguous(memory_format=CL)
    gy = torch.randn(y.shape, device="cuda", generator=g).contiguous(memory_format=CL)
    y.backward(gy)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, wt, b))
    pre = F.conv2d(x64, w64, b64, 1, 1)
    assert _rel(y, F.relu(pre.detach())) < TOL
    # a pre-activation within rounding of zero may fall on the other side of the ReLU (one such element moves the data gradient of
    # its 3 x 3 neighbourhood by |w| |gy|): few of them, and the fp64 backward takes the side the kernel took
    on = y.detach() > 0
    flips = (on != (pre.detach() > 0)).sum().item()
    assert flips <= 1e-5 * y.numel()
    (pre * on.double()).backward(gy.double())
    assert _rel(x.grad, x64.grad) < TOL and _rel(wt.grad, w64.grad) < 2e-5 and _rel(b.grad, b64.grad) < 2e-5


@pytest.mark.parametrize("B,c,h,w,groups", [(4, 64, 60, 80, 1), (4, 64, 60, 80, 2), (2, 128, 13, 27, 1)])
def test_statistics_spread_over_slots(B, c, h, w, groups):
    """dvs_conv3x3_wino_fwd with stat_slots = 16: the workgroups add their BatchNorm statistics into 16 copies of the table (one workgroup per CU
    ends with these atomics; on ONE copy they serialise); the copies add up to the sums, and bn.bn_act consumes the copies."""
    import torch.nn as nn
    from deep_visual_slam_amd import bn as DB, conv as DC
    x, wt = _mk(B, c, c, h, w, seed=9)
    y64 = F.conv2d(x.double(), wt.double(), None, 1, 1)
    st = torch.zeros(16, groups, 2, c, device="cuda")
    y = DC.conv3x3_wino(x, wt, st, groups, stat_slots=16)
    assert _rel(y, y64) < TOL
    if B * h * w >= 4 * 60 * 80:                                    # (small launches take the K split: statistics by a pass of their own, copy 0)
        assert int((st.abs().sum((1, 2, 3)) > 0).sum()) > 1        # more than one copy was used
    parts = y64.chunk(groups, 0)
    ref = torch.stack([torch.stack([p.sum((0, 2, 3)), (p * p).sum((0, 2, 3))]) for p in parts])
    tot = st.double().sum(0)
    assert float((tot - ref).abs().max() / ref.abs().max()) < 2e-5
    # BatchNorm forward from the slotted table == from the summed table
    m1, m2 = nn.BatchNorm2d(c).cuda().train(), nn.BatchNorm2d(c).cuda().train()
    z1 = DB.bn_act(y, m1, st, True, groups=groups)
    z2 = DB.bn_act(y, m2, st.sum(0) if groups > 1 else st.sum(0)[0], True, groups=groups)
    assert float((z1 - z2).abs().max()) < 1e-5
    assert torch.allclose(m1.running_var, m2.running_var, rtol=1e-5, atol=1e-7)
