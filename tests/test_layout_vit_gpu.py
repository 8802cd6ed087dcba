"""The layout contract of the Depth-Anything-V2 training path (depth_anything_v2.py): the autograd Functions _AttentionF,
_LayerNormF, _ActF, _ResizeF, _ShuffleF and linear_train with every tensor argument in every memory layout of the view zoo
(tests/layouts.py) and every cotangent layout -- autograd chooses the cotangent's layout, not the caller, so a Function must
accept all of them.  csrc/vit.hip reads its operands with 16-byte vector loads and checks no alignment itself: the Functions
copy what is not dense or not on a 16-byte boundary (_host.aligned).

The weight and LayerNorm parameter gradients add with float atomics, so nothing here is compared bit for bit: the view run and
the dense run are both judged against the fp64 formulas (torch's own, as in test_dav2_gpu.py) by that file's relmax bounds;
linear_train, a 1x1 convolution, by the convolution tolerances of test_conv_gpu.py (raft_update_ref.check_rel).

The inference helpers of the module are model-internal.  gemm, resize_bilinear_ac and conv_transpose_s accept every layout (they
normalise through conv._nhwc / _host.aligned) and are in the matrix, forward only; layernorm and attention refuse what is not
dense and aligned, by name, before any launch: those cells are test_layouts_cpu.py's REFUSED table."""
import pytest
import torch
import torch.nn.functional as F

import layouts
import raft_update_ref as U
from test_dav2_gpu import TOL, relmax

pytestmark = pytest.mark.gpu

B, N, HEADS, HD = 2, 33, 2, 64
M, C = 7, 64


def _randn(*shape, seed=0, scale=1.0, shift=0.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) + shift


def _relmax_rule(out, grad):
    def judge(what, got, want):
        e, b = relmax(got, want), TOL[out if what.startswith("out") else grad]
        print("%s: relmax %.3e, bound %.1e" % (what, e, b))
        assert torch.isfinite(got).all() and e < b, (what, e, b)
    return judge


def _attention_ref(qkv2d):
    q, k, v = qkv2d.reshape(B, N, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
    return (((q * HD ** -0.5) @ k.transpose(-2, -1)).softmax(-1) @ v).transpose(1, 2).reshape(B * N, HEADS * HD)


def _shuffle_ref(g, k, cout):
    """The scatter half of a stride == kernel ConvTranspose2d: channel (a*k + c)*cout + o of pixel (i, j) -> (o, i*k + a, j*k + c)."""
    Bn, _, h, w = g.shape
    return g.reshape(Bn, k, k, cout, h, w).permute(0, 3, 4, 1, 5, 2).reshape(Bn, cout, h * k, w * k)


def _cases():
    from deep_visual_slam_amd import depth_anything_v2 as D
    cases = {}
    cases["attention"] = layouts.Case(lambda qkv2d: D._AttentionF.apply(qkv2d, B, N, HEADS, HD),
                                      {"qkv2d": _randn(B * N, 3 * HEADS * HD, seed=1, scale=1.2)}, _attention_ref,
                                      _relmax_rule("attention", "attention/grad"), grads=("qkv2d",), exact=False)
    cases["layernorm"] = layouts.Case(
        lambda x2d, weight, bias: D._LayerNormF.apply(x2d, weight, bias, 1e-6),
        {"x2d": _randn(M, C, seed=2, scale=2.0, shift=0.3), "weight": _randn(C, seed=3), "bias": _randn(C, seed=4)},
        lambda x2d, weight, bias: F.layer_norm(x2d, (C,), weight, bias, 1e-6),
        _relmax_rule("layernorm", "layernorm/grad"), grads=("x2d", "weight", "bias"), exact=False)
    for act, fn in (("gelu", F.gelu), ("relu", F.relu)):
        cases["act_" + act] = layouts.Case(lambda x, act=act: D._ActF.apply(x, act), {"x": _randn(M, C, seed=5)}, lambda x, fn=fn: fn(x),
                                           _relmax_rule("act", "act/grad"), grads=("x",), exact=False)
        cases["act_%s_map" % act] = layouts.Case(lambda x, act=act: D._ActF.apply(x, act), {"x": _randn(2, 8, 3, 5, seed=6)}, lambda x, fn=fn: fn(x),
                                                 _relmax_rule("act", "act/grad"), grads=("x",), exact=False)
    cases["resize"] = layouts.Case(lambda x: D._ResizeF.apply(x, 7, 9), {"x": _randn(2, 8, 3, 5, seed=7)},
                                   lambda x: F.interpolate(x, (7, 9), mode="bilinear", align_corners=True),
                                   _relmax_rule("resize", "resize/grad"), grads=("x",), exact=False)

    def same(what, got, want):          # a permutation, forward and backward: test_dav2_gpu compares it with torch.equal
        assert torch.equal(got, want.float()), what
    cases["shuffle"] = layouts.Case(lambda g: D._ShuffleF.apply(g, 2, 8), {"g": _randn(2, 4 * 8, 3, 5, seed=8)},
                                    lambda g: _shuffle_ref(g, 2, 8), same, grads=("g",), exact=False)
    w4 = _randn(16, C, 1, 1, seed=12, scale=C ** -0.5)
    cases["gemm"] = layouts.Case(
        lambda x2d, w4d, bias, residual: D.gemm(x2d, w4d, bias, residual=residual),
        {"x2d": _randn(M, C, seed=13), "w4d": w4, "bias": _randn(16, seed=14, scale=0.1), "residual": _randn(M, 16, seed=15)},
        lambda x2d, w4d, bias, residual: F.linear(x2d, w4d[:, :, 0, 0], bias) + residual,
        lambda what, got, want: _relmax_rule("gemm", "gemm")(what, got, want), exact=False)
    cases["resize_bilinear_ac"] = layouts.Case(lambda x: D.resize_bilinear_ac(x, 7, 9), {"x": _randn(2, 8, 3, 5, seed=7)},
                                               lambda x: F.interpolate(x, (7, 9), mode="bilinear", align_corners=True),
                                               _relmax_rule("resize", "resize"), exact=False)
    wt = _randn(16, 8, 2, 2, seed=16, scale=0.1)                    # ConvTranspose2d(16, 8, 2, stride=2)
    cases["conv_transpose_s"] = layouts.Case(
        lambda x, w_gemm, bias_rep: D.conv_transpose_s(x, w_gemm, bias_rep, 2, 8),
        {"x": _randn(2, 16, 3, 5, seed=17), "w_gemm": wt.permute(2, 3, 1, 0).reshape(2 * 2 * 8, 16, 1, 1).contiguous(),
         "bias_rep": _randn(8, seed=18).repeat(4)},
        lambda x, w_gemm, bias_rep: F.conv_transpose2d(x, w_gemm.reshape(2, 2, 8, 16).permute(3, 2, 0, 1), bias_rep[:8], stride=2),
        _relmax_rule("gemm", "gemm"), exact=False)
    cases["linear_train"] = layouts.Case(
        lambda x2d, weight, bias: D.linear_train(x2d, weight, bias),
        {"x2d": _randn(M, C, seed=9), "weight": _randn(16, C, seed=10, scale=C ** -0.5), "bias": _randn(16, seed=11, scale=0.1)},
        lambda x2d, weight, bias: F.linear(x2d, weight, bias), lambda what, got, want: U.check_rel(what.replace("d_", "d/"), got, want), grads=("x2d", "weight", "bias"), exact=False)
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


@pytest.mark.parametrize("case,arg,kind", layouts.input_cells(cases()))
def test_an_argument_in_any_layout_gives_the_dense_result(gpu_device, case, arg, kind):
    cases()[case].check_input(gpu_device, arg, kind)


@pytest.mark.parametrize("case,kind", layouts.cotangent_cells(cases()))
def test_a_cotangent_in_any_layout_gives_the_dense_gradients(gpu_device, case, kind):
    cases()[case].check_cotangent(gpu_device, kind)


@pytest.mark.parametrize("case", list(cases()))
def test_all_arguments_as_views_at_once(gpu_device, case):
    cases()[case].check_all_at_once(gpu_device)


# ---- the whole model: the input images as views -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["crop", "cl"])
def test_depth_anything_reads_image_views_as_it_reads_dense_images(gpu_device, kind):
    """DepthAnythingV2 (ViT-S) at 28x42 with test_dav2_gpu's seeded weights: images handed in as a crop of a padded frame and in
    channels_last memory give the dense-input depth within the model's rel-L2 tolerance (test_dav2_gpu.TOL["model"])."""
    from deep_visual_slam_amd.depth_anything_v2 import DepthAnythingV2
    from oracle.depth_anything import seeded_weights
    from test_dav2_gpu import rel
    net = DepthAnythingV2(encoder="vits", features=64, out_channels=[48, 96, 192, 384]).eval()
    net.pretrained.load_state_dict(seeded_weights(net.pretrained.state_dict(), seed=0))
    net.depth_head.load_state_dict(seeded_weights(net.depth_head.state_dict(), seed=4))
    net = net.to(gpu_device)
    view = layouts.make(_randn(2, 3, 28, 42, seed=21).to(gpu_device), kind)
    with torch.no_grad():
        got, want = net(view), net(layouts.dense(view))
    assert got.shape == want.shape == (2, 28, 42) and bool(torch.isfinite(got).all()) and float(want.abs().max()) > 0
    assert rel(got, want.cpu()) < TOL["model"]
