"""Inference conv epilogues against fp64: folded-BatchNorm bias, BasicBlock identity and ReLU, one case per launch regime.

A. conv.conv2d_forward(x, w, bias, ..., act="relu", residual=...) -- what nn_ops.conv_bn_act calls under eval() + no_grad --
   on every row of tests/infer_cases.py: split-K with the finish kernel, the in-kernel epilogue of the LDS-DMA and of the
   register-staged kernel, the stem on the generic planar kernel; fp32, fp32 deterministic (never splits) and the bf16 mode.
   Reference: act(conv + bias + residual) in fp64 on the CPU.  Operands sit between guard bands (tests/guard.py), the output and
   every workspace the call allocates too.  Tolerance: 2e-5 of the tensor's max-abs (TOL of tests/test_conv_sequences_gpu.py);
   in the bf16 mode against fp64 on bf16-rounded x and w.  ReLU is continuous: no element is exempt.
B. nn_ops.conv_bn_act on one BasicBlock group in its three modes (fold, eval() with autograd, and the two against each other),
   with the gradients of the eval()-with-autograd path (bn._AffineAct) against fp64 autograd.
"""
import pytest
import torch
import torch.nn.functional as F

import guard
import infer_cases as IC
from test_guard_kernels_gpu import _cl, bf16_mode, r16, relmax  # noqa: F401  (bf16_mode is a fixture)

pytestmark = pytest.mark.gpu
CL = torch.channels_last
TOL = 2e-5                      # tests/test_conv_sequences_gpu.py TOL["fp32"][0] == TOL["bf16"][0]

_conv64 = {}                    # (row id, bf16) -> fp64 convolution of the row's seeded operands, computed once


def _reference(row, combo, bf16=False):
    x, w, b, r, norm = IC.inputs(row, dyadic=bf16)
    key = (row.id, bf16)
    if key not in _conv64:
        _conv64[key] = IC.conv_reference(row, x, w, norm, r16 if bf16 else None)
    return IC.epilogue(_conv64[key], b, r, combo)


def _place(dev, row, bf16=False):
    """The row's operands on the GPU between NaN bands, in the layouts the kernels take without a copy."""
    x, w, b, r, norm = IC.inputs(row, dyadic=bf16)
    g = guard.Bands(dev)
    gx, gw = (g.place(x), g.place(w)) if row.planar else (_cl(g, x), _cl(g, w))
    gnorm = tuple(g.place(t) for t in norm) if norm is not None else (None, None)
    return g, (gx, gw, g.place(b), _cl(g, r), gnorm)


def _forward(row, ops, combo):
    from deep_visual_slam_amd import conv as DC
    gx, gw, gb, gr, (sc, sh) = ops
    has_b, has_r, relu = combo
    return DC.conv2d_forward(gx, gw, gb if has_b else None, row.s, IC.pad(row), act="relu" if relu else None, in_scale=sc,
                             in_shift=sh, nchw_planar=row.planar, residual=gr if has_r else None)


def _guarded_forward(dev, row, combo, bf16=False):
    from deep_visual_slam_amd import conv as DC, zeropool
    g, ops = _place(dev, row, bf16)
    with guard.allocations(DC, zeropool) as rec:
        y = _forward(row, ops, combo)
        torch.cuda.synchronize()
    assert rec.count >= 1, rec.count                      # the output: the zero and finish kernels write M * Cout / 4 vectors
    g.check()
    return y


@pytest.fixture
def deterministic_mode():
    from deep_visual_slam_amd import _lib
    old = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(old)


CASES = [(r, c) for r in IC.ROWS for c in IC.combos(r)]
CASE_IDS = ["%s-%s" % (r.id, IC.combo_id(c)) for r, c in CASES]
CASES16 = [(r, c) for r, c in CASES if r.bf16]
CASE16_IDS = ["%s-%s" % (r.id, IC.combo_id(c)) for r, c in CASES16]


def _check(y, ref, what):
    err = relmax(y, ref)
    print("%s: max error %.2e of the tensor's max-abs (bound %.0e)" % (what, err, TOL))
    assert err < TOL, (what, err)


@pytest.mark.parametrize("row,combo", CASES, ids=CASE_IDS)
def test_epilogue_fp32(gpu_device, row, combo):
    """The launch the product gets: rows that split K run splitk_zero_kernel -> atomics -> splitk_finish_kernel."""
    _check(_guarded_forward(gpu_device, row, combo), _reference(row, combo), row.id)


@pytest.mark.parametrize("row,combo", CASES, ids=CASE_IDS)
def test_epilogue_fp32_deterministic(gpu_device, deterministic_mode, row, combo):
    """The deterministic mode never splits K: every shape also runs the in-kernel epilogue (conv_epilogue_body with its
    residual loads from clamped addresses; n_ok / nc at Cout = 96 and 36)."""
    _check(_guarded_forward(gpu_device, row, combo), _reference(row, combo), row.id)


@pytest.mark.parametrize("row,combo", CASES16, ids=CASE16_IDS)
def test_epilogue_bf16(gpu_device, bf16_mode, row, combo):
    """launch_buf<..., BF16>: bf16 tiles, fp32 accumulation and epilogue.  Specification: fp64 on bf16-rounded x and w (the
    stem: on the bf16-rounded normalised image); bias and residual are not rounded."""
    _check(_guarded_forward(gpu_device, row, combo, bf16=True), _reference(row, combo, bf16=True), row.id)


@pytest.mark.parametrize("row", IC.ROWS, ids=[r.id for r in IC.ROWS])
def test_rows_run_the_regime_they_name(gpu_device, row):
    """Each fp32 row once with the deterministic mode off and once on.  dvs_conv2d_fwd consults the mode in one place only --
    launch_dma's decision to split K (a launch with a statistics epilogue aside, which these are not) -- so the two runs
    of a row that does not split launch the same kernel on the same grid and must agree bit for bit, and a row that splits
    sums its K >= 64 products in another order (partial sums per channel block, added by atomics) and must differ in at
    least one of its >= 1 000 elements.  A retuned threshold that moved a row out of its regime fails here."""
    from deep_visual_slam_amd import _lib
    _, ops = _place(gpu_device, row)
    split = IC.regime(row)[3] > 1
    assert split == (row.ksplit > 1) and IC.regime(row, deterministic=True)[3] == 1
    old = _lib.deterministic()
    try:
        _lib.set_deterministic(False)
        y0 = _forward(row, ops, row.combo).clone()
        _lib.set_deterministic(True)
        y1 = _forward(row, ops, row.combo).clone()
    finally:
        _lib.set_deterministic(old)
    torch.cuda.synchronize()
    assert y0.numel() >= 1000
    differ = int((y0 != y1).sum())
    print("%s: %d of %d elements differ between the modes" % (row.id, differ, y0.numel()))
    assert (differ > 0) == split, (row.id, "expected split-K" if split else "expected no split", differ)
    assert relmax(y1, y0) < TOL


@pytest.mark.parametrize("rid", ["l1_split2", "l4_split16_b3"])
def test_splitk_graph_replay(gpu_device, rid):
    """Zero -> accumulate -> finish inside a captured graph (the warm-up pattern of inference.Graphed): three replays with
    fresh x and residual copied into the static buffers, each against fp64.  A zero fill that a replay does not order in front
    of the atomics, or a finish that runs early, leaves the previous replay's values in y."""
    row = IC.BY_ID[rid]
    assert IC.regime(row)[3] > 1
    x, w, b, r, norm = IC.inputs(row)
    dev = gpu_device
    sx, sr = (torch.zeros_like(t).contiguous(memory_format=CL).to(dev) for t in (x, r))
    ops = (sx, w.contiguous(memory_format=CL).to(dev), b.to(dev), sr, (None, None))
    assert sx.is_contiguous(memory_format=CL) and sr.is_contiguous(memory_format=CL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            _forward(row, ops, (1, 1, 1))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        y = _forward(row, ops, (1, 1, 1))
    gen = torch.Generator().manual_seed(77)
    for i in range(3):
        xi, ri = torch.randn(x.shape, generator=gen), torch.randn(r.shape, generator=gen)
        sx.copy_(xi.to(dev))
        sr.copy_(ri.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        _check(y, IC.reference(row, xi, w, b, ri, None, (1, 1, 1)), "%s replay %d" % (rid, i))


# ---- B. one BasicBlock group: conv -> BatchNorm (eval) -> (+ identity | + downsample branch) -> ReLU -----------------------------
FWD_TOL = 5e-5                  # tests/test_bn_gpu.py's forward bound; the fold moves where the scale is rounded
GRAD_TOL = 1e-4                 # the project's fp32 gradient tolerance (tests/test_conv_sequences_gpu.py TOL["fp32"][1])
NEAR_ZERO = 1e-4                # cotangent zeroed where the fp64 pre-activation is within this share of its max-abs of 0
EPS = 1e-5


def _bn_params(C, gen):
    """Running statistics and affine parameters as tests/test_inference_gpu.py's _randomise_bn draws them."""
    return dict(rm=torch.randn(C, generator=gen) * 0.2, rv=torch.rand(C, generator=gen) * 1.5 + 0.25,
                gamma=torch.rand(C, generator=gen) + 0.5, beta=torch.randn(C, generator=gen) * 0.1)


def _block_inputs(blk, B):
    gen = torch.Generator().manual_seed(100 * B + IC.BLOCKS.index(blk))
    t = dict(x=torch.randn(B, blk.ci, blk.H, blk.W, generator=gen),
             w=torch.randn(blk.co, blk.ci, 3, 3, generator=gen) * (2.0 / (blk.ci * 9)) ** 0.5, bn=_bn_params(blk.co, gen))
    Ho, Wo = (blk.H - 1) // blk.s + 1, (blk.W - 1) // blk.s + 1
    if blk.res_bn:
        t.update(res=torch.randn(B, blk.ci, blk.H, blk.W, generator=gen),
                 wd=torch.randn(blk.co, blk.ci, 1, 1, generator=gen) * (2.0 / blk.ci) ** 0.5, bnd=_bn_params(blk.co, gen))
    elif blk.residual:
        t["res"] = torch.randn(B, blk.co, Ho, Wo, generator=gen)
    t["cot"] = torch.randn(B, blk.co, Ho, Wo, generator=gen)
    return t


GRAD_NAMES = ("x", "w", "gamma", "beta", "res", "wd", "gamma_d", "beta_d")


def _block_torch(blk, t, dtype, cot=None):
    """The group composed from torch's own operators on the CPU in `dtype`: (z, pre-activation u, {name: gradient})."""
    c = lambda v: v.to(dtype).clone().requires_grad_(True)
    leaves = dict(x=c(t["x"]), w=c(t["w"]), gamma=c(t["bn"]["gamma"]), beta=c(t["bn"]["beta"]))
    bn = t["bn"]
    u = F.batch_norm(F.conv2d(leaves["x"], leaves["w"], None, blk.s, 1), bn["rm"].to(dtype), bn["rv"].to(dtype), leaves["gamma"],
                     leaves["beta"], False, 0.0, EPS)
    if "res" in t:
        leaves["res"] = c(t["res"])
        idn = leaves["res"]
        if blk.res_bn:
            leaves.update(wd=c(t["wd"]), gamma_d=c(t["bnd"]["gamma"]), beta_d=c(t["bnd"]["beta"]))
            bd = t["bnd"]
            idn = F.batch_norm(F.conv2d(idn, leaves["wd"], None, blk.s, 0), bd["rm"].to(dtype), bd["rv"].to(dtype), leaves["gamma_d"],
                               leaves["beta_d"], False, 0.0, EPS)
        u = u + idn
    z = F.relu(u) if blk.relu else u
    grads = {}
    if cot is not None:
        names = [n for n in GRAD_NAMES if n in leaves]
        grads = dict(zip(names, torch.autograd.grad(z, [leaves[n] for n in names], cot.to(dtype))))
    return z.detach(), u.detach(), grads


def _gpu_bn(p, dev):
    bn = torch.nn.BatchNorm2d(p["rm"].numel(), eps=EPS)
    bn.running_mean.copy_(p["rm"])
    bn.running_var.copy_(p["rv"])
    bn.weight.data.copy_(p["gamma"])
    bn.bias.data.copy_(p["beta"])
    return bn.to(dev).eval()


def _buffers(*bns):
    return [b.detach().clone() for bn in bns if bn is not None for b in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]


def _block_gpu(blk, t, dev, grad, cot=None):
    """nn_ops.conv_bn_act on the GPU, eval() mode: (z, {name: gradient}); grad False: under no_grad (the fold)."""
    from deep_visual_slam_amd import gradsink, nn_ops
    p = lambda v: v.contiguous(memory_format=CL).to(dev).requires_grad_(True) if v.dim() == 4 else v.to(dev).requires_grad_(True)
    x, w, bn = p(t["x"]), p(t["w"]), _gpu_bn(t["bn"], dev)
    leaves = dict(x=x, w=w, gamma=bn.weight, beta=bn.bias)
    res = wd = bnd = None
    if "res" in t:
        res = leaves["res"] = p(t["res"])
        if blk.res_bn:
            wd, bnd = p(t["wd"]), _gpu_bn(t["bnd"], dev)
            leaves.update(wd=wd, gamma_d=bnd.weight, beta_d=bnd.bias)
    before = _buffers(bn, bnd)
    with torch.set_grad_enabled(grad):
        z = nn_ops.conv_bn_act(x, w, bn, blk.s, 1, blk.relu, res, (wd, bnd, blk.s) if blk.res_bn else None)
    assert z.requires_grad == grad
    grads = {}
    if cot is not None:
        names = [n for n in GRAD_NAMES if n in leaves]
        grads = dict(zip(names, torch.autograd.grad(z, [leaves[n] for n in names], cot.contiguous(memory_format=CL).to(dev))))
        gradsink.join()
    torch.cuda.synchronize()
    for a, b in zip(before, _buffers(bn, bnd)):            # eval mode: running statistics and the step counter bit-identical
        assert a.dtype == b.dtype and torch.equal(a, b)
    return z.detach(), grads


BLOCK_CASES = [(blk, B) for blk in IC.BLOCKS for B in (1, 3)]
BLOCK_IDS = ["%s-b%d" % (blk.id, B) for blk, B in BLOCK_CASES]


@pytest.mark.parametrize("blk,B", BLOCK_CASES, ids=BLOCK_IDS)
def test_block_forward_fold_and_affine(gpu_device, blk, B):
    """eval() + no_grad (BatchNorm folded into the weights, bias + identity + ReLU in the conv epilogue) and eval() with autograd
    (bn.affine_act behind the convolution): each within 5e-5 of the tensor's max-abs of fp64 F.batch_norm(training=False)
    around F.conv2d, and of each other; the BatchNorm buffers bit-identical afterwards."""
    t = _block_inputs(blk, B)
    z64, _, _ = _block_torch(blk, t, torch.float64)
    zf, _ = _block_gpu(blk, t, gpu_device, grad=False)
    za, _ = _block_gpu(blk, t, gpu_device, grad=True)
    errs = relmax(zf, z64), relmax(za, z64), relmax(za, zf)
    print("%s b%d: fold %.2e, affine_act %.2e, one against the other %.2e (bound %.0e)" % ((blk.id, B) + errs + (FWD_TOL,)))
    assert max(errs) < FWD_TOL, errs


@pytest.mark.parametrize("blk,B", BLOCK_CASES, ids=BLOCK_IDS)
def test_block_gradients_eval_with_autograd(gpu_device, blk, B):
    """Gradients of the eval()-with-autograd path (bn._AffineAct: dvs_bn_bwd_reduce / dvs_bn_bwd_apply with (mean, invstd) =
    (0, 1), and the convolutions' backward behind it) against fp64 autograd: dx, dw, d gamma, d beta, d residual, and for the
    downsample branch d wd, d gamma_d, d beta_d.

    ReLU's derivative jumps at 0, so the cotangent is zero wherever the fp64 pre-activation u has |u| < 1e-4 max|u|: a branch
    that rounding flips contributes nothing.  The masked share must stay <= 0.5 %.  Bound per tensor, relative to its max-abs:
    the larger of 1e-4 and 3 x the error of the same composition run by torch in fp32 on the CPU; both are computed here and
    printed with the GPU's error.

    Measured on the MI355X, worst tensor of each case (masked share; GPU error; fp32 CPU yardstick) -- 3 x the yardstick stays
    below 1e-4 everywhere, so every bound is 1e-4:
        plain    b1  0.072 %  4.0e-07  2.2e-07      plain    b3  0.063 %  4.3e-07  8.0e-07
        residual b1  0.039 %  2.8e-07  2.4e-07      residual b3  0.043 %  3.6e-07  2.3e-07   (d residual: 0 on both, the cotangent itself)
        res_bn   b1  0.037 %  5.9e-07  3.6e-07      res_bn   b3  0.070 %  5.4e-07  6.2e-07
        norelu   b1  none     4.0e-07  5.2e-07      norelu   b3  none     4.3e-07  1.2e-06   (no ReLU: nothing is masked)"""
    t = _block_inputs(blk, B)
    _, u64, _ = _block_torch(blk, t, torch.float64)
    cot, share = t["cot"], 0.0
    if blk.relu:
        near = u64.abs() < NEAR_ZERO * u64.abs().max()
        share = float(near.double().mean())
        cot = torch.where(near, torch.zeros_like(cot), cot)
    assert share <= 5e-3, share
    _, _, g64 = _block_torch(blk, t, torch.float64, cot)
    _, _, g32 = _block_torch(blk, t, torch.float32, cot)
    _, got = _block_gpu(blk, t, gpu_device, grad=True, cot=cot)
    assert set(got) == set(g64) and len(got) == (8 if blk.res_bn else 5 if blk.residual else 4)
    bad = []
    for n in g64:
        yard = relmax(g32[n], g64[n])
        bound = max(GRAD_TOL, 3.0 * yard)
        err = relmax(got[n], g64[n])
        print("%s b%d d%-8s GPU %.2e  fp32 CPU %.2e  bound %.2e  (masked cotangent share %.3f %%)" % (blk.id, B, n, err, yard, bound, 100 * share))
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("B,cin,H,W", IC.STEMS)
def test_stem_fold_and_pool(gpu_device, B, cin, H, W):
    """nn_ops.stem_conv_bn_relu_pool under eval() + no_grad: conv1 on the generic planar kernel with the input normalisation, the
    folded bias and the ReLU, then the pool -- against fp64 (z, max_pool2d(z, 3, 2, 1))."""
    from deep_visual_slam_amd import nn_ops
    gen = torch.Generator().manual_seed(B * H)
    x = torch.rand(B, cin, H, W, generator=gen)
    w = torch.randn(64, cin, 7, 7, generator=gen) * (2.0 / (cin * 49)) ** 0.5
    p = _bn_params(64, gen)
    z64 = F.relu(F.batch_norm(F.conv2d((x.double() - 0.45) / 0.225, w.double(), None, 2, 3), p["rm"].double(), p["rv"].double(),
                              p["gamma"].double(), p["beta"].double(), False, 0.0, EPS))
    p64 = F.max_pool2d(z64, 3, 2, 1)
    dev = gpu_device
    bn = _gpu_bn(p, dev)
    before = _buffers(bn)
    norm = (torch.full((cin,), 1.0 / 0.225, device=dev), torch.full((cin,), -0.45 / 0.225, device=dev))
    with torch.no_grad():
        z, pooled = nn_ops.stem_conv_bn_relu_pool(x.to(dev), w.to(dev), bn, norm)
    torch.cuda.synchronize()
    errs = relmax(z, z64), relmax(pooled, p64)
    print("stem %s: z %.2e, pool %.2e (bound %.0e)" % ((B, cin, H, W), errs[0], errs[1], FWD_TOL))
    assert max(errs) < FWD_TOL, errs
    assert all(torch.equal(a, b) for a, b in zip(before, _buffers(bn)))
