"""Training-mode BatchNorm2d (+ residual, + ReLU) on NHWC activations over dvs_bn_* of libdvslam_hip.so.

The batch statistics arrive from the producing convolution's epilogue (`stats` = per-channel sum and
sum of squares), so nn.BatchNorm2d + add + ReLU of a torchvision BasicBlock tail is one HBM pass forward
and two backward (model/resnet_encoder.py:100-111 through torchvision's BasicBlock).
"""
import os

import torch

from . import _lib, gradsink, zeropool
from ._host import aligned
from ._lib import check, ptr

# DVS_BN_BWD_FUSED=1: reduce + apply without the partial-row sum kernel (dvs_bn_bwd).  Measured SLOWER over the step (26.96 -> 27.07 ms):
# the deep layers' tables are large next to their data (C = 512: 450 workgroups x 1 024 float atomics, then 128 KB of copies read by
# every workgroup of the apply pass: +12 us on each 11 us kernel), only the 64-channel layers break even -- so it stays off; the stem
# tail (C = 64, 10^6 rows) always uses the slot table.
_BWD_FUSED = os.environ.get("DVS_BN_BWD_FUSED", "0") == "1"
_YMASK = os.environ.get("DVS_BN_YMASK", "1") != "0"     # ReLU mask of residual-free BatchNorms recomputed from y in the backward

CL = torch.channels_last


def _nn_generation_bump():
    from . import nn_ops
    nn_ops.bump_generation()


def _cl(t):
    """t in channels-last (NHWC) memory on a 16-byte boundary (the kernels read C/4 vectors); a copy only when it is not there
    already."""
    return aligned(t, CL)


def _dp(t):
    """Device pointer of an NHWC tensor, or NULL for None (_lib.ptr insists on the default memory format)."""
    return t.data_ptr() if t is not None else None


def _running_args(bn):
    """(running_mean, running_var, momentum, eps, num_batches_tracked) for the kernels that update bn's running statistics through
    raw pointers, as one forward call of nn.BatchNorm2d in training mode would; the tensors are None when bn does not track them."""
    train_stats = bn.training and bn.track_running_stats
    nbt = bn.num_batches_tracked if train_stats else None
    if nbt is not None and (nbt.dtype != torch.int64 or not nbt.is_cuda):
        raise _lib.DvsError("bn: num_batches_tracked must be an int64 GPU tensor")
    if train_stats:
        _nn_generation_bump()
    return (bn.running_mean if train_stats else None, bn.running_var if train_stats else None,
            bn.momentum if bn.momentum is not None else 0.1, bn.eps, nbt)


def _sinks(gamma, beta):
    """The gradient sinks of an affine pair -- (d gamma, d beta) accumulators, or (None, None) unless both parameters have one --
    with the current stream noted as their writer."""
    gs, bs = gradsink.target(gamma), gradsink.target(beta)
    for par in (gamma, beta):
        gradsink.note(par, gradsink.cur_stream())
    return (gs, bs) if gs is not None and bs is not None else (None, None)


def _param_grads(sums):
    """(d gamma, d beta) from sums [G][2][C] = per-group sum(du), sum(du * xhat)."""
    return (sums[0, 1], sums[0, 0]) if sums.shape[0] == 1 else (sums[:, 1].sum(0), sums[:, 0].sum(0))


def _finalize_groups(stats, count, bn, groups):
    """stats [G][2][C] (sum, sum of squares per sub-batch) -> [G][4][C] = scale, shift, mean, invstd, one launch;
    running statistics and num_batches_tracked are updated as G successive forward calls of nn.BatchNorm2d in
    training mode would have done."""
    C = stats.shape[-1]
    slots = stats.shape[0] if stats.dim() == 4 else 1        # [slots][G][2][C]: copies the Winograd forward spread its atomics over
    out = torch.empty(groups, 4, C, device=stats.device, dtype=torch.float32)
    rmean, rvar, momentum, eps, nbt = _running_args(bn)
    check(_lib.lib().dvs_bn_finalize(stats.data_ptr(), slots, float(count), ptr(bn.weight), ptr(bn.bias), ptr(rmean), ptr(rvar),
                                     float(momentum), float(eps), out[0, 0].data_ptr(), out[0, 1].data_ptr(), out[0, 2].data_ptr(),
                                     out[0, 3].data_ptr(), C, _dp(nbt), groups, _lib.stream()), "dvs_bn_finalize")
    return out


def _bwd_branch(g, z, y, fin, ymask, gamma, du, dy, sums, ws, sinks, M, G, fused):
    """The backward of one BatchNorm, reduce then apply: dy = the gradient of its input y from g, the gradient of its output
    masked by [z > 0] (z None: by the mask recomputed from y and fin when `ymask`, else not at all); du (None = not needed) receives
    the masked g.  sums [G][2][C] ends up as (d beta, d gamma) unless they went to `sinks`.  ws = the partial-row workspace, or,
    `fused`, the zero-filled slot table of dvs_bn_bwd (no partial-row sum kernel between the two passes)."""
    l, st, C = _lib.lib(), _lib.stream(), y.shape[1]
    gs, bs = sinks
    if fused:
        check(l.dvs_bn_bwd(g.data_ptr(), _dp(z), y.data_ptr(), fin.data_ptr(), int(ymask), ptr(gamma), _dp(du), dy.data_ptr(),
                           ws.data_ptr(), None if gs is not None else sums.data_ptr(), M, C, ptr(gs), ptr(bs), G, st), "dvs_bn_bwd")
        return
    check(l.dvs_bn_bwd_reduce(g.data_ptr(), _dp(z), y.data_ptr(), fin.data_ptr(), int(ymask), _dp(du), sums.data_ptr(), ptr(ws),
                              M, C, G, st), "dvs_bn_bwd_reduce")
    check(l.dvs_bn_bwd_apply((du if du is not None else g).data_ptr(), y.data_ptr(), fin.data_ptr(), int(ymask), ptr(gamma),
                             sums.data_ptr(), dy.data_ptr(), M, C, ptr(gs), ptr(bs), G, st), "dvs_bn_bwd_apply")


class _BNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, gamma, beta, residual, res_gamma, res_beta, stat_args, res_fin, relu, groups):
        """z = act(bn(y) [+ residual | + bn_r(residual)]) in ONE launch: stat_args = (stats [G][2][C] from the conv
        epilogue, count, running_mean, running_var, momentum, eps, num_batches_tracked); scale / shift are derived in
        the kernel, which also leaves fin = [G][scale, shift, mean, invstd] for the backward and updates the running
        statistics.  res_fin = the downsample branch's own table.  With G = 2 the first and the second half of the
        batch are normalised with their own statistics."""
        B, C, H, W = y.shape
        M = B * H * W // groups                       # rows per group
        z = torch.empty_like(y)
        stats, count, rmean, rvar, momentum, eps, nbt = stat_args
        slots = stats.shape[0] if stats.dim() == 4 else 1    # [slots][G][2][C] from the Winograd forward: added up in the kernel
        fin = torch.empty(groups, 4, C, device=y.device, dtype=torch.float32)
        # group g = rows [g M, (g + 1) M) with row g of the [G][.][C] tables
        check(_lib.lib().dvs_bn_fwd(y.data_ptr(), stats.data_ptr(), slots, float(count), ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar),
                                    float(momentum), float(eps), _dp(nbt), fin.data_ptr(), _dp(residual),
                                    res_fin[0, 0].data_ptr() if res_fin is not None else None,
                                    res_fin[0, 1].data_ptr() if res_fin is not None else None,
                                    z.data_ptr(), M, C, int(relu), groups, _lib.stream()), "dvs_bn_fwd")
        ctx.relu, ctx.groups = relu, groups
        ctx.affine = (gamma, beta, res_gamma, res_beta)          # only to find their gradient sinks in backward
        # ReLU without a residual: the backward recomputes the mask from y (the y-mask form) and does not need z
        ctx.ymask = bool(relu) and residual is None and _YMASK
        ctx.save_for_backward(y, gamma, residual, res_gamma, fin, res_fin, z if relu and not ctx.ymask else None)
        return z

    @staticmethod
    def backward(ctx, dz):
        y, gamma, residual, res_gamma, fin, res_fin, z = ctx.saved_tensors        # z: only where it is the mask
        l = _lib.lib()
        G = ctx.groups
        B, C, H, W = y.shape
        M = B * H * W // G
        dz = _cl(dz)
        fused = not _lib.deterministic() and _BWD_FUSED      # dvs_bn_bwd: no partial-row sum kernel between the two passes
        pooled = gamma.is_leaf and gamma.grad is not None
        # du = the masked gradient as a tensor: what a residual receives, and what the apply pass re-reads after a z mask
        du = torch.empty_like(y) if (ctx.relu or residual is not None) and not ctx.ymask else None
        dy = torch.empty_like(y)
        ws = None if fused else torch.empty(l.dvs_bn_bwd_workspace(M, C, G) // 4, device=y.device, dtype=torch.float32)

        def buffers():      # (sums, workspace) of one branch; fused: sums are written, not added to, and the slot table is zero-filled
            if fused:
                return (torch.empty((G, 2, C), device=y.device, dtype=torch.float32),
                        zeropool.zeros((l.dvs_bn_bwd_slot_floats(C, G),), y.device))
            return zeropool.zeros((G, 2, C), y.device, pooled=pooled), ws

        g_par, b_par, rg_par, rb_par = ctx.affine
        sums, work = buffers()
        sinks = _sinks(g_par, b_par)
        _bwd_branch(dz, z, y, fin, ctx.ymask, gamma, du, dy, sums, work, sinks, M, G, fused)
        d_gamma, d_beta = (None, None) if sinks[0] is not None else _param_grads(sums)
        d_res, d_rg, d_rb = (du if residual is not None else None), None, None
        if residual is not None and res_fin is not None:              # the downsample branch's own BatchNorm
            d_res = torch.empty_like(residual)
            rsums, work = buffers()
            rsinks = _sinks(rg_par, rb_par)
            _bwd_branch(du, None, residual, res_fin, False, res_gamma, None, d_res, rsums, work, rsinks, M, G, fused)
            if rsinks[0] is None:
                d_rg, d_rb = _param_grads(rsums)
        return dy, d_gamma, d_beta, d_res, d_rg, d_rb, None, None, None, None


class _BNReluPool(torch.autograd.Function):
    """(maxpool3x3s2(z) [, z]) with z = relu(bn(y)) -- the stem tail of model/resnet_encoder.py:102-104 (bn1, relu, maxpool) in
    one forward pass over y (dvs_bn_relu_maxpool_fwd; z is only written when a caller reads it: DepthNet's finest skip) and two
    backward passes (dvs_bn_relu_maxpool_bwd) that gather the pool gradient instead of reading a materialised dz."""

    @staticmethod
    def forward(ctx, y, gamma, beta, fin, groups, need_z):
        B, C, H, W = y.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        pooled = torch.empty((B, C, Ho, Wo), device=y.device, dtype=torch.float32, memory_format=CL)
        idx = torch.empty((B, Ho, Wo, C), device=y.device, dtype=torch.uint8)
        z = torch.empty_like(y) if need_z else None
        check(_lib.lib().dvs_bn_relu_maxpool_fwd(y.data_ptr(), fin.data_ptr(), _dp(z), pooled.data_ptr(), idx.data_ptr(), B, H, W, C,
                                                 groups, _lib.stream()), "dvs_bn_relu_maxpool_fwd")
        ctx.groups = groups
        ctx.affine = (gamma, beta)               # only to find their gradient sinks in backward
        ctx.save_for_backward(y, gamma, fin, idx)
        ctx.set_materialize_grads(False)
        return (pooled, z) if need_z else pooled

    @staticmethod
    def backward(ctx, dpool, dz=None):
        if dpool is None and dz is None:
            return None, None, None, None, None, None
        y, gamma, fin, idx = ctx.saved_tensors
        l = _lib.lib()
        G = ctx.groups
        B, C, H, W = y.shape
        if dpool is None:
            dpool = zeropool.zeros((B, idx.shape[1], idx.shape[2], C), y.device).permute(0, 3, 1, 2)
        dpool = _cl(dpool)
        if dz is not None:
            dz = _cl(dz)
        dy = torch.empty_like(y)
        sums = torch.empty((G, 2, C), device=y.device, dtype=torch.float32)
        ws = zeropool.zeros((l.dvs_bn_bwd_slot_floats(C, G),), y.device)      # the slot table of dvs_bn_bwd
        gs, bs = _sinks(*ctx.affine)
        check(l.dvs_bn_relu_maxpool_bwd(dpool.data_ptr(), idx.data_ptr(), _dp(dz), y.data_ptr(), fin.data_ptr(), ptr(gamma),
                                        sums.data_ptr(), ptr(ws), dy.data_ptr(), B, H, W, C, ptr(gs), ptr(bs), G, _lib.stream()),
              "dvs_bn_relu_maxpool_bwd")
        d_gamma, d_beta = (None, None) if gs is not None else _param_grads(sums)
        return dy, d_gamma, d_beta, None, None, None


def bn_relu_pool(y, bn, stats, groups=1, need_z=True):
    """(z or None, maxpool3x3s2(z)) with z = relu(bn(y)), training-mode BatchNorm with the batch statistics in `stats` (from the
    conv epilogue), running statistics updated as bn_act does."""
    if not y.is_cuda:
        raise _lib.DvsError("bn_relu_pool: GPU tensors only; this package has no CPU path")
    B, C, H, W = y.shape
    if B % groups:
        raise _lib.DvsError("bn_relu_pool: batch %d does not split into %d groups" % (B, groups))
    count = (B // groups) * H * W
    y = _cl(y)
    st = stats if stats.dim() >= 3 else stats.unsqueeze(0)
    fin = _finalize_groups(st, count, bn, groups)
    out = _BNReluPool.apply(y, bn.weight, bn.bias, fin, groups, bool(need_z))
    return (out[1], out[0]) if need_z else (None, out)


def channel_stats(y, groups=1):
    """[G][2][C] per-channel sum / sum of squares of y (NHWC) in a fixed summation order: the deterministic stand-in for the
    convolution's atomic statistics epilogue (dvs_set_deterministic).  It is the BatchNorm backward's reduction kernel with
    (dz, mean, invstd) = (y, 0, 1): sum g = sum y, sum g * (y - 0) * 1 = sum y^2."""
    B, C, H, W = y.shape
    M = B * H * W // groups
    y = _cl(y)
    l = _lib.lib()
    table = torch.zeros(groups, 4, C, device=y.device, dtype=torch.float32)        # rows 2, 3: mean = 0, invstd = 1
    table[:, 3].fill_(1.0)
    sums = torch.zeros(groups, 2, C, device=y.device, dtype=torch.float32)
    ws = torch.empty(l.dvs_bn_bwd_workspace(M, C, groups) // 4, device=y.device, dtype=torch.float32)
    check(l.dvs_bn_bwd_reduce(y.data_ptr(), None, y.data_ptr(), table.data_ptr(), 0, None, sums.data_ptr(), ptr(ws), M, C, groups,
                              _lib.stream()), "dvs_bn_bwd_reduce")
    return sums if groups > 1 else sums[0]


def affine_supported(C):
    """C % 4 == 0 and C/4 dividing 256: C = 4, 8, 16 ... 1024 (a lane owns four channels, and a workgroup's 256 lanes hold whole
    rows of C/4 lanes)."""
    return C % 4 == 0 and 256 % (C // 4) == 0


def supported_c(C, bn):
    """The fused kernels cover training-mode affine BatchNorm at the channel counts of affine_supported."""
    return bn.training and bn.affine and affine_supported(C)


def bn_act(y, bn, stats, relu=False, residual=None, res_bn=None, res_stats=None, groups=1):
    """act(bn(y) + residual') with batch statistics taken from `stats` (filled by the conv that produced y);
    residual' = residual, or res_bn(residual) with its own `res_stats` (the BasicBlock downsample branch).
    groups = 2: y holds two independent batches back to back (PoseNet's two frame pairs); each half is
    normalised with its own statistics (stats = [2][2][C]) and the running statistics get both updates in order."""
    if not y.is_cuda:
        raise _lib.DvsError("bn_act: GPU tensors only; this package has no CPU path")
    B, C, H, W = y.shape
    if B % groups:
        raise _lib.DvsError("bn_act: batch %d does not split into %d groups" % (B, groups))
    count = (B // groups) * H * W
    y = _cl(y)
    stat_args = (stats, count) + _running_args(bn)
    res_fin = None
    if residual is not None:
        residual = _cl(residual)
        if res_bn is not None:
            res_fin = _finalize_groups(res_stats, count, res_bn, groups)
    return _BNAct.apply(y, bn.weight, bn.bias, residual, res_bn.weight if res_bn is not None else None,
                        res_bn.bias if res_bn is not None else None, stat_args, res_fin, relu, groups)


class _AffineAct(torch.autograd.Function):
    """z = act(y * scale[c] + shift[c] [+ residual]) on NHWC tensors -- an eval-mode BatchNorm2d (running statistics) with
    the BasicBlock tail, differentiable w.r.t. y, scale, shift and residual.  Same kernels as the training path with the
    statistics frozen: dvs_bn_apply_fwd forward; backward = dvs_bn_bwd_reduce with (mean, invstd) = (0, 1), which yields
    du = dz * [z > 0], sum(du) = d shift and sum(du * y) = d scale, then dvs_bn_bwd_apply with zero sums and gamma = scale,
    which is dy = scale * du."""

    @staticmethod
    def forward(ctx, y, scale, shift, residual, relu):
        B, C, H, W = y.shape
        M = B * H * W
        scale, shift = scale.contiguous(), shift.contiguous()
        z = torch.empty_like(y)
        check(_lib.lib().dvs_bn_apply_fwd(y.data_ptr(), ptr(scale), ptr(shift), _dp(residual), None, None, z.data_ptr(), M, C,
                                          int(relu), 1, _lib.stream()), "dvs_bn_apply_fwd")
        ctx.relu = relu
        ctx.has_res = residual is not None
        ctx.save_for_backward(y, scale, z if relu else None)
        return z

    @staticmethod
    def backward(ctx, dz):
        y, scale, z = ctx.saved_tensors
        l = _lib.lib()
        B, C, H, W = y.shape
        M = B * H * W
        dz = _cl(dz)
        # rows 2, 3: mean = 0, invstd = 1; rows 0, 1 (scale / shift, not read without the y-mask) stay zero: the apply pass's sums
        table = torch.zeros(1, 4, C, device=y.device, dtype=torch.float32)
        table[0, 3].fill_(1.0)
        sums = torch.zeros(1, 2, C, device=y.device, dtype=torch.float32)
        du = torch.empty_like(y) if ctx.relu else None
        dy = torch.empty_like(y)
        ws = torch.empty(l.dvs_bn_bwd_workspace(M, C, 1) // 4, device=y.device, dtype=torch.float32)
        check(l.dvs_bn_bwd_reduce(dz.data_ptr(), _dp(z), y.data_ptr(), table.data_ptr(), 0, _dp(du), sums.data_ptr(), ptr(ws), M, C, 1,
                                  _lib.stream()), "dvs_bn_bwd_reduce")
        check(l.dvs_bn_bwd_apply((du if ctx.relu else dz).data_ptr(), y.data_ptr(), table.data_ptr(), 0, ptr(scale), table.data_ptr(),
                                 dy.data_ptr(), M, C, None, None, 1, _lib.stream()), "dvs_bn_bwd_apply")
        d_scale, d_shift = _param_grads(sums)
        return dy, d_scale, d_shift, ((du if ctx.relu else dz) if ctx.has_res else None), None


def affine_act(y, scale, shift, relu=False, residual=None):
    """act(y * scale + shift [+ residual]); scale / shift are [C] tensors (eval-mode BatchNorm as an affine map)."""
    if not y.is_cuda:
        raise _lib.DvsError("affine_act: GPU tensors only; this package has no CPU path")
    C = y.shape[1]
    if not affine_supported(C):
        raise _lib.DvsError("affine_act: C %% 4 == 0 and C/4 dividing 256 required (got C = %d)" % C)
    y = _cl(y)
    if residual is not None:
        residual = _cl(residual)
        if residual.shape != y.shape:
            raise _lib.DvsError("affine_act: residual shape %s != %s" % (tuple(residual.shape), tuple(y.shape)))
    return _AffineAct.apply(y, scale, shift, residual, relu)
