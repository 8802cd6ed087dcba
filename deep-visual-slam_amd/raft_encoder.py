"""SmallRAFT's encoders on the device (model/raft/core/extractor.py:60-116, 195-267): Bottleneck stacks whose convolutions run on
conv.conv2d and whose norm / ReLU / residual tails run on csrc/inorm.hip.

    fnet = raft_encoder.SmallEncoder(128, "instance")       # raft.py:34
    cnet = raft_encoder.SmallEncoder(160, "none")           # raft.py:35
    fmap1, fmap2 = fnet([image1, image2])

`instance_norm_act(y, norm, relu, residual)` is the tail alone:

    z = (y - mean[n, c]) * invstd[n, c]  if norm     nn.InstanceNorm2d(C): no affine parameters, no running statistics, biased
    z = max(z, 0)                        if relu     variance, eps 1e-5, the input's own statistics in train and eval mode alike
    out = max(residual + z, 0)           if residual is not None

With norm_fn='none' every relu(conv + b) is the convolution's own act="relu" and only the block's closing relu(x + relu(.)) takes
the tail kernel (norm=False).  Parameter names and shapes are the reference's (conv1, layer{1,2,3}.{0,1}.conv{1,2,3},
layer{2,3}.0.downsample.0, conv2; the norms have no parameters), so the fnet. / cnet. parts of raft-small.pth load with
load_state_dict.  conv1 reads 3 channels: the image and the filter are zero-padded to 4, as raft_update pads the flow.
GPU and fp32 only; no host synchronisation in forward or backward.

BasicEncoder (extractor.py:118-192, full-size RAFT's fnet and cnet) follows further down: ResidualBlock stacks with the same
tail kernel, and norm_fn='batch' on the BatchNorm kernels of bn.py.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, conv
from . import bn as _bn_ops
from ._lib import DvsError, check
from ._raft_host import CL, DerivedOperands, aligned, gpu_arg


def slice_pixels():
    """T: the pixels of one slice of csrc/inorm.hip (one workgroup's share of an image)."""
    return int(_lib.lib().dvs_inorm_slice_pixels())


def _workspace(N, HW, Cn, device):
    nbytes = int(_lib.lib().dvs_inorm_workspace(N, HW, Cn))
    if nbytes == 0:
        raise DvsError("instance_norm_act: unsupported shape N=%d, HW=%d, C=%d (C %% 4 == 0, HW >= 2)" % (N, HW, Cn))
    return torch.empty(nbytes, device=device, dtype=torch.uint8), nbytes


class _InormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, residual, norm, relu):
        y = aligned(y.detach(), CL)
        N, Cn, H, W = y.shape
        res = aligned(residual.detach(), CL) if residual is not None else None
        out = torch.empty((N, H, W, Cn), device=y.device, dtype=torch.float32)
        table = ws = None
        nbytes = 0
        if norm:
            table = torch.empty((N, 2, Cn), device=y.device, dtype=torch.float32)
            ws, nbytes = _workspace(N, H * W, Cn, y.device)
        check(_lib.lib().dvs_inorm_fwd(y.data_ptr(), res.data_ptr() if res is not None else None, out.data_ptr(),
                                       table.data_ptr() if norm else None, ws.data_ptr() if norm else None, nbytes, N, H * W, Cn,
                                       int(norm), int(relu), _lib.stream()), "dvs_inorm_fwd")
        ctx.save_for_backward(y, out if res is not None else None, table)
        ctx.flags = (bool(norm), bool(relu))
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        y, out, table = ctx.saved_tensors
        norm, relu = ctx.flags
        N, Cn, H, W = y.shape
        dout = aligned(dout, CL)
        dy = torch.empty((N, H, W, Cn), device=y.device, dtype=torch.float32)
        dres = torch.empty((N, H, W, Cn), device=y.device, dtype=torch.float32) if out is not None else None
        ws, nbytes = _workspace(N, H * W, Cn, y.device) if norm else (None, 0)
        check(_lib.lib().dvs_inorm_bwd(dout.data_ptr(), y.data_ptr(), out.data_ptr() if out is not None else None,
                                       table.data_ptr() if norm else None, dy.data_ptr(), dres.data_ptr() if dres is not None else None,
                                       ws.data_ptr() if norm else None, nbytes, N, H * W, Cn, int(norm), int(relu), _lib.stream()),
              "dvs_inorm_bwd")
        return dy.permute(0, 3, 1, 2), dres.permute(0, 3, 1, 2) if dres is not None else None, None, None


def instance_norm_act(y, norm=True, relu=True, residual=None):
    """The fused tail (module docstring) of a [N,C,H,W] fp32 GPU tensor, differentiable in y and residual.  The result is in
    channels_last memory."""
    gpu_arg("instance_norm_act: y", y, "[N,C,H,W] expected")
    N, Cn, H, W = y.shape
    if Cn % 4 or Cn < 4 or Cn > 1024:
        raise DvsError("instance_norm_act: C=%d must be a multiple of 4 in 4 .. 1024 (16-byte channel groups)" % Cn)
    if N < 1 or H * W < 2:
        raise DvsError("instance_norm_act: %s: instance norm needs more than one spatial element per image (torch rejects it too)"
                       % (tuple(y.shape),))
    if residual is not None:
        gpu_arg("instance_norm_act: residual", residual, "[N,C,H,W] expected")
        if residual.shape != y.shape or residual.device != y.device:
            raise DvsError("instance_norm_act: residual %s on %s, y %s on %s"
                           % (tuple(residual.shape), residual.device, tuple(y.shape), y.device))
    return _InormAct.apply(y, residual, bool(norm), bool(relu))


# ---- the encoder ---------------------------------------------------------------------------------------------------------------
def _image4(x):
    """The image in NHWC memory with a zero fourth channel."""
    return F.pad(x.permute(0, 2, 3, 1), (0, 1)).permute(0, 3, 1, 2)


class _Encoder(DerivedOperands, nn.Module):
    """What the two encoders share (extractor.py:118-192, 195-267): conv1 7x7/2, three stages of two blocks, conv2 1x1.  A subclass
    names its blocks' convolutions in BLOCK_CONVS and provides _block(b, w, x)."""
    BLOCK_CONVS = ()

    def _build(self, widths, output_dim, block):
        """conv1, layer1 .. layer3 of two block(in_planes, planes, stride) each, conv2, in the reference's order and with its init
        (extractor.py:150-157, 226-228)."""
        if int(output_dim) <= 0 or int(output_dim) % 4:
            raise DvsError("%s: output_dim=%r must be a positive multiple of 4" % (type(self).__name__, output_dim))
        self.conv1 = nn.Conv2d(3, widths[0], kernel_size=7, stride=2, padding=3)
        planes = widths[0]
        for i, (dim, stride) in enumerate(zip(widths, (1, 2, 2)), 1):
            setattr(self, "layer%d" % i, nn.Sequential(block(planes, dim, stride), block(dim, dim, 1)))
            planes = dim
        self.conv2 = nn.Conv2d(planes, int(output_dim), kernel_size=1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self._drop()

    def _blocks(self):
        return [b for i in (1, 2, 3) for b in getattr(self, "layer%d" % i)]

    def _convs(self):
        out = [self.conv1]
        for b in self._blocks():
            out += [getattr(b, n) for n in self.BLOCK_CONVS] + ([b.downsample[0]] if b.downsample is not None else [])
        return out + [self.conv2]

    def _padding(self, m):
        """(zero input channels, zero output channels) that convolution `m` runs with: conv1 reads the 4-channel image."""
        return (1 if m is self.conv1 else 0), 0

    def _operands(self):
        """{conv module: (channels_last weight, bias)}, zero-padded by self._padding."""
        w = {}
        for m in self._convs():
            wt, b = m.weight, m.bias
            pad_i, pad_o = self._padding(m)
            if pad_i or pad_o:
                wt = F.pad(wt, (0, 0, 0, 0, 0, pad_i, 0, pad_o))
            if pad_o:
                b = F.pad(b, (0, pad_o))
            w[m] = (wt.contiguous(memory_format=CL), b)
        return w, [t for pair in w.values() for t in pair]

    def _unit(self, x, w, m, norm, stride=1, padding=0, relu=True):
        """[relu](norm(conv m)); `norm` is the norm's module, which only the 'batch' form reads."""
        wt, b = w[m]
        if self.norm_fn == "instance":
            return instance_norm_act(conv.conv2d(x, wt, b, stride=stride, padding=padding), relu=relu)
        return conv.conv2d(x, wt, b, stride=stride, padding=padding, act="relu" if relu else None)

    def forward(self, x, _image4_operand=False):
        """_image4_operand (private, raft.encode_frame's): x already is conv1's operand, the normalised image [N,4,H,W] in NHWC
        memory with a zero fourth channel, which dvs_frame_ingest writes: nothing stands between the ingest and conv1."""
        who = type(self).__name__
        if _image4_operand:
            gpu_arg(who + ": input", x, "[N,4,H,W] expected", ok=lambda shape: shape[1] == 4)
            if not x.is_contiguous(memory_format=CL) or x.data_ptr() % 16:
                raise DvsError("%s: the 4-channel operand must be dense NHWC memory on a 16-byte boundary, got strides %s" % (who, x.stride()))
            self._check_size(x)
            return self._from_image4(x, self._derive())
        is_list = isinstance(x, (tuple, list))
        if is_list:
            if len(x) != 2:
                raise DvsError("%s: a list input holds two image batches (extractor.py:171-174, 246-265), got %d" % (who, len(x)))
            for t in x:
                gpu_arg(who + ": input", t, "[N,C,H,W] expected")
            if x[0].shape != x[1].shape:
                raise DvsError("%s: the two batches differ: %s and %s" % (who, tuple(x[0].shape), tuple(x[1].shape)))
            batch_dim = x[0].shape[0]
            x = torch.cat(list(x), 0)
        gpu_arg(who + ": input", x, "[N,C,H,W] expected")
        if x.shape[1] != 3:
            raise DvsError("%s: 3 input channels expected, got %s" % (who, tuple(x.shape)))
        self._check_size(x)
        w = self._derive()
        x = self._from_image4(_image4(x), w)
        if is_list:
            return torch.split(x, [batch_dim, batch_dim], dim=0)
        return x

    def _check_size(self, x):
        who = type(self).__name__
        if x.shape[2] < 16 or x.shape[3] < 16:
            raise DvsError("%s: images of at least 16x16 expected (the instance norm needs 2 features), got %s" % (who, tuple(x.shape)))
        for p in self.parameters():
            if p.device != x.device or p.dtype != torch.float32:
                raise DvsError("%s: parameters on %s / %s, input on %s / fp32; move the module with .to()"
                               % (who, p.device, p.dtype, x.device))

    def _from_image4(self, x4, w):
        """conv1 onwards on the operand conv1 reads: the normalised image [N,4,H,W] in NHWC memory, fourth channel zero."""
        x = self._unit(x4, w, self.conv1, getattr(self, "norm1", None), 2, 3)
        for b in self._blocks():
            x = self._block(b, w, x)
        return conv.conv2d(x, *w[self.conv2])


class _Bottleneck(nn.Module):
    """Holds the parameters of one BottleneckBlock (extractor.py:60-104) under the reference's names."""

    def __init__(self, in_planes, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes // 4, kernel_size=1, padding=0)
        self.conv2 = nn.Conv2d(planes // 4, planes // 4, kernel_size=3, padding=1, stride=stride)
        self.conv3 = nn.Conv2d(planes // 4, planes, kernel_size=1, padding=0)
        self.stride = stride
        self.downsample = None if stride == 1 else nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride))


class SmallEncoder(_Encoder):
    BLOCK_CONVS = ("conv1", "conv2", "conv3")

    def __init__(self, output_dim=128, norm_fn="instance", dropout=0.0):
        super().__init__()
        if norm_fn not in ("instance", "none"):
            raise DvsError("SmallEncoder: norm_fn=%r is not built: SmallRAFT uses 'instance' (fnet) and 'none' (cnet) only" % (norm_fn,))
        if dropout and dropout > 0:
            raise DvsError("SmallEncoder: dropout=%r is not built: SmallRAFT forces it to 0 (raft.py:29)" % (dropout,))
        self.norm_fn = norm_fn
        self._build((32, 64, 96), output_dim, _Bottleneck)

    def _block(self, b, w, x):
        norm = self.norm_fn == "instance"
        s = b.stride
        y = self._unit(x, w, b.conv1, None)
        y = self._unit(y, w, b.conv2, None, s, 1)
        y = conv.conv2d(y, *w[b.conv3])
        if b.downsample is not None:
            x = conv.conv2d(x, *w[b.downsample[0]], stride=s)
            if norm:
                x = instance_norm_act(x, relu=False)
        return instance_norm_act(y, norm=norm, relu=True, residual=x)          # relu(x + relu(norm3(conv3(.)))), extractor.py:111-116


# ---- the full-size encoder -----------------------------------------------------------------------------------------------------
BN_WIDTH = {64: 64, 96: 128, 128: 128}      # channels a stage runs at: dvs_bn_* cover C/4 dividing 256, which 96 / 4 = 24 does not


class _Residual(nn.Module):
    """Holds the parameters and buffers of one ResidualBlock (extractor.py:6-56) under the reference's names, in its order."""

    def __init__(self, in_planes, planes, norm_fn, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        make = (lambda: nn.BatchNorm2d(planes)) if norm_fn == "batch" else (lambda: nn.Sequential())
        self.norm1, self.norm2 = make(), make()
        if stride != 1:
            self.norm3 = make()
        self.stride = stride
        # the reference's Sequential(conv, norm3): norm3 is registered twice, its state-dict keys appear under both names
        self.downsample = None if stride == 1 else nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm3)


class BasicEncoder(_Encoder):
    """extractor.py:118-192: conv1 7x7/2 3->64, norm, ReLU, three stages of two ResidualBlocks (64, 96/2, 128/2), conv2 1x1.

    norm_fn 'instance' (RAFT's fnet) and 'none' run as SmallEncoder does.  'batch' (RAFT's cnet) runs on bn.bn_act in train mode
    (batch statistics from the convolution's epilogue, running statistics and num_batches_tracked updated as nn.BatchNorm2d does)
    and on bn.affine_act in eval mode and under freeze_bn (running statistics).  The convolutions in front of a BatchNorm have
    biases here, unlike ResNet's, and the BatchNorm kernels take the convolution's output without one:
        train   bn(conv + b) = bn(conv), the batch mean absorbs b; running_mean, which does see it, gets momentum * b added.
                b receives an exactly-zero gradient (torch's is zero up to rounding).
        eval    bn(conv + b) = conv * scale + (shift + b * scale), differentiable in b.
    The 96-channel stage runs zero-padded to 128 channels in the 'batch' form: filters, gamma (1), beta (0) and the running
    statistics are padded by differentiable torch ops, the padded channels stay exactly zero through ReLU, the residual adds and
    the next stage's zero input filters, and their gradients are dropped by the padding's backward."""

    BLOCK_CONVS = ("conv1", "conv2")

    def __init__(self, output_dim=128, norm_fn="batch", dropout=0.0):
        super().__init__()
        if norm_fn not in ("instance", "batch", "none"):
            raise DvsError("BasicEncoder: norm_fn=%r is not built: RAFT uses 'instance' (fnet) and 'batch' (cnet); 'none' is built too"
                           % (norm_fn,))
        if dropout and dropout > 0:
            raise DvsError("BasicEncoder: dropout=%r is not built: train with dropout=0 (the released RAFT checkpoints do)" % (dropout,))
        self.norm_fn = norm_fn
        self.norm1 = nn.BatchNorm2d(64) if norm_fn == "batch" else nn.Sequential()
        self._build((64, 96, 128), output_dim, lambda in_planes, planes, stride: _Residual(in_planes, planes, norm_fn, stride))

    def _padding(self, m):
        """In the 'batch' form every 96 becomes 128 as well: zero filters, zero input channels, zero biases."""
        pad_i, pad_o = super()._padding(m)
        if self.norm_fn == "batch":
            co, ci = m.weight.shape[:2]
            if m is not self.conv1:
                pad_i = BN_WIDTH.get(ci, ci) - ci
            if m is not self.conv2:
                pad_o = BN_WIDTH.get(co, co) - co
        return pad_i, pad_o

    # ---- conv -> norm -> ReLU, by norm_fn --------------------------------------------------------------------------------------
    def _bn(self, y_conv, bias, bn, relu):
        """[relu](bn(conv + bias)) from the bias-free convolution `y_conv` = (x, weight, stride, padding)."""
        x, weight, stride, padding = y_conv
        C = weight.shape[0]
        pad = C - bn.num_features
        if not bn.affine or not bn.track_running_stats or bn.momentum is None:
            raise DvsError("BasicEncoder: BatchNorm2d as the reference builds it expected (affine, running statistics, a momentum)")
        if bn.training:
            if _lib.deterministic():                        # no atomic statistics epilogue: an ordered reduction pass (nn_ops.conv_bn_act)
                y = conv.conv2d(x, weight, None, stride=stride, padding=padding)
                stats = _bn_ops.channel_stats(y.detach())
            else:
                y, stats = conv.conv2d(x, weight, None, stride=stride, padding=padding, want_stats=1)
            view = _TrainBN(bn, pad, bias)
            out = _bn_ops.bn_act(y, view, stats, relu=relu)
            view.write_back()
            return out
        inv = torch.rsqrt(bn.running_var + bn.eps)
        scale = bn.weight * inv
        shift = bn.bias - bn.running_mean * scale
        if pad:
            scale, shift = F.pad(scale, (0, pad), value=1.0), F.pad(shift, (0, pad))
        y = conv.conv2d(x, weight, None, stride=stride, padding=padding)
        return _bn_ops.affine_act(y, scale, shift + bias * scale, relu=relu)

    def _unit(self, x, w, m, norm, stride=1, padding=0, relu=True):
        if self.norm_fn == "batch":
            wt, b = w[m]
            return self._bn((x, wt, stride, padding), b, norm, relu)
        return super()._unit(x, w, m, norm, stride, padding, relu)

    def _block(self, b, w, x):
        s = b.stride
        y = self._unit(x, w, b.conv1, b.norm1, s, 1)
        if b.downsample is not None:
            x = self._unit(x, w, b.downsample[0], b.norm3, s, 0, relu=False)
        if self.norm_fn == "instance":
            wt, bias = w[b.conv2]                           # relu(x + relu(norm2(conv2 y))) is the fused tail
            return instance_norm_act(conv.conv2d(y, wt, bias, padding=1), norm=True, relu=True, residual=x)
        y = self._unit(y, w, b.conv2, b.norm2, 1, 1)
        return instance_norm_act(y, norm=False, relu=False, residual=x)      # relu(x + y), extractor.py:56


class _TrainBN:
    """A train-mode nn.BatchNorm2d as bn.bn_act sees it behind a convolution whose bias was left out, `pad` channels wider: gamma
    padded with ones, beta with zeros (differentiable; the convolution's bias rides on beta with factor 0, so that it receives
    the exactly-zero gradient it has instead of none), running statistics in padded copies.  write_back() returns them to the
    module's own buffers and adds momentum * bias to running_mean, which, unlike the output, does see the bias."""

    def __init__(self, bn, pad, conv_bias):
        self.bn, self.n, self.pad = bn, bn.num_features, pad
        self.conv_bias = conv_bias.detach()[:self.n]
        self.weight = F.pad(bn.weight, (0, pad), value=1.0)
        self.bias = F.pad(bn.bias + 0.0 * conv_bias[:self.n], (0, pad))
        self.running_mean = F.pad(bn.running_mean, (0, pad)) if pad else bn.running_mean
        self.running_var = F.pad(bn.running_var, (0, pad), value=1.0) if pad else bn.running_var
        self.momentum, self.eps, self.num_batches_tracked = bn.momentum, bn.eps, bn.num_batches_tracked
        self.training = self.track_running_stats = self.affine = True

    def write_back(self):
        with torch.no_grad():
            if self.pad:
                self.bn.running_mean.copy_(self.running_mean[:self.n])
                self.bn.running_var.copy_(self.running_var[:self.n])
            self.bn.running_mean.add_(self.conv_bias, alpha=float(self.momentum))
