"""PoseNet and FlowPoseNet -- drop-ins for the reference's model/posenet_single.py:149-202 and 91-147.

    pose_net = PoseNet(num_layers=18, pretrained=True, num_input_images=2)       # what vo/train.py:89 constructs
    pose_net = FlowPoseNet()                                                     # the alternate: reads ./raft-small.pth
    axisangle, translation = pose_net(torch.cat([frame_a, frame_b], 1))          # [B,6,H,W] in 0 .. 1 -> two [B,1,1,3]

`FlowPoseNet` is SmallRAFT (raft.py) on the frame pair, its final flow through three strided convolutions (conv.conv2d) and the
pooling head of csrc/posehead.hip: ReLU, global average pooling, Linear(128, 6) and the 0.01 pose scale in two launches forward and
two backward (`pool_fc`).  The RAFT checkpoint is absent from the reference tree: without the file the
constructor raises `NoRaftCheckpoint`, as the reference raises FileNotFoundError.  The reference's ConvGRU and FlowUpdateModule
(lines 21-89) are dead code there and are not built.  GPU and fp32 only; no host synchronisation in forward or backward."""
import os
from collections import OrderedDict
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, nn_ops
from ._lib import DvsError, check
from ._raft_host import CL, aligned, gpu_arg
from .raft import SmallRAFT
from .resnet_encoder import ResnetEncoder


class PoseNet(nn.Module):
    """Pose estimation network with ResNet encoder and pose decoder"""
    supports_pairs = True      # forward(x, pairs=2): two frame pairs in one pass (see forward)

    def __init__(self, num_layers=18, pretrained=True, num_input_images=2, stride=1):
        super().__init__()
        self.num_input_images = num_input_images
        self.stride = stride
        self.encoder = ResnetEncoder(num_layers=num_layers, pretrained=pretrained,
                                     num_input_images=num_input_images)
        self.encoder.need_feature0 = False      # only feature[-1] is read below
        self.num_ch_enc = self.encoder.num_ch_enc
        self.convs = OrderedDict()
        self.convs[("squeeze")] = nn.Conv2d(self.num_ch_enc[-1], 256, 1)
        self.convs[("pose", 0)] = nn.Conv2d(256, 256, 3, stride, 1)
        self.convs[("pose", 1)] = nn.Conv2d(256, 256, 3, stride, 1)
        self.convs[("pose", 2)] = nn.Conv2d(256, 6, 1)
        self.relu = nn.ReLU()
        self.net = nn.ModuleList(list(self.convs.values()))
        # weights live as [Cout][kh][kw][Cin] in memory (same logical shapes / state_dict)
        self.to(memory_format=torch.channels_last)

    def forward(self, input_images, pairs=1):
        """pairs = 2 (an extension of the reference signature): `input_images` holds two batches back to back --
        MonodepthTrainer's (left, target) and (target, right) pairs -- evaluated in one pass; BatchNorm treats each
        half as its own batch, so outputs, gradients and running statistics equal two calls."""
        with nn_ops.batch_groups(pairs):
            feature = self.encoder(input_images)
        sq = self.convs["squeeze"]
        out = nn_ops.conv2d(feature[-1], sq.weight, sq.bias, 1, 0, act="relu")
        for i in range(3):
            c = self.convs[("pose", i)]
            out = nn_ops.conv2d(out, c.weight, c.bias, c.stride[0], c.padding[0], act="relu" if i != 2 else None)
        out = out.mean(3).mean(2)
        out = 0.01 * out.view(-1, 1, 1, 6)
        return out[..., :3], out[..., 3:]


class NoRaftCheckpoint(DvsError, NotImplementedError, FileNotFoundError):
    """FlowPoseNet found no RAFT checkpoint.  The reference fails with FileNotFoundError at this point (posenet_single.py:104);
    NotImplementedError is what callers caught while the class was a name only (the precedent of raft_corr.NoCpuPath)."""


def pool_fc_slice_pixels():
    """T: the pixels of one slice of csrc/posehead.hip (one workgroup's share of a sample)."""
    return int(_lib.lib().dvs_pool_fc_slice_pixels())


class _PoolFc(torch.autograd.Function):
    """scale * fc(mean_hw(relu(y))) on dvs_pool_fc_fwd / dvs_pool_fc_bwd (csrc/posehead.hip); y is read in NHWC memory."""

    @staticmethod
    def forward(ctx, y, weight, bias, relu, scale):
        y = aligned(y.detach(), CL)
        weight, bias = aligned(weight.detach()), aligned(bias.detach()) if bias is not None else None
        N, Cn, H, W = y.shape
        J, P = weight.shape[0], H * W
        lib = _lib.lib()
        nbytes = int(lib.dvs_pool_fc_workspace(N, P, Cn))
        if nbytes == 0 or not 1 <= J <= 16:
            raise DvsError("pool_fc: unsupported shape N=%d, P=%d, C=%d, J=%d (C %% 4 == 0 up to 1024, J <= 16)" % (N, P, Cn, J))
        ws = torch.empty(nbytes, device=y.device, dtype=torch.uint8)
        out = torch.empty((N, J), device=y.device, dtype=torch.float32)
        mean = torch.empty((N, Cn), device=y.device, dtype=torch.float32)
        check(lib.dvs_pool_fc_fwd(y.data_ptr(), weight.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(),
                                  mean.data_ptr(), ws.data_ptr(), nbytes, N, P, Cn, J, int(relu), float(scale), _lib.stream()),
              "dvs_pool_fc_fwd")
        ctx.save_for_backward(y, mean, weight)
        ctx.head = (bool(relu), float(scale), bias is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, mean, weight = ctx.saved_tensors
        relu, scale, has_bias = ctx.head
        N, Cn, H, W = y.shape
        J = weight.shape[0]
        dout = aligned(dout)
        dy = torch.empty((N, H, W, Cn), device=y.device, dtype=torch.float32)
        dw = torch.empty((J, Cn), device=y.device, dtype=torch.float32)
        db = torch.empty((J,), device=y.device, dtype=torch.float32) if has_bias else None
        check(_lib.lib().dvs_pool_fc_bwd(dout.data_ptr(), y.data_ptr(), mean.data_ptr(), weight.data_ptr(), dy.data_ptr(),
                                         dw.data_ptr(), db.data_ptr() if has_bias else None, N, H * W, Cn, J, int(relu), scale,
                                         _lib.stream()), "dvs_pool_fc_bwd")
        return dy.permute(0, 3, 1, 2), dw, db, None, None


def pool_fc(y, weight, bias=None, relu=True, scale=1.0):
    """scale * (mean over H x W of relu(y)) @ weight.T + scale * bias of a [N,C,H,W] fp32 GPU tensor: [N,J].  Differentiable in y,
    weight and bias; bit-reproducible in both directions."""
    for name, t in (("y", y), ("weight", weight)) + ((("bias", bias),) if bias is not None else ()):
        gpu_arg("pool_fc: " + name, t)
    if y.dim() != 4 or weight.dim() != 2 or weight.shape[1] != y.shape[1] or (bias is not None and tuple(bias.shape) != (weight.shape[0],)):
        raise DvsError("pool_fc: y [N,C,H,W], weight [J,C], bias [J] expected, got %s, %s, %s"
                       % (tuple(y.shape), tuple(weight.shape), tuple(bias.shape) if bias is not None else None))
    return _PoolFc.apply(y, weight, bias, bool(relu), float(scale))


class FlowPoseNet(nn.Module):
    """The reference's alternate pose network (model/posenet_single.py:91-147): SmallRAFT flow of the frame pair, three strided
    convolutions, global average pooling, Linear(128, 6), * 0.01.  Module tree and state-dict keys are the reference's
    (flow_net.*, pose_cnn.{0,2,4}.*, fc.*).  raft_checkpoint=None skips the checkpoint load (an extension, for callers that load
    a whole FlowPoseNet state dict next); iters and alternate_corr go to SmallRAFT (the reference hard-codes 12 and False)."""
    supports_pairs = True      # nothing couples the samples of a batch (instance norm is per image): `pairs` is accepted and ignored

    def __init__(self, raft_checkpoint="./raft-small.pth", iters=12, alternate_corr=False):
        super().__init__()
        self.iters = int(iters)
        self.flow_net = SmallRAFT(SimpleNamespace(small=True, alternate_corr=bool(alternate_corr), mixed_precision=False))
        if raft_checkpoint is not None:
            if not os.path.isfile(raft_checkpoint):
                raise NoRaftCheckpoint("FlowPoseNet: no RAFT checkpoint at %s (%s): put raft-small.pth there, or pass "
                                       "raft_checkpoint=None and load a whole FlowPoseNet state dict"
                                       % (raft_checkpoint, os.path.abspath(raft_checkpoint)))
            ckpt = torch.load(raft_checkpoint, map_location="cpu", weights_only=True)
            self.flow_net.load_state_dict({(k[len("module."):] if k.startswith("module.") else k): v for k, v in ckpt.items()},
                                          strict=True)
        self.pose_cnn = nn.Sequential(
            nn.Conv2d(2, 32, kernel_size=7, stride=2, padding=3),
            nn.ReLU(inplace=True),
            nn.Conv2d(32, 64, kernel_size=5, stride=2, padding=2),
            nn.ReLU(inplace=True),
            nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1),
            nn.ReLU(inplace=True),
            nn.AdaptiveAvgPool2d(1),
        )
        self.fc = nn.Linear(128, 6)
        self.pose_scale = 0.01
        self.pose_cnn.to(memory_format=torch.channels_last)     # weights as [Cout][kh][kw][Cin], as everywhere in the package

    def _check(self, x):
        gpu_arg("FlowPoseNet", x, "[B,6,H,W] expected (two RGB frames along the channels)",
                ok=lambda shape: shape[1] == 6 and shape[0] >= 1)

    def extract_flow(self, x1, x2):
        return self.flow_net(x1, x2, iters=self.iters, last_only=True)[-1]

    def regress(self, flow):
        """pose_cnn, fc and the scale on a planar [B,2,H,W] flow: [B,6]."""
        c0, c2, c4 = self.pose_cnn[0], self.pose_cnn[2], self.pose_cnn[4]
        # the flow goes in as raft_update's convf1 takes it: NHWC with two zero channels behind its own, the filter padded to match
        # by a differentiable op so that the gradient lands on the [32,2,7,7] parameter
        flow4 = F.pad(flow.permute(0, 2, 3, 1), (0, 2)).contiguous().permute(0, 3, 1, 2)
        w0 = F.pad(c0.weight, (0, 0, 0, 0, 0, 2)).contiguous(memory_format=torch.channels_last)
        x = nn_ops.conv2d(flow4, w0, c0.bias, 2, 3, act="relu")
        x = nn_ops.conv2d(x, c2.weight, c2.bias, 2, 2, act="relu")
        x = nn_ops.conv2d(x, c4.weight, c4.bias, 2, 1)          # its ReLU is the pooling head's
        return pool_fc(x, self.fc.weight, self.fc.bias, relu=True, scale=self.pose_scale)

    def forward(self, input_images, pairs=1):
        self._check(input_images)
        flow = self.extract_flow(input_images[:, :3], input_images[:, 3:])
        pose6 = self.regress(flow).view(-1, 1, 1, 6)
        return pose6[..., :3], pose6[..., 3:]
