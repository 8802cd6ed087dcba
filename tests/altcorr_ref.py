"""The on-the-fly correlation block, restated (model/raft/core/corr.py:63-91 over model/raft/alt_cuda_corr/correlation_kernel.cu).

Plain torch on the CPU, one function for every precision, like tests/corr_ref.py -- but windowed: no volume.  Per level the
(2r+2)^2 cells around floor(coords / 2^i) are gathered from the pooled fmap2 by index (memory O(C * N * (2r+2)^2)), dotted with
the pixel's fmap1 vector over C, divided by sqrt(C), set to 0 where the cell lies outside the map, and blended into the
(2r+1)^2 taps.  Pooling is linear, so in exact arithmetic this is corr_ref.corr_block; it exists because corr_ref builds the
(h*w)^2 volume and cannot run where that does not fit.  Differentiable in the feature maps, never in the coordinates.

The corner is floor(coords / 2^i), as in the kernel file, not corr_ref's trip through the normalised grid (the alternate form
of the reference never builds that grid).

    channel  i * (2r+1)^2 + a * (2r+1) + e   =   level i at (x / 2^i + a - r,  y / 2^i + e - r)        a: the slow index
"""
import math

import torch


def pooled(fmap2, num_levels):
    """[fmap2, avg_pool2d(fmap2, 2, 2), ...]: num_levels maps; an odd trailing row / column is dropped."""
    maps = [fmap2]
    for _ in range(num_levels - 1):
        m = maps[-1]
        B, C, h, w = m.shape
        h2, w2 = h // 2, w // 2
        m = m[:, :, :2 * h2, :2 * w2].reshape(B, C, h2, 2, w2, 2)
        maps.append((m[:, :, :, 0, :, 0] + m[:, :, :, 0, :, 1] + m[:, :, :, 1, :, 0] + m[:, :, :, 1, :, 1]) * 0.25)
    return maps


def lookup_level(fmap1, f2, coords, i, r):
    """[B, (2r+1)^2, H, W] of level i: f2 is the i times pooled fmap2, coords [B,2,H,W] at level-0 scale, x first."""
    B, C, H, W = fmap1.shape
    h, w = f2.shape[-2:]
    N, S, T = H * W, 2 * r + 2, 2 * r + 1
    dt = fmap1.dtype
    c = coords.detach().to(dt).reshape(B, 2, N) / 2 ** i
    lo = torch.floor(c)
    fx, fy = (c - lo)[:, 0, :, None, None], (c - lo)[:, 1, :, None, None]                 # [B,N,1,1]
    d = torch.arange(-r, r + 2)
    X = lo[:, 0].long()[:, :, None, None] + d[None, None, None, :]                        # [B,N,1,S]  (u)
    Y = lo[:, 1].long()[:, :, None, None] + d[None, None, :, None]                        # [B,N,S,1]  (v)
    inside = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)                                      # [B,N,S,S]  [v][u]
    idx = (Y.clamp(0, h - 1) * w + X.clamp(0, w - 1)).reshape(B, N * S * S)
    rows = f2.reshape(B, C, h * w).transpose(1, 2)                                        # [B, h*w, C]
    cells = torch.gather(rows, 1, idx[:, :, None].expand(B, N * S * S, C)).reshape(B, N, S * S, C)
    f1 = fmap1.reshape(B, C, N).transpose(1, 2)                                           # [B, N, C]
    s = (cells * f1[:, :, None, :]).sum(3).reshape(B, N, S, S) / math.sqrt(C)
    s = torch.where(inside, s, torch.zeros((), dtype=dt))
    taps = (s[:, :, :T, :T] * (1 - fx) * (1 - fy) + s[:, :, :T, 1:] * fx * (1 - fy)
            + s[:, :, 1:, :T] * (1 - fx) * fy + s[:, :, 1:, 1:] * fx * fy)                # [B,N,T(e),T(a)]
    return taps.transpose(2, 3).reshape(B, N, T * T).transpose(1, 2).reshape(B, T * T, H, W)


def corr_block(fmap1, fmap2, coords_list, num_levels=4, radius=4):
    """[lookup(coords) for coords in coords_list], every level from the same pooled maps."""
    maps = pooled(fmap2, num_levels)
    return [torch.cat([lookup_level(fmap1, m, c, i, radius) for i, m in enumerate(maps)], 1) for c in coords_list]


def grads(fmap1, fmap2, coords_list, douts, num_levels=4, radius=4):
    """(outs, dfmap1, dfmap2) for the loss sum_k <out_k, dout_k>: the signature of corr_ref.grads."""
    f1 = fmap1.detach().clone().requires_grad_(True)
    f2 = fmap2.detach().clone().requires_grad_(True)
    outs = corr_block(f1, f2, coords_list, num_levels, radius)
    loss = sum((o * d.to(o.dtype)).sum() for o, d in zip(outs, douts))
    g1, g2 = torch.autograd.grad(loss, [f1, f2])
    return [o.detach() for o in outs], g1, g2
