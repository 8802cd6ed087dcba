"""The correlation block, restated (model/raft/core/corr.py:12-60 with bilinear_sampler, utils/utils.py:57-71).

Plain torch on the CPU, one function for every precision: pass fp64 tensors for the truth and fp32 tensors for the error that
fp32 arithmetic of this formulation makes on the same inputs.  Everything is an explicit gather: a tap's four corners are
found with `floor`, looked up by index, and a corner outside the map contributes 0.  Differentiable in the feature maps (the
gathers are torch.gather), never in the coordinates.

The sample position goes through the normalised grid the reference builds (x -> 2x/(W-1) - 1 -> back): in fp64 that is the
identity to 1e-16, in fp32 it is where most of the reference's own rounding comes from, so the fp32 run of this file carries it.

    channel  i * (2r+1)^2 + a * (2r+1) + e   =   level i at (x / 2^i + a - r,  y / 2^i + e - r)        a: the slow index
"""
import math

import numpy as np
import torch


def level_sizes(H, W, num_levels):
    return [(H >> i, W >> i) for i in range(num_levels)]


def volume(fmap1, fmap2):
    """[B, N, h, w]: row p = correlation of position p of fmap1 with every position of fmap2, / sqrt(C)."""
    B, C, H, W = fmap1.shape
    a = fmap1.reshape(B, C, H * W).transpose(1, 2)
    v = torch.matmul(a, fmap2.reshape(B, C, H * W)) / math.sqrt(C)
    return v.reshape(B, H * W, H, W)


def pool2(v):
    """2 x 2 mean with stride 2; an odd trailing row / column is dropped."""
    B, N, h, w = v.shape
    h2, w2 = h // 2, w // 2
    v = v[:, :, :2 * h2, :2 * w2].reshape(B, N, h2, 2, w2, 2)
    return (v[:, :, :, 0, :, 0] + v[:, :, :, 0, :, 1] + v[:, :, :, 1, :, 0] + v[:, :, :, 1, :, 1]) * 0.25


def pyramid(fmap1, fmap2, num_levels=4):
    levels = [volume(fmap1, fmap2)]
    for _ in range(num_levels - 1):
        levels.append(pool2(levels[-1]))
    return levels


def _axis(c, r, size):
    """c [B,N] centre along one axis -> (lower corner index [B,N,T] int64, fraction [B,N,T]) of the T = 2r+1 taps."""
    d = torch.arange(-r, r + 1, dtype=c.dtype)
    pos = c[:, :, None] + d
    pos = ((2 * pos / (size - 1) - 1) + 1) / 2 * (size - 1)         # through the normalised grid and back
    lo = torch.floor(pos)
    return lo.long(), pos - lo


def _gather(level, yi, xi):
    """level [B,N,h,w]; yi [B,N,T] (tap e), xi [B,N,T] (tap a) -> [B,N,T(a),T(e)] values, 0 outside the map."""
    B, N, h, w = level.shape
    Y, X = yi[:, :, None, :], xi[:, :, :, None]
    inside = (Y >= 0) & (Y < h) & (X >= 0) & (X < w)
    idx = (Y.clamp(0, h - 1) * w + X.clamp(0, w - 1)).reshape(B, N, -1)
    val = torch.gather(level.reshape(B, N, h * w), 2, idx).reshape(inside.shape)
    return torch.where(inside, val, torch.zeros((), dtype=level.dtype))


def lookup_level(level, coords, i, r):
    """[B, (2r+1)^2, H, W] of one level (coords [B,2,H,W] at level-0 scale, x first)."""
    B, N, h, w = level.shape
    H, W = coords.shape[-2:]
    c = coords.detach().to(level.dtype).reshape(B, 2, N) / 2 ** i
    x0, fx = _axis(c[:, 0], r, w)
    y0, fy = _axis(c[:, 1], r, h)
    FX, FY = fx[:, :, :, None], fy[:, :, None, :]
    out = (_gather(level, y0, x0) * (1 - FX) * (1 - FY) + _gather(level, y0, x0 + 1) * FX * (1 - FY)
           + _gather(level, y0 + 1, x0) * (1 - FX) * FY + _gather(level, y0 + 1, x0 + 1) * FX * FY)
    T = 2 * r + 1
    return out.reshape(B, N, T * T).transpose(1, 2).reshape(B, T * T, H, W)


def lookup(levels, coords, r):
    return torch.cat([lookup_level(lv, coords, i, r) for i, lv in enumerate(levels)], 1)


def corr_block(fmap1, fmap2, coords_list, num_levels=4, radius=4):
    """[lookup(coords) for coords in coords_list] on one pyramid."""
    levels = pyramid(fmap1, fmap2, num_levels)
    return [lookup(levels, c, radius) for c in coords_list]


def grads(fmap1, fmap2, coords_list, douts, num_levels=4, radius=4):
    """(outs, dfmap1, dfmap2) for the loss sum_k <out_k, dout_k>."""
    f1 = fmap1.detach().clone().requires_grad_(True)
    f2 = fmap2.detach().clone().requires_grad_(True)
    outs = corr_block(f1, f2, coords_list, num_levels, radius)
    loss = sum((o * d.to(o.dtype)).sum() for o, d in zip(outs, douts))
    g1, g2 = torch.autograd.grad(loss, [f1, f2])
    return [o.detach() for o in outs], g1, g2


def level_slices(num_levels, radius):
    T2 = (2 * radius + 1) ** 2
    return [slice(i * T2, (i + 1) * T2) for i in range(num_levels)]


def level_grads(fmap1, fmap2, coords_list, douts, num_levels, radius):
    """Per level: (dfmap1, dfmap2) of the loss restricted to that level's channels (what a wrong coarse level would change)."""
    res = []
    for sl in level_slices(num_levels, radius):
        masked = []
        for d in douts:
            m = torch.zeros_like(d)
            m[:, sl] = d[:, sl]
            masked.append(m)
        _, g1, g2 = grads(fmap1, fmap2, coords_list, masked, num_levels, radius)
        res.append((g1, g2))
    return res


# ---- what the GPU tests share: the bound, the comparison, seeded cases ---------------------------------------------------------
def bound(ref64, ref32):
    floor = 2.0 * float(np.spacing(np.float32(float(ref64.abs().max()))))
    return max(3.0 * float((ref32.double() - ref64).abs().max()), floor)


def check(name, got, ref64, ref32):
    got = got.detach().double().cpu()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    err, b = float((got - ref64).abs().max()), bound(ref64, ref32)
    print("%s: max |err| %.3e, bound %.3e" % (name, err, b))
    assert err <= b, (name, err, b)


def make_case(B, Cn, H, W, L, r, n_lookups=1, seed=0, sigma=2.0):
    gen = torch.Generator().manual_seed(seed)
    f1, f2 = torch.randn(B, Cn, H, W, generator=gen), torch.randn(B, Cn, H, W, generator=gen)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None].repeat(B, 1, 1, 1)
    coords = []
    for _ in range(n_lookups):
        c = grid + sigma * torch.randn(B, 2, H, W, generator=gen)
        c[0, :, 0, 0:4] = torch.tensor([[2.0, -0.5, -1.0, W - 1.0], [3.0, -0.25, H - 1.0, -1.0]])
        c[-1, :, 1, 0:2] = torch.tensor([[-(r + 3.0), W - 1 + r + 3.0], [H - 1 + r + 3.0, 1.5]])
        coords.append(c)
    douts = [torch.randn(B, L * (2 * r + 1) ** 2, H, W, generator=gen) for _ in range(n_lookups)]
    return f1, f2, coords, douts


def reference(f1, f2, coords, douts, L, r):
    res = {}
    for dt in (torch.float64, torch.float32):
        res[dt] = grads(f1.to(dt), f2.to(dt), coords, douts, L, r)
    return res
