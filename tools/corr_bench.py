"""Correlation block at the FlowPoseNet working shape: feature maps 60x80, C=128, r=3, 4 levels; B=1 and B=12; one build + 12
lookups forward, and the same with its backward.  Device events after warm-up, one process, the two arms alternated:

  hip    raft_corr.CorrBlock (csrc/corr.hip)
  torch  the same computation composed from PyTorch-ROCm ops -- matmul, avg_pool2d, grid_sample: the reference's formulation

Per C entry point of the hip arm, each called directly on preallocated buffers and timed alone with events: dvs_corr_build (the
pool pre-kernel and the GEMM; the pre-kernel is microseconds) with its achieved TF/s against the 157.3 TF fp32 matrix peak,
flops 2 * (h*w) * (sum of level sizes) * C, and its bytes written per second against a device-to-device copy of the same size
timed in the same run (not the project's earlier 5.5 TB/s figure), and which of the two bounds it; one lookup forward, one
lookup backward, the volume backward.

usage: corr_bench.py [--batches 1,12] [--iters 10] [--warmup 3] [--repeats 3] [--lookups 12] [--out FILE]
Prints one JSON line; per number the median over the iterations of every repeat (their spread is the run-to-run spread)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_visual_slam_amd import raft_corr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,12")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--lookups", type=int, default=12)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
H, W, C, R, L = 60, 80, 128, 3, 4
PEAK_TF = 157.3
CL = torch.channels_last


SIZES = [(H >> i, W >> i) for i in range(L)]
T = 2 * R + 1


def torch_block(f1, f2):
    """Pyramid of the baseline: one matmul for the volume, then avg_pool2d level by level on [B*N, 1, h_i, w_i] images."""
    B, N = f1.shape[0], H * W
    vol = torch.bmm(f1.flatten(2).transpose(1, 2), f2.flatten(2)) * (1.0 / math.sqrt(C))
    pyr = [vol.view(B * N, 1, H, W)]
    while len(pyr) < L:
        pyr.append(F.avg_pool2d(pyr[-1], kernel_size=2))
    return pyr


def torch_lookup(pyr, coords):
    """Baseline lookup: per level ONE grid_sample call whose grid [B*N, T, T, 2] holds, for every pixel, the window
    (x / 2^i + a - r, y / 2^i + e - r) normalised to [-1, 1] for align_corners=True, window index a (the x offset) first."""
    B, N = coords.shape[0], H * W
    xy = coords.flatten(2).transpose(1, 2).reshape(B * N, 2)                    # [B*N, (x, y)]
    win = torch.arange(-R, R + 1, device=dev, dtype=torch.float32)
    feats = []
    for i, (hi, wi) in enumerate(SIZES):
        gx = ((xy[:, 0:1] * 0.5 ** i + win) * (2.0 / (wi - 1)) - 1.0)[:, :, None].expand(B * N, T, T)        # varies with a
        gy = ((xy[:, 1:2] * 0.5 ** i + win) * (2.0 / (hi - 1)) - 1.0)[:, None, :].expand(B * N, T, T)        # varies with e
        taps = F.grid_sample(pyr[i], torch.stack([gx, gy], dim=3), mode="bilinear", padding_mode="zeros", align_corners=True)
        feats.append(taps.view(B, N, T * T))
    return torch.cat(feats, dim=2).transpose(1, 2).reshape(B, L * T * T, H, W)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def spread(vals):
    return {"median_ms": round(statistics.median(vals), 4), "min_ms": round(min(vals), 4), "max_ms": round(max(vals), 4)}


result = {"shape": dict(H=H, W=W, C=C, radius=R, levels=L, lookups=args.lookups), "cases": {}}
for B in [int(b) for b in args.batches.split(",")]:
    gen = torch.Generator(device="cpu").manual_seed(B)
    f1 = torch.randn(B, C, H, W, generator=gen).to(dev).contiguous(memory_format=CL)
    f2 = torch.randn(B, C, H, W, generator=gen).to(dev).contiguous(memory_format=CL)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None].repeat(B, 1, 1, 1)
    coords = [(grid + 4.0 * torch.randn(B, 2, H, W, generator=gen)).to(dev) for _ in range(args.lookups)]
    ch = L * (2 * R + 1) ** 2
    dout = torch.randn(B, ch, H, W, generator=gen).to(dev)

    def hip_fwd():
        with torch.no_grad():
            blk = raft_corr.CorrBlock(f1, f2, L, R)
            return [blk(c) for c in coords]

    def torch_fwd():
        with torch.no_grad():
            pyr = torch_block(f1, f2)
            return [torch_lookup(pyr, c) for c in coords]

    def hip_fwd_bwd():
        a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
        blk = raft_corr.CorrBlock(a, b, L, R)
        torch.autograd.grad([blk(c) for c in coords], [a, b], [dout] * len(coords))

    def torch_fwd_bwd():
        a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
        pyr = torch_block(a, b)
        torch.autograd.grad([torch_lookup(pyr, c) for c in coords], [a, b], [dout] * len(coords))

    # agreement of the two arms before anything is timed
    diff = max(float((x - y).abs().max()) for x, y in zip(hip_fwd(), torch_fwd()))
    arms = {"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_fwd_bwd": hip_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd}
    times = {k: [] for k in arms}
    for _ in range(args.repeats):                       # alternated: hip, torch, hip, torch, ...
        for k, fn in arms.items():
            times[k].append(timed(fn, args.iters, args.warmup))
            torch.cuda.empty_cache()

    # per entry point, each called directly on preallocated buffers (no allocation, no autograd, one C call per sample)
    blk = raft_corr.CorrBlock(f1, f2, L, R)
    st = blk._state
    cfg, lib, cp, Cb = st.cfg, raft_corr._lib.lib(), raft_corr.ptr, raft_corr.C.byref
    stream = raft_corr._lib.stream
    n_floats, _, ws_bytes = raft_corr._sizes(cfg)
    pyr_bytes = raft_corr.pyramid_bytes(B, H, W, L)
    assert pyr_bytes == 4 * n_floats
    p_f1, p_f2 = f1.permute(0, 2, 3, 1), f2.permute(0, 2, 3, 1)
    pyr2, wsp = torch.empty(n_floats, device=dev), torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    src, dst = torch.empty(n_floats, device=dev), torch.empty(n_floats, device=dev)
    g = torch.zeros(n_floats, device=dev)
    out = torch.empty(B, ch, H, W, device=dev)
    d1, d2 = torch.empty(B, H * W, C, device=dev), torch.empty(B, H * W, C, device=dev)
    ok = lambda rc: raft_corr.check(rc, "corr_bench")
    kern = {
        "build": lambda: ok(lib.dvs_corr_build(Cb(cfg), cp(p_f1), cp(p_f2), cp(pyr2), cp(wsp), stream())),
        "copy_same_bytes": lambda: dst.copy_(src),
        "lookup_fwd": lambda: ok(lib.dvs_corr_lookup_fwd(Cb(cfg), cp(st.pyramid), cp(coords[0]), cp(out), 0, stream())),
        "lookup_bwd": lambda: ok(lib.dvs_corr_lookup_bwd(Cb(cfg), cp(coords[0]), cp(dout), 0, cp(g), stream())),
        "volume_bwd": lambda: ok(lib.dvs_corr_volume_bwd(Cb(cfg), cp(g), cp(p_f1), cp(p_f2), cp(wsp), cp(d1), cp(d2), stream())),
    }
    ktimes = {k: [timed(fn, args.iters, args.warmup) for _ in range(args.repeats)] for k, fn in kern.items()}
    del src, dst, g, out, pyr2, wsp
    build_ms = statistics.median(ktimes["build"])
    copy_ms = statistics.median(ktimes["copy_same_bytes"])
    flops = raft_corr.build_flops(B, C, H, W, L)
    tf = flops / (build_ms * 1e-3) / 1e12
    wr = pyr_bytes / (build_ms * 1e-3) / 1e9
    copy_rate = pyr_bytes / (copy_ms * 1e-3) / 1e9           # bytes written per second by a copy (it also reads as many)
    case = {
        "max_abs_diff_hip_vs_torch": diff,
        "end_to_end": {k: spread(v) for k, v in times.items()},
        "speedup_fwd": round(statistics.median(times["torch_fwd"]) / statistics.median(times["hip_fwd"]), 3),
        "speedup_fwd_bwd": round(statistics.median(times["torch_fwd_bwd"]) / statistics.median(times["hip_fwd_bwd"]), 3),
        "kernels": {k: spread(v) for k, v in ktimes.items()},
        "build": {"flops": flops, "tf_per_s": round(tf, 2), "of_fp32_matrix_peak": round(tf / PEAK_TF, 3),
                  "pyramid_bytes": pyr_bytes, "written_gb_per_s": round(wr, 1), "copy_written_gb_per_s": round(copy_rate, 1),
                  "of_copy_rate": round(wr / copy_rate, 3),
                  "nearer_bound": "fp32 matrix peak" if tf / PEAK_TF > wr / copy_rate else "store bandwidth"},
    }
    result["cases"]["B%d" % B] = case
    del blk, st
    torch.cuda.empty_cache()

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
