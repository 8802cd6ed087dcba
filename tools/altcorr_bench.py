"""The two forms of the correlation block side by side: raft_corr.CorrBlock (all-pairs volume, pyramid, lookup) and
raft_corr.AlternateCorrBlock (on the fly, no volume).  C=128, r=3, 4 levels; feature maps 60x80 at B=1 and B=12, and 120x160 at
B=1 (the largest of the three where the all-pairs form still runs: its pyramid is 1.96 GB there, and as much again for the
gradient).  Device events after warm-up, one process, the two arms alternated:

  work per arm   one block build + `--lookups` lookups forward (no grad), and the same with its backward
  memory         rise of torch.cuda.max_memory_allocated over memory_allocated before the arm, for one forward+backward pass
  kernels        dvs_altcorr_fwd and dvs_altcorr_bwd called directly on preallocated buffers, next to dvs_corr_lookup_fwd /
                 dvs_corr_lookup_bwd of the all-pairs form (whose build and volume backward are in tools/corr_bench.py)

usage: altcorr_bench.py [--iters 5] [--warmup 2] [--repeats 3] [--lookups 12] [--out FILE]
Prints one JSON line; per number the median over the repeats of the per-repeat medians, with the min and max of those."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_visual_slam_amd import raft_corr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--lookups", type=int, default=12)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
C, R, L = 128, 3, 4
SHAPES = [(1, 60, 80), (12, 60, 80), (1, 120, 160)]
CL = torch.channels_last
ARMS = {"all_pairs": raft_corr.CorrBlock, "on_the_fly": raft_corr.AlternateCorrBlock}


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


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


result = {"shape": dict(C=C, radius=R, levels=L, lookups=args.lookups), "cases": {}}
for B, H, W in SHAPES:
    gen = torch.Generator(device="cpu").manual_seed(B + H)
    f1 = torch.randn(B, C, H, W, generator=gen).to(dev).contiguous(memory_format=CL)
    f2 = torch.randn(B, C, H, W, generator=gen).to(dev).contiguous(memory_format=CL)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys])[None].repeat(B, 1, 1, 1)
    coords = [(grid + 4.0 * torch.randn(B, 2, H, W, generator=gen)).to(dev) for _ in range(args.lookups)]
    ch = L * (2 * R + 1) ** 2
    dout = torch.randn(B, ch, H, W, generator=gen).to(dev)

    def fwd(cls):
        with torch.no_grad():
            blk = cls(f1, f2, L, R)
            return [blk(c) for c in coords]

    def fwd_bwd(cls):
        a, b = f1.detach().requires_grad_(True), f2.detach().requires_grad_(True)
        blk = cls(a, b, L, R)
        return torch.autograd.grad([blk(c) for c in coords], [a, b], [dout] * len(coords))

    # agreement of the two arms before anything is timed (one lookup's worth of outputs is kept at a time)
    diff_out = max(float((x - y).abs().max()) for x, y in zip(fwd(ARMS["all_pairs"]), fwd(ARMS["on_the_fly"])))
    ga, gb = fwd_bwd(ARMS["all_pairs"]), fwd_bwd(ARMS["on_the_fly"])
    diff_grad = max(float((x - y).abs().max()) for x, y in zip(ga, gb))
    del ga, gb
    times = {"%s_%s" % (arm, kind): [] for arm in ARMS for kind in ("fwd", "fwd_bwd")}
    for _ in range(args.repeats):                           # alternated: all-pairs, on the fly, all-pairs, ...
        for kind, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
            for arm, cls in ARMS.items():
                times["%s_%s" % (arm, kind)].append(timed(lambda: fn(cls), args.iters, args.warmup))
                torch.cuda.empty_cache()
    memory = {arm: {"fwd_bwd_peak_rise_bytes": peak_rise(lambda: fwd_bwd(cls)), "fwd_peak_rise_bytes": peak_rise(lambda: fwd(cls))}
              for arm, cls in ARMS.items()}

    # the entry points alone, on preallocated buffers (no allocation, no autograd)
    lib, cp, Cb, stream = raft_corr._lib.lib(), raft_corr.ptr, raft_corr.C.byref, raft_corr._lib.stream
    ok = lambda rc: raft_corr.check(rc, "altcorr_bench")
    out = torch.empty(B, ch, H, W, device=dev)
    alt = raft_corr.AlternateCorrBlock(f1, f2, L, R)
    st, pooled = alt._state, alt._pooled
    d1, d2, dp = (torch.zeros(B, H * W, C, device=dev), torch.zeros(B, H * W, C, device=dev), torch.zeros_like(pooled))
    kern = {
        "altcorr_fwd": lambda: ok(lib.dvs_altcorr_fwd(Cb(st.cfg), cp(st.f1), cp(st.f2), cp(pooled), cp(st.workspace), cp(coords[0]),
                                                      cp(out), 0, stream())),
        "altcorr_bwd": lambda: ok(lib.dvs_altcorr_bwd(Cb(st.cfg), cp(st.f1), cp(st.f2), cp(pooled), cp(st.workspace), cp(coords[0]),
                                                      cp(dout), 0, cp(d1), cp(d2), cp(dp), stream())),
    }
    ktimes = {k: [timed(fn, args.iters, args.warmup) for _ in range(args.repeats)] for k, fn in kern.items()}
    del alt, st, pooled, d1, d2, dp
    blk = raft_corr.CorrBlock(f1, f2, L, R)
    cst = blk._state
    g = torch.zeros_like(cst.pyramid)
    kern = {
        "corr_lookup_fwd": lambda: ok(lib.dvs_corr_lookup_fwd(Cb(cst.cfg), cp(cst.pyramid), cp(coords[0]), cp(out), 0, stream())),
        "corr_lookup_bwd": lambda: ok(lib.dvs_corr_lookup_bwd(Cb(cst.cfg), cp(coords[0]), cp(dout), 0, cp(g), stream())),
    }
    ktimes.update({k: [timed(fn, args.iters, args.warmup) for _ in range(args.repeats)] for k, fn in kern.items()})
    del blk, cst, g, out
    torch.cuda.empty_cache()
    med = lambda k: statistics.median(times[k])
    result["cases"]["B%d_%dx%d" % (B, H, W)] = {
        "max_abs_diff_outputs": diff_out, "max_abs_diff_gradients": diff_grad,
        "end_to_end": {k: spread(v) for k, v in times.items()},
        "on_the_fly_over_all_pairs_fwd": round(med("on_the_fly_fwd") / med("all_pairs_fwd"), 3),
        "on_the_fly_over_all_pairs_fwd_bwd": round(med("on_the_fly_fwd_bwd") / med("all_pairs_fwd_bwd"), 3),
        "memory": memory,
        "pyramid_bytes": raft_corr.pyramid_bytes(B, H, W, L), "altcorr_bytes": raft_corr.altcorr_bytes(B, C, H, W, L, R),
        "kernels": {k: spread(v) for k, v in ktimes.items()},
    }

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
