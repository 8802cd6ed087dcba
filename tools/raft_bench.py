"""SmallRAFT end to end (model/raft/core/raft.py:66-119): this package's raft.SmallRAFT against the restatement on PyTorch-ROCm ops
(tests/raft_ref.py: F.conv2d, F.instance_norm, F.interpolate, the explicit-gather correlation block of tests/corr_ref.py) on the same
GPU with the same weights.  480x640 images, B=1 and B=12, iters=12.  One process, device events after a warm-up of every shape, the
two arms alternated:

  end to end     forward (no grad), and forward + backward (gradients of every parameter for the loss sum_k <flow_k, cot>)
  kernels        dvs_inorm_fwd / dvs_inorm_bwd at fnet's first layer [2B,240,320,32] and dvs_upflow8_fwd / _bwd at N = iters * B,
                 60x80, alone on preallocated buffers, next to a device copy that moves the same bytes

Before anything is timed the two arms run ONE forward on the same inputs, and the restatement runs once more in fp64 on the device;
the script fails unless every flow of this package is within max(OUT_TOL * max, 3 x the fp32 restatement's own error, 2 ulp) of
the fp64 flows -- the forward rule of tests/test_raft_gpu.py.

usage: raft_bench.py [--iters 5] [--warmup 1] [--repeats 3] [--steps 12] [--batches 1,12] [--out FILE]
Prints one JSON line; per number the median over the repeats of the per-repeat medians, with the min and max of those."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from deep_visual_slam_amd import _lib, raft  # noqa: E402
import raft_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--batches", default="1,12")
ap.add_argument("--size", default="480x640")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
H, W = (int(v) for v in args.size.split("x"))


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


weights = R.make_weights(1)
model = raft.SmallRAFT()
model.load_state_dict(weights)
model = model.to(dev)
ref_w = {k: v.to(dev).requires_grad_(True) for k, v in weights.items()}
params = list(model.parameters())

result = {"shape": dict(H=H, W=W, steps=args.steps), "cases": {}}
for B in (int(b) for b in args.batches.split(",")):
    im1, im2 = (t.to(dev) for t in R.make_images(B, H, W, seed=B))
    cot = torch.randn(B, 2, H, W, generator=torch.Generator().manual_seed(B + 1)).to(dev)

    def ours(grad):
        flows = model(im1, im2, iters=args.steps)
        return torch.autograd.grad(sum((f * cot).sum() for f in flows), params) if grad else flows

    def theirs(grad):
        with torch.device(dev):                             # the restatement's own torch.arange / meshgrid calls land on the GPU
            _, flows = R.small_raft(ref_w, im1, im2, args.steps)
        return torch.autograd.grad(sum((f * cot).sum() for f in flows), list(ref_w.values())) if grad else flows

    def no_grad(fn):
        with torch.no_grad():
            return fn(False)

    a, b = no_grad(ours), no_grad(theirs)
    with torch.no_grad(), torch.device(dev):
        _, c = R.small_raft({k: v.detach().double() for k, v in ref_w.items()}, im1.double(), im2.double(), args.steps)
    diffs = {}
    for k in range(args.steps):
        err, bound = float((a[k].double() - c[k]).abs().max()), max(R.OUT_TOL * float(c[k].abs().max()), R.bound(c[k], b[k]))
        diffs["flow%d" % k] = {"max_abs_err": err, "bound": bound, "max_abs": float(c[k].abs().max())}
        if err > bound:
            raise SystemExit("raft_bench: flow %d is %.3e from the fp64 restatement, bound %.3e" % (k, err, bound))
    del a, b, c
    arms = {"dvs": ours, "torch": theirs}
    times = {"%s_%s" % (arm, kind): [] for arm in arms for kind in ("fwd", "fwd_bwd")}
    for fn in arms.values():
        fn(True)                                            # every shape and path warm before the first timed region
    for _ in range(args.repeats):                           # alternated: dvs, torch, dvs, ...
        for arm, fn in arms.items():
            times[arm + "_fwd"].append(timed(lambda: no_grad(fn), args.iters, args.warmup))
        for arm, fn in arms.items():
            times[arm + "_fwd_bwd"].append(timed(lambda: fn(True), args.iters, args.warmup))
    torch.cuda.empty_cache()

    # the new entry points alone (no allocation, no autograd), and a copy that moves as many bytes (half read, half written)
    lib, st = _lib.lib(), _lib.stream
    ok = lambda rc: _lib.check(rc, "raft_bench")
    N, HW, Cn = 2 * B, (H // 2) * (W // 2), 32
    t = {k: torch.randn(N, HW, Cn, device=dev) for k in ("y", "res", "out", "dout", "dy", "dres")}
    table = torch.empty(N, 2, Cn, device=dev)
    nb = int(lib.dvs_inorm_workspace(N, HW, Cn))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    p = {k: v.data_ptr() for k, v in t.items()}
    Nf, h, w = args.steps * B, H // 8, W // 8
    flow, up = torch.randn(Nf, h, w, 2, device=dev), torch.empty(Nf, 2, H, W, device=dev)
    dflow = torch.empty_like(flow)
    elems = N * HW * Cn
    kern = {    # name: (call, bytes moved)
        "inorm_fwd_norm_relu": (lambda: ok(lib.dvs_inorm_fwd(p["y"], None, p["out"], table.data_ptr(), ws.data_ptr(), nb, N, HW, Cn, 1, 1,
                                                             st())), 4 * 3 * elems),
        "inorm_fwd_norm_relu_res": (lambda: ok(lib.dvs_inorm_fwd(p["y"], p["res"], p["out"], table.data_ptr(), ws.data_ptr(), nb, N, HW, Cn,
                                                                 1, 1, st())), 4 * 4 * elems),
        "inorm_bwd_norm_relu": (lambda: ok(lib.dvs_inorm_bwd(p["dout"], p["y"], None, table.data_ptr(), p["dy"], None, ws.data_ptr(), nb, N,
                                                             HW, Cn, 1, 1, st())), 4 * 5 * elems),
        "inorm_bwd_norm_relu_res": (lambda: ok(lib.dvs_inorm_bwd(p["dout"], p["y"], p["out"], table.data_ptr(), p["dy"], p["dres"],
                                                                 ws.data_ptr(), nb, N, HW, Cn, 1, 1, st())), 4 * 8 * elems),
        "upflow8_fwd": (lambda: ok(lib.dvs_upflow8_fwd(flow.data_ptr(), up.data_ptr(), Nf, h, w, 0, st())), 4 * (flow.numel() + up.numel())),
        "upflow8_bwd": (lambda: ok(lib.dvs_upflow8_bwd(up.data_ptr(), dflow.data_ptr(), Nf, h, w, 0, st())), 4 * (flow.numel() + up.numel())),
    }
    kernels = {}
    for name, (call, nbytes) in kern.items():
        src = torch.empty(nbytes // 8, device=dev)
        dst = torch.empty_like(src)
        ms = [timed(call, 10, 2) for _ in range(args.repeats)]
        cp = [timed(lambda: dst.copy_(src), 10, 2) for _ in range(args.repeats)]
        kernels[name] = dict(spread(ms), bytes_moved=nbytes, gb_per_s=round(nbytes / statistics.median(ms) / 1e6, 1),
                             copy_same_bytes=spread(cp), of_copy_time=round(statistics.median(ms) / statistics.median(cp), 3))
        del src, dst
    del t, flow, up, dflow
    torch.cuda.empty_cache()
    med = lambda k: statistics.median(times[k])
    result["cases"]["B%d_%dx%d" % (B, H, W)] = {
        "one_forward_difference": diffs,
        "end_to_end": {k: spread(v) for k, v in times.items()},
        "dvs_over_torch_fwd": round(med("dvs_fwd") / med("torch_fwd"), 3),
        "dvs_over_torch_fwd_bwd": round(med("dvs_fwd_bwd") / med("torch_fwd_bwd"), 3),
        "kernels": kernels,
    }

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
