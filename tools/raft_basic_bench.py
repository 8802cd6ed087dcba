"""Full-size RAFT end to end (model/raft/core/raft.py:122-244): this package's raft.RAFT against the restatement on PyTorch-ROCm ops
(tests/raft_basic_ref.py: F.conv2d with the (1,5) / (5,1) filters, F.instance_norm, the written-out BatchNorm and convex upsampling,
the explicit-gather correlation block of tests/corr_ref.py) on the same GPU with the same weights, BatchNorm on its running
statistics (eval mode: inference, and training under freeze_bn).  480x640 images, B=1 and B=4, iters=12.  One process, device
events after a warm-up of every shape, the two arms alternated:

  end to end     forward (no grad), and forward + backward (gradients of every parameter for the loss sum_k <flow_k, cot>), with
                 torch.cuda.max_memory_allocated of each arm's forward + backward
  kernels        dvs_convex_up_fwd / _bwd at N = iters * B and dvs_shift_stack_fwd / _bwd at [B,60,80,128], both axes, alone on
                 preallocated buffers, next to a device copy that moves the same bytes
  upsampling     all iterations' forward upsampling as RAFT.forward does it (torch.cat of the masks, one launch) and as one launch
                 per iteration without the copy
  iteration      one BasicUpdateBlock forward (no grad, mask head included) and the six shift-stack launches it contains, alone:
                 their share of the iteration

Before anything is timed the two arms run ONE forward on the same inputs, and the restatement runs once more in fp64 on the device;
the script fails unless every flow of this package is within max(OUT_TOL * max, 3 x the fp32 restatement's own error, 2 ulp) of
the fp64 flows -- the forward rule of tests/test_raft_basic_gpu.py.

usage: raft_basic_bench.py [--iters 5] [--warmup 1] [--repeats 3] [--steps 12] [--batches 1,4] [--out FILE]
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
import raft_basic_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--batches", default="1,4")
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
model = raft.RAFT({"small": False})
model.load_state_dict(weights, strict=True)
model = model.to(dev).eval()
pk = [k for k in R.parameter_keys(weights) if ".downsample.1." not in k]
ref_w = {k: (v.to(dev).requires_grad_(k in pk) if R.is_float_key(k) else v.to(dev)) for k, v in weights.items()}
params = list(model.parameters())

result = {"shape": dict(H=H, W=W, steps=args.steps), "cases": {}}
for B in (int(b) for b in args.batches.split(",")):
    im1, im2 = (t.to(dev) for t in R.S.make_images(B, H, W, seed=B))
    cot = torch.randn(B, 2, H, W, generator=torch.Generator().manual_seed(B + 1)).to(dev)

    def ours(grad):
        flows = model(im1, im2, iters=args.steps)
        return torch.autograd.grad(sum((f * cot).sum() for f in flows), params) if grad else flows

    def theirs(grad):
        with torch.device(dev):                             # the restatement's own torch.arange / meshgrid calls land on the GPU
            _, flows = R.basic_raft(ref_w, im1, im2, args.steps)
        return torch.autograd.grad(sum((f * cot).sum() for f in flows), [ref_w[k] for k in pk]) if grad else flows

    def no_grad(fn):
        with torch.no_grad():
            return fn(False)

    a, b = no_grad(ours), no_grad(theirs)
    with torch.no_grad(), torch.device(dev):
        _, c = R.basic_raft({k: (v.detach().double() if R.is_float_key(k) else v) for k, v in ref_w.items()}, im1.double(), im2.double(),
                            args.steps)
    diffs = {}
    for k in range(args.steps):
        err, bound = float((a[k].double() - c[k]).abs().max()), max(R.OUT_TOL * float(c[k].abs().max()), R.bound(c[k], b[k]))
        diffs["flow%d" % k] = {"max_abs_err": err, "bound": bound, "max_abs": float(c[k].abs().max())}
        if err > bound:
            raise SystemExit("raft_basic_bench: flow %d is %.3e from the fp64 restatement, bound %.3e" % (k, err, bound))
    del a, b, c
    arms = {"dvs": ours, "torch": theirs}
    times = {"%s_%s" % (arm, kind): [] for arm in arms for kind in ("fwd", "fwd_bwd")}
    peak = {}
    for arm, fn in arms.items():                            # every shape and path warm before the first timed region
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn(True)
        torch.cuda.synchronize()
        peak[arm] = {"max_memory_allocated_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
                     "allocated_before_mib": round(base / 2 ** 20, 1)}
    for _ in range(args.repeats):                           # alternated: dvs, torch, dvs, ...
        for arm, fn in arms.items():
            times[arm + "_fwd"].append(timed(lambda: no_grad(fn), args.iters, args.warmup))
        for arm, fn in arms.items():
            times[arm + "_fwd_bwd"].append(timed(lambda: fn(True), args.iters, args.warmup))
    torch.cuda.empty_cache()

    # the new entry points alone (no allocation, no autograd), and a copy that moves as many bytes (half read, half written)
    lib, st = _lib.lib(), _lib.stream
    ok = lambda rc: _lib.check(rc, "raft_basic_bench")
    Nf, h, w, Cn = args.steps * B, H // 8, W // 8, 128
    flow, mask, up = torch.randn(Nf, 2, h, w, device=dev), torch.randn(Nf, h, w, 576, device=dev), torch.randn(Nf, 2, H, W, device=dev)
    dflow, dmask = torch.empty_like(flow), torch.empty_like(mask)
    nb = int(lib.dvs_convex_up_workspace(Nf, h, w))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    x, x5 = torch.randn(B, h, w, Cn, device=dev), torch.randn(B, h, w, 5 * Cn, device=dev)
    dx = torch.empty_like(x)
    fl, mk, upn = 4 * flow.numel(), 4 * mask.numel(), 4 * up.numel()
    kern = {    # name: (call, bytes moved)
        "convex_up_fwd": (lambda: ok(lib.dvs_convex_up_fwd(flow.data_ptr(), mask.data_ptr(), up.data_ptr(), Nf, h, w, 0.25, st())),
                          fl + mk + upn),
        "convex_up_bwd": (lambda: ok(lib.dvs_convex_up_bwd(up.data_ptr(), flow.data_ptr(), mask.data_ptr(), dflow.data_ptr(),
                                                           dmask.data_ptr(), ws.data_ptr(), nb, Nf, h, w, 0.25, st())),
                          upn + 2 * fl + 2 * mk + 2 * nb),
    }
    for axis in (0, 1):
        kern["shift_stack_fwd_axis%d" % axis] = ((lambda axis=axis: ok(lib.dvs_shift_stack_fwd(x.data_ptr(), x5.data_ptr(), B, h, w, Cn, axis,
                                                                                              st()))), 4 * (x.numel() + x5.numel()))
        kern["shift_stack_bwd_axis%d" % axis] = ((lambda axis=axis: ok(lib.dvs_shift_stack_bwd(x5.data_ptr(), dx.data_ptr(), B, h, w, Cn, axis,
                                                                                              st()))), 4 * (x.numel() + x5.numel()))
    kernels = {}
    for name, (call, nbytes) in kern.items():
        src = torch.empty(nbytes // 8, device=dev)
        dst = torch.empty_like(src)
        ms = [timed(call, 10, 2) for _ in range(args.repeats)]
        cp = [timed(lambda: dst.copy_(src), 10, 2) for _ in range(args.repeats)]
        kernels[name] = dict(spread(ms), bytes_moved=nbytes, gb_per_s=round(nbytes / statistics.median(ms) / 1e6, 1),
                             copy_same_bytes=spread(cp), of_copy_time=round(statistics.median(ms) / statistics.median(cp), 3))
        del src, dst

    # RAFT.forward upsamples every iteration in ONE launch, which first copies the `steps` masks side by side (torch.cat): that
    # against `steps` launches on the masks where they are
    m_parts, f_parts, u_parts = (list(t.view(args.steps, B, *t.shape[1:]).unbind(0)) for t in (mask, flow, up))

    def cat_then_one_launch():
        m, f = torch.cat(m_parts, 0), torch.cat(f_parts, 0)
        ok(lib.dvs_convex_up_fwd(f.data_ptr(), m.data_ptr(), up.data_ptr(), Nf, h, w, 0.25, st()))

    def one_launch_per_iteration():
        for m, f, u in zip(m_parts, f_parts, u_parts):
            ok(lib.dvs_convex_up_fwd(f.data_ptr(), m.data_ptr(), u.data_ptr(), B, h, w, 0.25, st()))

    upsampling = {"cat_then_one_launch": spread([timed(cat_then_one_launch, 10, 2) for _ in range(args.repeats)]),
                  "one_launch_per_iteration": spread([timed(one_launch_per_iteration, 10, 2) for _ in range(args.repeats)])}
    del m_parts, f_parts, u_parts

    # one iteration of the update block, and the six shift-stack launches it contains
    gen = torch.Generator().manual_seed(3)
    t = {"net": torch.tanh(torch.randn(B, 128, h, w, generator=gen)), "inp": torch.relu(torch.randn(B, 128, h, w, generator=gen)),
         "corr": torch.randn(B, R.PLANES, h, w, generator=gen), "flow": torch.randn(B, 2, h, w, generator=gen)}
    t = {k: v.to(dev).contiguous(memory_format=torch.channels_last) for k, v in t.items()}

    def one_iteration():
        with torch.no_grad():
            model.update_block(t["net"], t["inp"], t["corr"], t["flow"])

    def six_stacks():
        for axis in (0, 1):
            for _ in range(3):
                ok(lib.dvs_shift_stack_fwd(x.data_ptr(), x5.data_ptr(), B, h, w, Cn, axis, st()))

    it_ms = [timed(one_iteration, 10, 2) for _ in range(args.repeats)]
    st_ms = [timed(six_stacks, 10, 2) for _ in range(args.repeats)]
    iteration = {"update_block_fwd": spread(it_ms), "six_shift_stacks_fwd": spread(st_ms),
                 "stack_share_of_iteration": round(statistics.median(st_ms) / statistics.median(it_ms), 3)}
    del t, flow, mask, up, dflow, dmask, ws, x, x5, dx
    torch.cuda.empty_cache()
    med = lambda k: statistics.median(times[k])
    result["cases"]["B%d_%dx%d" % (B, H, W)] = {
        "one_forward_difference": diffs,
        "end_to_end": {k: spread(v) for k, v in times.items()},
        "memory_fwd_bwd": peak,
        "dvs_over_torch_fwd": round(med("dvs_fwd") / med("torch_fwd"), 3),
        "dvs_over_torch_fwd_bwd": round(med("dvs_fwd_bwd") / med("torch_fwd_bwd"), 3),
        "kernels": kernels,
        "upsampling_all_iterations_fwd": upsampling,
        "iteration": iteration,
    }

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
