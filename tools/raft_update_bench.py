"""SmallRAFT's refinement loop, `lookup -> update block` x 12 on one CorrBlock (model/raft/core/raft.py:100-117), with the update
block of this package (raft_update.SmallUpdateBlock) against the same block on PyTorch-ROCm ops (tests/raft_update_ref.py: F.conv2d,
torch.cat, torch.sigmoid, torch.tanh -- what a user of the reference runs today) on the same GPU with the same weights.
hidden 96, 196 correlation planes (4 levels, radius 3), C=128 feature maps of 60x80, B=1 and B=12.  One process, device events after
warm-up of every shape, the two arms alternated:

  end to end     the 12 iterations forward (no grad), and forward + backward (gradients of net, inp and every parameter)
  no hoist       this package's forward with a fresh clone of inp per call, which defeats the hoisted context term
  kernels        the four dvs_gru_* entry points alone on preallocated buffers, next to a device copy that moves the same bytes

Before anything is timed the two arms run ONE call on the same inputs; the script fails if they differ by more than the one-step
test tolerance (2e-5 of the tensor's max).

usage: raft_update_bench.py [--iters 10] [--warmup 2] [--repeats 3] [--steps 12] [--out FILE]
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
from deep_visual_slam_amd import _lib, raft_corr, raft_update  # noqa: E402
import raft_update_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
HIDDEN, LEVELS, RADIUS, C, H, W = 96, 4, 3, 128, 60, 80
PLANES = LEVELS * (2 * RADIUS + 1) ** 2
CL = torch.channels_last


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


weights = R.make_weights(HIDDEN, PLANES, seed=1)
block = raft_update.SmallUpdateBlock(HIDDEN, LEVELS, RADIUS)
block.load_state_dict(weights)
block = block.to(dev)
ref_w = {k: v.to(dev).requires_grad_(True) for k, v in weights.items()}
params = list(block.parameters())

result = {"shape": dict(hidden=HIDDEN, planes=PLANES, C=C, H=H, W=W, steps=args.steps), "cases": {}}
for B in (1, 12):
    gen = torch.Generator().manual_seed(B)
    f1 = torch.randn(B, C, H, W, generator=gen).to(dev).contiguous(memory_format=CL)
    f2 = torch.randn(B, C, H, W, generator=gen).to(dev).contiguous(memory_format=CL)
    x, cot = R.make_case(HIDDEN, PLANES, B, H, W, seed=B + 1)
    x = {k: v.to(dev) for k, v in x.items()}
    dn, dd = cot[0][0].to(dev), cot[0][1].to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    coords0 = torch.stack([xs, ys])[None].repeat(B, 1, 1, 1).to(dev)
    corr_fn = raft_corr.CorrBlock(f1, f2, LEVELS, RADIUS)

    ours = lambda net, inp, corr, flow: block(net, inp, corr, flow)[::2]
    theirs = lambda net, inp, corr, flow: R.update_block(ref_w, net, inp, corr, flow)

    def loop(step, net, inp, fmt, fresh_inp=False):
        """raft.py:100-117 without the upsampling: (net, [delta_flow per iteration])."""
        coords1, deltas = coords0 + x["flow"], []
        for _ in range(args.steps):
            coords1 = coords1.detach()
            corr = corr_fn(coords1, memory_format=fmt)
            net, delta = step(net, inp.clone() if fresh_inp else inp, corr, coords1 - coords0)
            coords1 = coords1 + delta
            deltas.append(delta)
        return net, deltas

    def fwd(step, fmt, fresh_inp=False):
        with torch.no_grad():       # a new inp object per forward, as from a context encoder: the hoisted term is made once per call
            return loop(step, x["net"], x["inp"].detach(), fmt, fresh_inp)

    def fwd_bwd(step, fmt, leaves):
        net0, inp = x["net"].detach().requires_grad_(True), x["inp"].detach().requires_grad_(True)
        net, deltas = loop(step, net0, inp, fmt)
        loss = (net * dn).sum() + sum((d * dd).sum() for d in deltas)
        return torch.autograd.grad(loss, [net0, inp] + leaves)

    arms = {"dvs": (ours, CL, params), "torch": (theirs, None, list(ref_w.values()))}

    # one call on the same inputs: the arms must agree at the one-step test tolerance before anything is timed
    with torch.no_grad():
        corr = corr_fn(coords0 + x["flow"])
        a, b = ours(x["net"], x["inp"], corr, x["flow"]), theirs(x["net"], x["inp"], corr, x["flow"])
    diffs = {}
    for name, u, v in (("net", a[0], b[0]), ("delta_flow", a[1], b[1])):
        diffs[name] = {"max_abs_diff": float((u - v).abs().max()), "max_abs": float(v.abs().max())}
        if diffs[name]["max_abs_diff"] > R.OUT_TOL * diffs[name]["max_abs"]:
            raise SystemExit("raft_update_bench: %s of the two arms differs by %.3e (max |.| %.3e): above %.0e of the max"
                             % (name, diffs[name]["max_abs_diff"], diffs[name]["max_abs"], R.OUT_TOL))
    na, nb = fwd(ours, CL)[0], fwd(theirs, None)[0]
    diffs["net_after_%d_iterations" % args.steps] = {"max_abs_diff": float((na - nb).abs().max()), "max_abs": float(nb.abs().max())}
    del a, b, na, nb, corr

    times = {"%s_%s" % (arm, kind): [] for arm in arms for kind in ("fwd", "fwd_bwd")}
    times["dvs_fwd_no_hoist"] = []
    for fn in [lambda: fwd(ours, CL), lambda: fwd(theirs, None), lambda: fwd(ours, CL, True),
               lambda: fwd_bwd(*arms["dvs"]), lambda: fwd_bwd(*arms["torch"])]:
        fn()                                                # every shape and path warm before the first timed region
    for _ in range(args.repeats):                           # alternated: dvs, torch, dvs, ...
        for arm, (step, fmt, leaves) in arms.items():
            times[arm + "_fwd"].append(timed(lambda: fwd(step, fmt), args.iters, args.warmup))
        times["dvs_fwd_no_hoist"].append(timed(lambda: fwd(ours, CL, True), args.iters, args.warmup))
        for arm, (step, fmt, leaves) in arms.items():
            times[arm + "_fwd_bwd"].append(timed(lambda: fwd_bwd(step, fmt, leaves), args.iters, args.warmup))
    torch.cuda.empty_cache()

    # the gate entry points alone (no allocation, no autograd), and a copy that moves as many bytes (half read, half written)
    P, hd = B * H * W, HIDDEN
    buf = lambda n: torch.randn(P, n, device=dev)
    t = {k: buf(n) for k, n in dict(a_h=2 * hd, a_x=3 * hd, c=3 * hd, a_q=hd, h=hd, g=hd, d_rh=hd, z=hd, r=hd, rh=hd, q=hd,
                                    h_new=hd, dpre=3 * hd, dah=2 * hd, dq=hd, dh_a=hd, dh=hd).items()}
    p = {k: v.data_ptr() for k, v in t.items()}
    lib, st = _lib.lib(), _lib.stream
    ok = lambda rc: _lib.check(rc, "raft_update_bench")
    kern = {    # name: (call, floats moved per pixel and hidden channel)
        "gru_gates_fwd": (lambda: ok(lib.dvs_gru_gates_fwd(p["a_h"], p["a_x"], p["c"], p["h"], p["z"], p["r"], p["rh"], P, hd, st())), 10),
        "gru_blend_fwd": (lambda: ok(lib.dvs_gru_blend_fwd(p["a_q"], p["a_x"], p["c"], p["z"], p["h"], p["q"], p["h_new"], P, hd, st())), 7),
        "gru_blend_bwd": (lambda: ok(lib.dvs_gru_blend_bwd(p["g"], p["z"], p["q"], p["h"], p["dpre"], p["dah"], p["dq"], p["dh_a"], P, hd,
                                                           st())), 9),
        "gru_gates_bwd": (lambda: ok(lib.dvs_gru_gates_bwd(p["d_rh"], p["h"], p["r"], p["dh_a"], p["dpre"], p["dah"], p["dh"], P, hd, st())), 7),
    }
    kernels = {}
    for name, (call, floats) in kern.items():
        nbytes = 4 * floats * hd * P
        src = torch.empty(nbytes // 8, device=dev)
        dst = torch.empty_like(src)
        ms = [timed(call, args.iters, args.warmup) for _ in range(args.repeats)]
        cp = [timed(lambda: dst.copy_(src), args.iters, args.warmup) for _ in range(args.repeats)]
        kernels[name] = dict(spread(ms), bytes_moved=nbytes, gb_per_s=round(nbytes / statistics.median(ms) / 1e6, 1),
                             copy_same_bytes=spread(cp), of_copy_time=round(statistics.median(ms) / statistics.median(cp), 3))
        del src, dst
    del t, corr_fn
    torch.cuda.empty_cache()
    med = lambda k: statistics.median(times[k])
    result["cases"]["B%d_%dx%d" % (B, H, W)] = {
        "one_call_difference": diffs,
        "end_to_end": {k: spread(v) for k, v in times.items()},
        "dvs_over_torch_fwd": round(med("dvs_fwd") / med("torch_fwd"), 3),
        "dvs_over_torch_fwd_bwd": round(med("dvs_fwd_bwd") / med("torch_fwd_bwd"), 3),
        "no_hoist_over_hoist_fwd": round(med("dvs_fwd_no_hoist") / med("dvs_fwd"), 3),
        "kernels": kernels,
    }

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
