"""FlowPoseNet (model/posenet_single.py:91-147): this package's posenet_single.FlowPoseNet against the restatement on PyTorch-ROCm
ops (tests/flowpose_ref.py over tests/raft_ref.py) on the same GPU with the same weights.  480x640 images, iters=12.  Device
events after a warm-up of every shape, medians of the repeats, the arms alternated:

  end to end     forward (no grad), and forward + backward (gradients of every parameter), at B=2 and at B=24 (the trainer's two
                 frame pairs at batch 12)
  memory         torch.cuda.max_memory_allocated of the B=24 forward + backward for CorrBlock and for AlternateCorrBlock
  kernels        dvs_pool_fc_fwd / dvs_pool_fc_bwd alone at N=24, 60x80, C=128, J=6 on preallocated buffers, next to a device copy
                 that moves the same bytes; 50 calls between one pair of events, so the events' own cost is a fiftieth per call.
                 Buffers of 59 and 118 MB stay in the 256 MiB Infinity Cache: both arms are cache-resident, not HBM figures
  trainer step   one MonodepthTrainer step (process_batch, backward, fused Adam with lr 0) at batch 12 with FlowPoseNet and with
                 PoseNet, each in a process of its own (a fresh child per arm and round, the arms alternated)

Before anything is timed the two arms run ONE forward on the same inputs and the restatement runs once more in fp64 on the device;
the script fails unless both outputs are within max(OUT_TOL * max, 3 x the fp32 restatement's own error, 2 ulp) of the fp64 ones
-- the forward rule of tests/test_flowpose_gpu.py.

usage: flowpose_bench.py [--iters 3] [--warmup 1] [--repeats 3] [--steps 12] [--batches 2,24] [--no-trainer] [--out FILE]
Prints one JSON line; per number the median over the repeats of the per-repeat medians, with the min and max of those."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--batches", default="2,24")
ap.add_argument("--size", default="480x640")
ap.add_argument("--trainer-batch", type=int, default=12)
ap.add_argument("--no-trainer", action="store_true")
ap.add_argument("--trainer-step", choices=["flow", "pose"], default=None, help="(internal) time one arm of the trainer step and exit")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch  # noqa: E402

from deep_visual_slam_amd import _lib, posenet_single  # noqa: E402
import flowpose_ref as P  # noqa: E402
import raft_ref as R  # noqa: E402

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


def trainer_step(kind):
    """One arm of the trainer step in this (fresh) process: prints {"ms": [per-repeat medians]}."""
    from deep_visual_slam_amd import dp, synth
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.learner_new import MonodepthTrainer
    B = args.trainer_batch
    torch.manual_seed(0)
    depth_net = DepthNet(18, pretrained=False).to(dev).train()
    if kind == "flow":
        pose_net = posenet_single.FlowPoseNet(None, iters=args.steps)
        pose_net.load_state_dict(P.make_weights(1))
    else:
        pose_net = posenet_single.PoseNet(18, pretrained=False, num_input_images=2)
    pose_net = pose_net.to(dev).train()
    flat = dp.FlatParams(dp.trainable_parameters(depth_net, pose_net))
    cfg = {"Train": dict(num_source=1, batch_size=B, img_h=H, img_w=W, smoothness_ratio=0.001, auto_mask=True, ssim_ratio=0.85,
                         min_depth=0.1, max_depth=10.0, use_compile=False)}
    trainer = MonodepthTrainer(depth_net, pose_net, cfg, dev)
    opt = dp.FusedAdam(flat, lr=0.0)                        # lr 0, as bench.py times it: the step's work without a trajectory
    sample = synth.throughput_sample(B, H, W, device=dev)

    def step():
        _, losses = trainer.process_batch(sample)
        losses["loss"].backward()
        opt.step(zero_grad=True)
        return losses

    loss = float(step()["loss"])
    if loss != loss or loss in (float("inf"), float("-inf")):
        raise SystemExit("flowpose_bench: the %s trainer step's loss is %r" % (kind, loss))
    ms = [timed(step, args.iters, args.warmup) for _ in range(args.repeats)]
    print(json.dumps({"ms": ms, "loss": loss}))


if args.trainer_step:
    trainer_step(args.trainer_step)
    sys.exit(0)

weights = P.make_weights(1)
result = {"shape": dict(H=H, W=W, steps=args.steps), "cases": {}}


def make_model(alternate):
    model = posenet_single.FlowPoseNet(None, iters=args.steps, alternate_corr=alternate)
    model.load_state_dict(weights)
    return model.to(dev)


model = make_model(False)
ref_w = {k: v.to(dev).requires_grad_(True) for k, v in weights.items()}
params = list(model.parameters())
for B in (int(b) for b in args.batches.split(",")):
    images = torch.cat(R.make_images(B, H, W, seed=B), 1).to(dev)
    gen = torch.Generator().manual_seed(B + 1)
    cot = [torch.randn(B, 1, 1, 3, generator=gen).to(dev) for _ in range(2)]
    loss_of = lambda aa, t: (aa * cot[0]).sum() + (t * cot[1]).sum()

    def ours(grad, net=model):
        out = net(images)
        return torch.autograd.grad(loss_of(*out), list(net.parameters())) if grad else out

    def theirs(grad):
        with torch.device(dev):                             # the restatement's own torch.arange / meshgrid calls land on the GPU
            out = P.flow_posenet(ref_w, images, args.steps)
        return torch.autograd.grad(loss_of(*out), list(ref_w.values())) if grad else out

    def no_grad(fn):
        with torch.no_grad():
            return fn(False)

    a, b = no_grad(ours), no_grad(theirs)
    with torch.no_grad(), torch.device(dev):
        c = P.flow_posenet({k: v.detach().double() for k, v in ref_w.items()}, images.double(), args.steps)
    diffs = {}
    for k, name in enumerate(("axisangle", "translation")):
        err, bound = float((a[k].double() - c[k]).abs().max()), max(R.OUT_TOL * float(c[k].abs().max()), R.bound(c[k], b[k]))
        diffs[name] = {"max_abs_err": err, "bound": bound, "max_abs": float(c[k].abs().max())}
        if err > bound:
            raise SystemExit("flowpose_bench: %s is %.3e from the fp64 restatement, bound %.3e" % (name, err, bound))
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
    med = lambda k: statistics.median(times[k])
    case = {"one_forward_difference": diffs, "end_to_end": {k: spread(v) for k, v in times.items()},
            "dvs_over_torch_fwd": round(med("dvs_fwd") / med("torch_fwd"), 3),
            "dvs_over_torch_fwd_bwd": round(med("dvs_fwd_bwd") / med("torch_fwd_bwd"), 3)}
    if B == 24:
        # peak memory of one training pass per correlation form, each on a fresh model after the caches are emptied
        case["max_memory_allocated_MiB"] = {}
        for name, alternate in (("CorrBlock", False), ("AlternateCorrBlock", True)):
            net = make_model(alternate)
            ours(True, net)                                 # warm: derived weights, operand caches
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ours(True, net)
            torch.cuda.synchronize()
            case["max_memory_allocated_MiB"][name] = {"peak": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
                                                      "before_the_pass": round(base / 2 ** 20, 1)}
            del net
    result["cases"]["B%d_%dx%d" % (B, H, W)] = case
    torch.cuda.empty_cache()

# the two entries alone (no allocation, no autograd), and a copy that moves as many bytes (half read, half written)
lib, st = _lib.lib(), _lib.stream
ok = lambda rc: _lib.check(rc, "flowpose_bench")
N, Pn, Cn, J = 24, (H // 8) * (W // 8), 128, 6
y, dy = torch.randn(N, Pn, Cn, device=dev), torch.empty(N, Pn, Cn, device=dev)
Wt, bt, dout = torch.randn(J, Cn, device=dev), torch.randn(J, device=dev), torch.randn(N, J, device=dev)
out, mean, dW, db = torch.empty(N, J, device=dev), torch.empty(N, Cn, device=dev), torch.empty(J, Cn, device=dev), torch.empty(J, device=dev)
nb = int(lib.dvs_pool_fc_workspace(N, Pn, Cn))
ws = torch.empty(nb, dtype=torch.uint8, device=dev)
p = lambda t: t.data_ptr()
kern = {    # name: (call, bytes moved: the small operands are left out)
    "pool_fc_fwd": (lambda: ok(lib.dvs_pool_fc_fwd(p(y), p(Wt), p(bt), p(out), p(mean), p(ws), nb, N, Pn, Cn, J, 1, 0.01, st())),
                    4 * y.numel()),
    "pool_fc_bwd": (lambda: ok(lib.dvs_pool_fc_bwd(p(dout), p(y), p(mean), p(Wt), p(dy), p(dW), p(db), N, Pn, Cn, J, 1, 0.01, st())),
                    4 * 2 * y.numel()),
}
KERNEL_BATCH = 50                                           # calls per event pair
result["kernels"] = {"shape": dict(N=N, P=Pn, C=Cn, J=J), "calls_per_event_pair": KERNEL_BATCH}
for name, (call, nbytes) in kern.items():
    src = torch.empty(nbytes // 8, device=dev)
    dst = torch.empty_like(src)
    ms, cp = [], []
    many = lambda fn: lambda: [fn() for _ in range(KERNEL_BATCH)]
    for _ in range(args.repeats):
        ms.append(timed(many(call), 10, 2) / KERNEL_BATCH)
        cp.append(timed(many(lambda: dst.copy_(src)), 10, 2) / KERNEL_BATCH)
    result["kernels"][name] = dict(spread(ms), bytes_moved=nbytes, gb_per_s=round(nbytes / statistics.median(ms) / 1e6, 1),
                                   copy_same_bytes=spread(cp), of_copy_time=round(statistics.median(ms) / statistics.median(cp), 3))
del y, dy
torch.cuda.empty_cache()

if not args.no_trainer:
    runs = {"flow": [], "pose": []}
    for _ in range(2):                                      # alternated: flow, pose, flow, pose -- a fresh process each
        for kind in runs:
            cmd = [sys.executable, os.path.abspath(__file__), "--trainer-step", kind, "--iters", str(args.iters), "--warmup",
                   str(args.warmup), "--repeats", str(args.repeats), "--steps", str(args.steps), "--size", args.size,
                   "--trainer-batch", str(args.trainer_batch)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit("flowpose_bench: the %s trainer step failed:\n%s" % (kind, r.stderr[-2000:]))
            runs[kind] += json.loads(r.stdout.strip().splitlines()[-1])["ms"]
    result["trainer_step_batch%d" % args.trainer_batch] = {
        "FlowPoseNet": spread(runs["flow"]), "PoseNet": spread(runs["pose"]),
        "flow_over_pose": round(statistics.median(runs["flow"]) / statistics.median(runs["pose"]), 3)}

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
