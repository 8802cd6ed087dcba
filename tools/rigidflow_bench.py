"""Rigid flow and the moving-object label (csrc/rigidflow.hip, raft_video.rigid_flow, raft_video.RigidFlowStream) on the GPU, with the
protocol of tools/raftbidir_bench.py: 480x640, N = 1, 20 calls between one pair of device events, medians of --repeats windows with
their minimum and maximum.  Three arms on preallocated buffers:

  entry        dvs_rigid_flow as the stream calls it: depth, flow and valid in, rigid and label out (no excess)
  copy         a device copy that moves the same bytes
  aten_chain   what the entry replaces: the reference's BackprojectDepth and Project3D arithmetic (vo/learner_func.py:106-159)
               restated with torch ops on the GPU -- the pixel grid and the row of ones precomputed, as the reference's modules
               keep them -- plus the residual, the threshold and the label

and, per model at B = 1, a frame of RigidFlowStream(bidirectional=True) beside the same FlowStream without the mode (graph=True,
host clock around a loop of --frames pushes that ends in a device synchronise, the arms alternated).  Before anything is timed the
kernel is compared bit for bit with the NumPy restatement of tests/rigidflow_ref.py, and the ATen chain's labels with the kernel's.

usage: rigidflow_bench.py [--frames 200] [--warmup 20] [--repeats 3] [--steps 12] [--size 480x640] [--models RAFT,SmallRAFT] [--out FILE]
Prints one JSON line and writes it to --out (default profiles/rigidflow_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--size", default="480x640")
ap.add_argument("--models", default="RAFT,SmallRAFT")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rigidflow_bench.json"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_visual_slam_amd import _lib, raft, raft_video  # noqa: E402
import raft_basic_ref as RB  # noqa: E402
import raft_ref as RS  # noqa: E402
import rigidflow_ref as R  # noqa: E402

dev = torch.device("cuda:0")
H, W = (int(v) for v in args.size.split("x"))
BATCH = 20                                                  # calls per event pair
NSRC = 8                                                    # distinct frames, pushed round robin


def spread(vals):
    return {"median_ms": round(statistics.median(vals), 5), "min_ms": round(min(vals), 5), "max_ms": round(max(vals), 5)}


def timed(fn, iters=5, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BATCH):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / BATCH)
    return statistics.median(ms)


result = {"shape": dict(H=H, W=W, B=1, iters=args.steps), "frames_per_window": args.frames, "repeats": args.repeats,
          "calls_per_event_pair": BATCH}

# ---- the entry alone, a copy of the same bytes, the ATen chain ------------------------------------------------------------------
s = R.scene(H, W, N=1, seed=9)
flow_np, valid_np = R.measured(s, band=False), R.mask(H, W, 1)
want = R.rigid(s.depth, s.T, s.K, s.iK, flow_np, valid_np, eps=s.eps)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
depth, T, K, iK, flow, valid = t(s.depth), t(s.T), t(s.K[None]), t(s.iK[None]), t(flow_np), t(valid_np)
got = raft_video.rigid_flow(depth, T, K, iK, flow=flow, valid=valid, excess=True)
if not (np.array_equal(R.bits(got[0].cpu().numpy()), R.bits(want.rigid)) and np.array_equal(got[1].cpu().numpy(), want.label)
        and np.array_equal(R.bits(got[2].cpu().numpy()), R.bits(want.excess))):
    raise SystemExit("rigidflow_bench: dvs_rigid_flow differs from the restatement")
rigid = torch.empty((1, 2, H, W), device=dev)
label = torch.empty((1, H, W), device=dev, dtype=torch.uint8)
nbytes = (4 + 8 + 1 + 8 + 1) * H * W                        # depth, flow and valid read once; rigid and label written
src = torch.empty(nbytes // 8, device=dev)
dst = torch.empty_like(src)
lib = _lib.lib()


def entry_call():
    _lib.check(lib.dvs_rigid_flow(depth.data_ptr(), H * W, W, K.data_ptr(), iK.data_ptr(), T.data_ptr(), flow.data_ptr(), 2 * H * W, H * W, W,
                                  valid.data_ptr(), rigid.data_ptr(), None, label.data_ptr(), 1, H, W, R.ALPHA, R.BETA, R.EPS, _lib.stream()),
               "dvs_rigid_flow")


ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
grid = torch.stack([xs, ys], 0)[None]                       # [1,2,H,W]
ones = torch.ones(1, 1, H * W, device=dev)
pix = torch.cat([grid.view(1, 2, -1), ones], 1)             # the reference's pix_coords


def aten_chain():
    cam = torch.matmul(iK[:, :3, :3], pix)                                  # BackprojectDepth
    cam = torch.cat([depth.view(1, 1, -1) * cam, ones], 1)
    c = torch.matmul(torch.matmul(K, T)[:, :3, :], cam)                     # Project3D, in pixels
    p = (c[:, :2] / (c[:, 2:3] + R.EPS)).view(1, 2, H, W)
    r = p - grid
    inside = (c[:, 2].view(1, H, W) > 0) & (p[:, 0] >= 0) & (p[:, 0] <= W - 1) & (p[:, 1] >= 0) & (p[:, 1] <= H - 1)
    e = flow - r
    excess = (e * e).sum(1) - (R.ALPHA * ((flow * flow).sum(1) + (r * r).sum(1)) + R.BETA)
    judged = inside & (valid != 0) & ~torch.isnan(excess)
    return r, torch.where(judged, torch.where(excess <= 0, 1, 2), 0).to(torch.uint8)


chain = aten_chain()
chain_differs = int((chain[1].cpu().numpy() != want.label).sum())
if chain_differs > 1e-3 * H * W:
    raise SystemExit("rigidflow_bench: the ATen chain's labels differ from the kernel's on %d pixels" % chain_differs)
ms, cp, at = [], [], []
for _ in range(args.repeats):
    ms.append(timed(entry_call))
    cp.append(timed(lambda: dst.copy_(src)))
    at.append(timed(aten_chain))
med = statistics.median
result["rigid_flow_%dx%d" % (H, W)] = dict(spread(ms), bytes_moved=nbytes, copy_same_bytes=spread(cp), aten_chain=spread(at),
                                           label_share=[round(float((want.label == k).mean()), 4) for k in range(3)],
                                           aten_chain_labels_differing=chain_differs, of_copy_time=round(med(ms) / med(cp), 2),
                                           aten_chain_over_entry=round(med(at) / med(ms), 2))


# ---- per frame -------------------------------------------------------------------------------------------------------------------
def make_frames():
    """NSRC uint8 frames [1,H,W,3] on the device: a seeded smooth image that moves two pixels a frame."""
    a, _ = RS.make_images(1, H + 2 * NSRC, W + 2 * NSRC, 5)
    q = (a * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return [q[:, 2 * k:2 * k + H, 2 * k:2 * k + W].contiguous().to(dev) for k in range(NSRC)]


def build(name):
    if name == "RAFT":
        model = raft.RAFT({"small": False})
        model.load_state_dict(RB.make_weights(RB.G6["weight_seed"]), strict=True)
    else:
        model = raft.SmallRAFT()
        model.load_state_dict(RS.make_weights(RS.G6["weight_seed"]), strict=True)
    return model.to(dev).eval()


def window(push, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        push(frames[k % NSRC])
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


frames = make_frames()
geo = dict(depth=depth, T=T, K=K[0], inv_K=iK[0])
result["per_frame"] = {"clock": "host, around a loop of pushes that ends in a device synchronise"}
for name in [m for m in args.models.split(",") if m]:
    model = build(name)
    plain = raft_video.FlowStream(model, iters=args.steps, bidirectional=True)
    with_rigid = raft_video.RigidFlowStream(model, iters=args.steps, bidirectional=True)
    arms = {"bidirectional": plain.push, "bidirectional_rigid": lambda f: with_rigid.push(f, **geo)}
    for arm, push in arms.items():
        push(frames[0])
        r = push(frames[1])
        if arm == "bidirectional_rigid":
            by_hand = raft_video.rigid_flow(depth, T, K, iK, flow=r.flow_up, valid=r.valid)
            if not (torch.equal(r.rigid.view(torch.int32), by_hand[0].view(torch.int32)) and torch.equal(r.motion, by_hand[1])):
                raise SystemExit("rigidflow_bench: %s: the stream's rigid flow differs from rigid_flow called by hand" % name)
            shares = [round(float((r.motion == k).float().mean()), 4) for k in range(3)]
    times = {k: [] for k in arms}
    for arm, push in arms.items():
        window(push, args.warmup)
    for _ in range(args.repeats):                               # alternated
        for arm, push in arms.items():
            times[arm].append(window(push, args.frames))
    m = {k: statistics.median(v) for k, v in times.items()}
    result["per_frame"][name] = dict({k: spread(v) for k, v in times.items()}, motion_share=shares,
                                     rigid_over_plain=round(m["bidirectional_rigid"] / m["bidirectional"], 4),
                                     added_ms=round(m["bidirectional_rigid"] - m["bidirectional"], 5))
    del arms, plain, with_rigid, model

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
