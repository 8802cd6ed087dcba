"""The pose fit (csrc/posefit.hip, raft_video.fit_pose, raft_video.PoseFlowStream) on the GPU, with the protocol of
tools/rigidflow_bench.py: 480x640, N = 1, 20 calls between one pair of device events, medians of --repeats windows with their minimum
and maximum.  Arms on preallocated buffers:

  entry        dvs_pose_fit at iters = 4 as the stream calls it: depth, flow and valid in, T and status out (8 launches)
  one_pass     the same with iters = 0 and the sums handed out: one accumulate and one update launch
  copy         a device copy of the bytes ONE iteration reads (depth, flow, valid)

and, per model at B = 1, a frame of PoseFlowStream beside the same RigidFlowStream, which is handed its T (graph=True, host
clock around a loop of --frames pushes that ends in a device synchronise, the arms alternated).  The streams run in ONE direction:
under the seeded weights the two flows of a bidirectional stream agree on no pixel, nothing would be judged and the accumulate
launches would return at their first branch; in one direction every pixel whose target stays in the image takes part, and the
share of judged pixels of the timed frames is recorded beside the time.  Before anything
is timed the kernel's sums are held against the NumPy restatement of tests/posefit_ref.py, and the stream's T against fit_pose and
rigid_flow composed by hand.

usage: posefit_bench.py [--frames 200] [--warmup 20] [--repeats 3] [--steps 12] [--size 480x640] [--models RAFT,SmallRAFT] [--out FILE]
Prints one JSON line and writes it to --out (default profiles/posefit_bench.json)."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posefit_bench.json"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_visual_slam_amd import _lib, raft, raft_video  # noqa: E402
import posefit_ref as P  # noqa: E402
import raft_basic_ref as RB  # noqa: E402
import raft_ref as RS  # noqa: E402
import rigidflow_ref as R  # noqa: E402

dev = torch.device("cuda:0")
H, W = (int(v) for v in args.size.split("x"))
BATCH = 20                                                  # calls per event pair
NSRC = 8                                                    # distinct frames, pushed round robin
ITERS = 4


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


result = {"shape": dict(H=H, W=W, B=1, iters=args.steps, pose_iters=ITERS), "frames_per_window": args.frames, "repeats": args.repeats,
          "calls_per_event_pair": BATCH}

# ---- the entry alone, and a copy of the bytes one iteration reads ----------------------------------------------------------------
s = P.scene(H, W, N=1, seed=9, noise=0.3, outliers=0.1)
valid_np = R.mask(H, W, 1)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
depth, K, iK, flow, valid = t(s.depth), t(s.K[None]), t(s.iK[None]), t(s.flow), t(valid_np)
eye = torch.eye(4, device=dev)[None].contiguous()
want = P.terms(s.depth, s.flow, s.K, s.iK, np.eye(4, dtype=np.float32)[None], valid_np, 1.0, s.eps)
row = raft_video.fit_pose(depth, flow, K, iK, valid=valid, iters=0, normal=True)[2].cpu().numpy()
ref = P.normal(want)
if not (np.array_equal(row[:, 29], ref[:, 29]) and (np.abs(row - ref) <= P.sum_bound(want)).all()):
    raise SystemExit("posefit_bench: dvs_pose_fit's sums differ from the restatement")
T_fit, status = raft_video.fit_pose(depth, flow, K, iK, valid=valid, iters=ITERS)
lib = _lib.lib()
need = int(lib.dvs_pose_fit_workspace(1, H, W))
ws = torch.empty(need, device=dev, dtype=torch.uint8)
T = torch.empty((1, 4, 4), device=dev)
st = torch.empty((1,), device=dev, dtype=torch.int32)
sums = torch.empty((1, 30), device=dev, dtype=torch.float64)
nbytes = (4 + 8 + 1) * H * W                                # depth, flow and valid, read once by every iteration
src = torch.empty(nbytes // 4, device=dev)
dst = torch.empty_like(src)


def entry_call(iters=ITERS, normal=None):
    _lib.check(lib.dvs_pose_fit(depth.data_ptr(), H * W, W, K.data_ptr(), iK.data_ptr(), eye.data_ptr(), flow.data_ptr(), 2 * H * W, H * W, W,
                                valid.data_ptr(), T.data_ptr(), st.data_ptr(), normal, ws.data_ptr(), need, 1, H, W, iters, 1.0, 1e-6,
                                P.EPS, _lib.stream()), "dvs_pose_fit")


ms, one, cp = [], [], []
for _ in range(args.repeats):
    ms.append(timed(entry_call))
    one.append(timed(lambda: entry_call(0, sums.data_ptr())))
    cp.append(timed(lambda: dst.copy_(src)))
med = statistics.median
result["pose_fit_%dx%d" % (H, W)] = dict(spread(ms), one_pass=spread(one), bytes_read_per_iteration=nbytes, copy_same_bytes=spread(cp),
                                         workgroups_per_image=need // 240, judged_share=round(float(ref[0, 29]) / (H * W), 4),
                                         status=int(status[0]), error_of_T=float(np.abs(T_fit.cpu().numpy() - s.T).max()),
                                         iteration_of_copy_time=round(med(ms) / ITERS / med(cp), 2),
                                         one_pass_of_copy_time=round(med(one) / med(cp), 2))


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
geo = dict(depth=depth, K=K[0], inv_K=iK[0])
T_true = t(s.T)
result["per_frame"] = {"clock": "host, around a loop of pushes that ends in a device synchronise"}
for name in [m for m in args.models.split(",") if m]:
    model = build(name)
    rigid = raft_video.RigidFlowStream(model, iters=args.steps)
    pose = raft_video.PoseFlowStream(model, iters=args.steps, pose_iters=ITERS)
    arms = {"rigid": lambda f: rigid.push(f, T=T_true, **geo), "pose": lambda f: pose.push(f, **geo)}
    pose.push(frames[0])
    r = pose.push(frames[1], **geo)
    T1 = raft_video.fit_pose(depth, r.flow_up, K, iK, valid=r.valid, iters=ITERS)[0]
    label = raft_video.rigid_flow(depth, T1, K, iK, flow=r.flow_up, valid=r.valid)[1]
    T2 = raft_video.fit_pose(depth, r.flow_up, K, iK, T0=T1, valid=(label == 1).view(torch.uint8), iters=ITERS)[0]
    if not torch.equal(r.T.view(torch.int32), T2.view(torch.int32)):
        raise SystemExit("posefit_bench: %s: the stream's T differs from fit_pose and rigid_flow composed by hand" % name)
    pose_status = r.pose_status.tolist()
    rigid.push(frames[0])
    arms["rigid"](frames[1])
    times = {k: [] for k in arms}
    for arm, push in arms.items():
        window(push, args.warmup)
    for _ in range(args.repeats):                               # alternated
        for arm, push in arms.items():
            times[arm].append(window(push, args.frames))
    m = {k: statistics.median(v) for k, v in times.items()}
    judged, last = [], []
    for k in range(NSRC + 1):                                   # the frames the windows cycle through, in their steady state
        r = pose.push(frames[k % NSRC], **geo)
        if k:
            sums = raft_video.fit_pose(depth, r.flow_up, K, iK, T0=r.T, valid=r.valid, iters=0, normal=True)[2]
            judged.append(round(float(sums[0, 29]) / (H * W), 4))
            last.append(int(r.pose_status[0]))
    result["per_frame"][name] = dict({k: spread(v) for k, v in times.items()}, pose_status_first_pair=pose_status,
                                     judged_share_per_frame=judged, pose_status_per_frame=last,
                                     pose_over_rigid=round(m["pose"] / m["rigid"], 4), added_ms=round(m["pose"] - m["rigid"], 5))
    del arms, rigid, pose, model

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
