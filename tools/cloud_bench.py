"""ms/frame of the inference loop INCLUDING its output stage (world pose + coloured point cloud ready to publish), 480x640,
batch 1, one process, the arms alternated in blocks inside the same run, every frame device-synchronised:

  F   inference.FramePredictor (graph) alone                                   -- the 1.27 ms of DESIGN.md section 9
  A   F, then what a caller had to do before: D2H of depth, image and T, the ROS2 node's host work
      (visualizer_node.py:128-191) restated in numpy with the meshgrid hoisted out of the loop, tobytes()
  B   inference.CloudPredictor (graph, dense, world frame) up to the as_records view after its event
  Cf  B in compact mode (z_range keeping about half the pixels), whole capacity copied, sliced on the host
  Cc  the same, `count` copied first, then count[b] records

usage: cloud_bench.py [--frames 200] [--warmup 20] [--arms F,A,B,Cf,Cc] [--out FILE]
Prints one JSON line: ms/frame per arm and repeat (two repeats: their difference is the run-to-run spread), B - F and
A - F, the D2H time and bytes of one dense frame."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deep_visual_slam_amd import inference, pointcloud  # noqa: E402
from deep_visual_slam_amd.depthnet import DepthNet  # noqa: E402
from deep_visual_slam_amd.posenet_single import PoseNet  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--arms", default="F,A,B,Cf,Cc")
ap.add_argument("--out", default=None)
args = ap.parse_args()
arms = args.arms.split(",")

torch.set_num_threads(min(16, os.cpu_count()))
dev = torch.device("cuda:0")
H, W = 480, 640
torch.manual_seed(0)
dn, pn = DepthNet(18, pretrained=False).to(dev), PoseNet(18, pretrained=False, num_input_images=2).to(dev)
inference.prepare(dn, pn, scales=(0,))
frames = [(torch.rand(1, 3, H, W, device=dev), torch.rand(1, 6, H, W, device=dev)) for _ in range(4)]
Kd = torch.tensor([[[0.58 * W, 0, 0.5 * W, 0], [0, 0.77 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], device=dev)
zero = (torch.zeros_like(frames[0][0]), torch.zeros_like(frames[0][1]))

fp = inference.FramePredictor(dn, pn, *zero)
with torch.no_grad():
    z_mid = float(fp(*frames[0])[1].median())                    # compact arms keep about half the pixels
run = {}

if "F" in arms:
    def arm_f(x, x6):
        fp(x, x6)
        torch.cuda.synchronize()
    run["F"] = arm_f

if "A" in arms:
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    u, v = u.flatten(), v.flatten()
    state = {"world": np.eye(4, dtype=np.float32)}

    def arm_a(x, x6):
        T, depth, _ = fp(x, x6)
        K = Kd[0].cpu().numpy()
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        T = T.cpu().numpy()[0]
        depth_map = depth.cpu().numpy()[0, 0]
        state["world"] = world = state["world"] @ T
        z = depth_map.flatten()
        pts = np.vstack(((u - cx) * z / fx, (v - cy) * z / fy, z)).T
        img = (x * 255.0).clamp(0, 255).byte()[0].cpu().numpy().transpose(1, 2, 0)     # vo/predict.py:93-94
        colors = img.reshape(-1, 3)
        rgb = ((colors[:, 0].astype(np.uint32) << 16) | (colors[:, 1].astype(np.uint32) << 8)
               | colors[:, 2].astype(np.uint32)).view(np.float32)
        pc = np.zeros(pts.shape[0], dtype=pointcloud.RECORD_DTYPE)
        pc["x"], pc["y"], pc["z"], pc["rgb"] = pts[:, 0], pts[:, 1], pts[:, 2], rgb
        data = pc.tobytes()
        rot = world[:3, :3]
        qw = np.sqrt(1 + rot[0, 0] + rot[1, 1] + rot[2, 2]) / 2
        q = ((rot[2, 1] - rot[1, 2]) / (4 * qw), (rot[0, 2] - rot[2, 0]) / (4 * qw), (rot[1, 0] - rot[0, 1]) / (4 * qw), qw)
        return data, q
    run["A"] = arm_a


def cloud_arm(**kw):
    cp = inference.CloudPredictor(dn, pn, *zero, Kd, **kw)

    def arm(x, x6):
        f = cp(x, x6)
        r = f.records                                               # waits for this frame's event
        torch.cuda.synchronize()
        return r, f.tq
    return arm, cp


cps = {}
for name, kw in (("B", {}), ("Cf", dict(z_range=(0.0, z_mid), d2h="full")), ("Cc", dict(z_range=(0.0, z_mid), d2h="count"))):
    if name in arms:
        run[name], cps[name] = cloud_arm(**kw)

block = 25
times = {a: [[], []] for a in run}
for a in run:                                                       # warm-up, every arm
    for i in range(args.warmup):
        run[a](*frames[i % 4])
for rep in range(2):
    done = 0
    while done < args.frames:
        n = min(block, args.frames - done)
        for a in run:                                               # the arms take turns, 25 frames each
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                run[a](*frames[i % 4])
            times[a][rep].append((time.perf_counter() - t0, n))
        done += n

res = {"image": "%dx%d" % (W, H), "batch": 1, "frames": args.frames, "warmup": args.warmup, "host_threads": torch.get_num_threads()}
ms = {}
for a, reps in times.items():
    per = [1e3 * sum(t for t, _ in r) / sum(n for _, n in r) for r in reps]
    ms[a] = sum(per) / 2
    res[a + "_ms"] = [round(p, 4) for p in per]
if "F" in ms:
    for a in ms:
        if a != "F":
            res[a + "_minus_F_ms"] = round(ms[a] - ms["F"], 4)
if "Cf" in cps:
    res["compact_kept"] = int(cps["Cf"](*frames[0]).count[0])
    res["compact_z_hi"] = round(z_mid, 5)
if "B" in cps:                                                      # the D2H alone: device events around one frame's copies
    cp = cps["B"]
    host = torch.zeros_like(cp.d_records, device="cpu").pin_memory()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(30):
        e0.record()
        host.copy_(cp.d_records, non_blocking=True)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    res["d2h_ms"] = round(float(np.median(ts[5:])), 4)
    res["d2h_bytes"] = host.numel() * 4 + 4 + 7 * 4 + 64
    res["d2h_GBps"] = round(host.numel() * 4 / (res["d2h_ms"] * 1e-3) / 1e9, 2)
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
