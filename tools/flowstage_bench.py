"""The video stage (csrc/flowstage.hip, raft_video.py) on the GPU.  One process, device events after a warm-up of every shape, medians
of the repeats:

  entries        dvs_forward_interp alone at 60x80 and 55x128 (the 1/8-resolution flows of 480x640 and Sintel 436x1024) and at the
                 cap P = 65536 (256x256); dvs_flow_radmax + dvs_flow_to_image alone at 480x640; each on preallocated buffers next to
                 a device copy that moves the same bytes, 20 calls between one pair of events.  The buffers stay in the 256 MiB
                 Infinity Cache: both arms are cache-resident, not HBM figures
  per frame      raft_video.FlowPredictor (pad, model, warm start, un-pad, colouring, all on the device) against the same model
                 followed by the host stage -- the device-to-host copies and the NumPy restatements of tests/flowstage_ref.py
                 (the reference tree is not needed) -- for raft.RAFT at 480x640, iters=12, B=1, the arms alternated; host clock
                 around a device synchronise, because the host arm's work is on the host.  The restatement's forward_interpolate is
                 a brute-force search, far slower than the reference's KD-tree: where SciPy imports, the same host stage is also
                 timed with scipy.interpolate.griddata, as the reference calls it

Before anything is timed the device results are compared with the restatements on the timed inputs (forward_interp exactly,
flow_to_image by the byte rule of tests/test_flowstage_gpu.py); the script fails otherwise.

usage: flowstage_bench.py [--iters 5] [--warmup 2] [--repeats 3] [--steps 12] [--size 480x640] [--out FILE]
Prints one JSON line; per number the median over the repeats of the per-repeat medians, with the min and max of those."""
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
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--size", default="480x640")
ap.add_argument("--out", default=None)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_visual_slam_amd import _lib, raft, raft_video  # noqa: E402
import flowstage_ref as F  # noqa: E402
import raft_basic_ref as RB  # noqa: E402
import raft_ref as RS  # noqa: E402

dev = torch.device("cuda:0")
H, W = (int(v) for v in args.size.split("x"))
lib, st = _lib.lib(), _lib.stream
ok = lambda rc: _lib.check(rc, "flowstage_bench")
p = lambda t: t.data_ptr()
BATCH = 20                                                  # calls per event pair


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


def wall(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def spread(vals):
    return {"median_ms": round(statistics.median(vals), 5), "min_ms": round(min(vals), 5), "max_ms": round(max(vals), 5)}


def beside_a_copy(call, nbytes):
    src = torch.empty(max(nbytes // 8, 1), device=dev)
    dst = torch.empty_like(src)
    many = lambda fn: lambda: [fn() for _ in range(BATCH)]
    ms, cp = [], []
    for _ in range(args.repeats):
        ms.append(timed(many(call), args.iters, args.warmup) / BATCH)
        cp.append(timed(many(lambda: dst.copy_(src)), args.iters, args.warmup) / BATCH)
    return dict(spread(ms), bytes_moved=nbytes, copy_same_bytes=spread(cp),
                of_copy_time=round(statistics.median(ms) / statistics.median(cp), 2))


def byte_rule(got, flow, what):
    img, exempt, _ = F.flow_to_image(flow, with_exempt=True)
    diff = np.abs(got.astype(np.int32) - img.astype(np.int32))
    if diff[~exempt].any() or diff.max() > 1 or exempt.mean() > F.MAX_EXEMPT:
        raise SystemExit("flowstage_bench: %s: %d bytes differ, %d of them where all variants agree, largest %d"
                         % (what, int((diff > 0).sum()), int((diff > 0)[~exempt].sum()), int(diff.max())))
    return {"bytes": int(diff.size), "differ_by_1": int((diff > 0).sum()), "exempt_share": float(exempt.mean())}


result = {"shape": dict(H=H, W=W, steps=args.steps), "calls_per_event_pair": BATCH, "entries": {}}

# ---- the entries alone ----------------------------------------------------------------------------------------------------
for h, w in ((60, 80), (55, 128), (256, 256)):
    gen = np.random.default_rng(h * w)
    flow = (gen.standard_normal((2, h, w)) * np.array([0.15 * w, 0.15 * h])[:, None, None]).astype(np.float32)
    d_flow = torch.from_numpy(flow)[None].to(dev)
    d_out = torch.empty_like(d_flow)
    call = lambda: ok(lib.dvs_forward_interp(p(d_flow), p(d_out), 1, h, w, st()))
    call()
    checked = None
    if h * w <= 8192:                                       # the brute-force restatement takes minutes at the cap
        want, margin, nvalid = F.forward_interpolate(flow)
        if not np.array_equal(d_out[0].cpu().numpy(), want):
            raise SystemExit("flowstage_bench: forward_interp %dx%d differs from the restatement" % (h, w))
        checked = {"valid_sources": nvalid, "smallest_margin": float(margin.min())}
    result["entries"]["forward_interp_%dx%d" % (h, w)] = dict(beside_a_copy(call, 2 * flow.nbytes), P=h * w, equals_restatement=checked)

gen = np.random.default_rng(7)
flow = (gen.standard_normal((2, H, W)) * 6.0).astype(np.float32)
d_flow = torch.from_numpy(flow)[None].to(dev)
d_max, d_img = torch.empty(1, device=dev), torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
radmax = lambda: ok(lib.dvs_flow_radmax(p(d_flow), H * W, W, 1, H, W, -1.0, p(d_max), st()))
colour = lambda: ok(lib.dvs_flow_to_image(p(d_flow), H * W, W, p(d_max), p(d_img), 1, H, W, -1.0, 0, st()))
radmax(), colour()
if float(d_max) != float(F.flow_radius(flow)[2]):
    raise SystemExit("flowstage_bench: radmax %r differs from the restatement's %r" % (float(d_max), float(F.flow_radius(flow)[2])))
result["entries"]["flow_radmax_%dx%d" % (H, W)] = beside_a_copy(radmax, flow.nbytes)
result["entries"]["flow_to_image_%dx%d" % (H, W)] = dict(beside_a_copy(colour, flow.nbytes + 3 * H * W),
                                                         byte_rule=byte_rule(d_img[0].cpu().numpy(), flow, "flow_to_image"))
result["entries"]["radmax_plus_image_%dx%d" % (H, W)] = beside_a_copy(lambda: (radmax(), colour()), 2 * flow.nbytes + 3 * H * W)

# ---- per frame: the predictor against the model followed by the host stage ------------------------------------------------
model = raft.RAFT({"small": False})
model.load_state_dict(RB.make_weights(RB.G6["weight_seed"]), strict=True)
model = model.to(dev).eval()
im1, im2 = (t.to(dev) for t in RS.make_images(1, H, W, 5))
pred = raft_video.FlowPredictor(model, iters=args.steps)
state = {"init": None}

try:
    from scipy import interpolate
except ImportError:
    interpolate = None


def griddata_interpolate(flow):
    """forward_interpolate with scipy's griddata(method='nearest'), the reference's own route (utils/utils.py:26-54)."""
    dx, dy = flow[0], flow[1]
    ht, wd = dx.shape
    x0, y0 = np.meshgrid(np.arange(wd), np.arange(ht))
    x1, y1 = (x0 + dx).reshape(-1), (y0 + dy).reshape(-1)
    valid = (x1 > 0) & (x1 < wd) & (y1 > 0) & (y1 < ht)
    pts = (x1[valid], y1[valid])
    fx = interpolate.griddata(pts, dx.reshape(-1)[valid], (x0, y0), method="nearest", fill_value=0)
    fy = interpolate.griddata(pts, dy.reshape(-1)[valid], (x0, y0), method="nearest", fill_value=0)
    return np.stack([fx, fy]).astype(np.float32)


def device_frame():
    return pred(im1, im2)


def host_frame(interp):
    with torch.no_grad():
        low, up = model(im1, im2, iters=args.steps, flow_init=state["init"], test_mode=True)
    state["init"] = torch.from_numpy(interp(low[0].cpu().numpy()))[None].to(dev)
    return F.flow_to_image(up[0].cpu().numpy())


def model_only():
    with torch.no_grad():
        return model(im1, im2, iters=args.steps, test_mode=True)


r = device_frame()
result["per_frame_check"] = byte_rule(r.image[0].cpu().numpy(), r.flow_up[0].cpu().numpy(), "FlowPredictor image")
want, margin, _ = F.forward_interpolate(r.flow_low[0].cpu().numpy())
result["per_frame_check"]["warm_start_equals_restatement"] = bool(np.array_equal(pred.flow_init[0].cpu().numpy(), want))
result["per_frame_check"]["warm_start_smallest_margin"] = float(margin.min())
if not result["per_frame_check"]["warm_start_equals_restatement"] and margin.min() >= 1e-9:
    raise SystemExit("flowstage_bench: the kept flow_init differs from the restatement")
arms = {"predictor": device_frame, "model_only": model_only,
        "model_plus_host_restatement": lambda: host_frame(lambda f: F.forward_interpolate(f)[0])}
if interpolate is not None:
    arms["model_plus_host_griddata"] = lambda: host_frame(griddata_interpolate)
times = {k: [] for k in arms}
for _ in range(args.repeats):                               # alternated
    for name, fn in arms.items():
        times[name].append(wall(fn, args.iters, args.warmup))
med = {k: statistics.median(v) for k, v in times.items()}
result["per_frame"] = {"model": "RAFT", "iters": args.steps, "B": 1, "clock": "host, around a device synchronise",
                       "arms": {k: spread(v) for k, v in times.items()},
                       "stage_ms": {k: round(med[k] - med["model_only"], 4) for k in arms if k != "model_only"}}

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
