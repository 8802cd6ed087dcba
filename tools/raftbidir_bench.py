"""Bidirectional RAFT on a frame stream (raft.refine_pair, csrc/flowcons.hip, raft_video.FlowStream(bidirectional=True)) on the GPU:
what the backward flow and the two consistency masks cost per frame, for raft.RAFT and raft.SmallRAFT at B = 1.  The protocol of
tools/raftstream_bench.py: one process, the arms alternated, a host clock around a loop of --frames pushes that ends in a device
synchronise, medians of --repeats windows after a warm-up loop:

  one_graph / one_eager     today's raft_video.FlowStream (forward pair only), graph=True (the default) and graph=False
  two_loops                 both directions composed by hand, eagerly: the frame encoded once, model.refine(previous, current) and
                            model.refine(current, previous) at batch N, a kept flow for each, raft_video.flow_consistency, the picture
  both_eager / both_graph   raft_video.FlowStream(bidirectional=True): ONE loop at batch 2N, graph=False and graph=True

and dvs_flow_consistency alone on preallocated buffers (both masks, no excess) beside a device copy that moves the same bytes, 20
calls between one pair of events.  Before anything is timed the kernel is compared bit for bit with the NumPy restatement of
tests/flowcons_ref.py, and the first pair's forward flow of every arm with one_graph's.

usage: raftbidir_bench.py [--frames 200] [--warmup 20] [--repeats 3] [--steps 12] [--size 480x640] [--out FILE]
Prints one JSON line and writes it to --out (default profiles/raftbidir_bench.json)."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raftbidir_bench.json"))
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deep_visual_slam_amd import _lib, raft, raft_video  # noqa: E402
import flowcons_ref as R  # noqa: E402
import raft_basic_ref as RB  # noqa: E402
import raft_ref as RS  # noqa: E402

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


def make_frames():
    """NSRC uint8 frames [1,H,W,3] on the device: a seeded smooth image that moves two pixels a frame."""
    a, _ = RS.make_images(1, H + 2 * NSRC, W + 2 * NSRC, 5)
    q = (a * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return [q[:, 2 * k:2 * k + H, 2 * k:2 * k + W].contiguous().to(dev) for k in range(NSRC)]


frames = make_frames()
result = {"shape": dict(H=H, W=W, B=1, iters=args.steps), "frames_per_window": args.frames, "repeats": args.repeats,
          "clock": "host, around a loop of pushes that ends in a device synchronise", "calls_per_event_pair": BATCH}

# ---- the consistency entry alone ----------------------------------------------------------------------------------------------
a_np, b_np = R.smooth(H, W)
b_np = (b_np + np.random.default_rng(3).standard_normal(b_np.shape).astype(np.float32) * np.float32(0.3)).astype(np.float32)
fa, fb = torch.from_numpy(a_np).to(dev), torch.from_numpy(b_np).to(dev)
got = raft_video.flow_consistency(fa, fb, excess=True)
want = R.consistency(a_np, b_np)
for i in range(2):
    if not (np.array_equal(got[i].cpu().numpy(), want[i].valid) and np.array_equal(R.bits(got[2 + i].cpu().numpy()), R.bits(want[i].excess))):
        raise SystemExit("raftbidir_bench: dvs_flow_consistency differs from the restatement")
valid = torch.empty((2, 1, H, W), device=dev, dtype=torch.uint8)
nbytes = 2 * 2 * 4 * H * W + 2 * H * W                      # both flows read once, both masks written (the taps hit the cache)
src = torch.empty(nbytes // 8, device=dev)
dst = torch.empty_like(src)
lib = _lib.lib()


def consistency_call():
    _lib.check(lib.dvs_flow_consistency(fa.data_ptr(), 2 * H * W, H * W, W, fb.data_ptr(), 2 * H * W, H * W, W, valid[0].data_ptr(),
                                        valid[1].data_ptr(), None, None, 1, H, W, R.ALPHA, R.BETA, _lib.stream()), "dvs_flow_consistency")


ms, cp = [], []
for _ in range(args.repeats):
    ms.append(timed(consistency_call))
    cp.append(timed(lambda: dst.copy_(src)))
result["consistency_%dx%d" % (H, W)] = dict(spread(ms), bytes_moved=nbytes, copy_same_bytes=spread(cp),
                                            valid_share=[round(float(w.valid.mean()), 4) for w in want],
                                            of_copy_time=round(statistics.median(ms) / statistics.median(cp), 2))


# ---- per frame -----------------------------------------------------------------------------------------------------------------
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


class TwoLoops:
    """Both directions as two refine calls of batch N around one encoder pass per frame, composed by hand."""

    def __init__(self, model, iters):
        self.model, self.iters = model, iters
        self.padder = raft_video.InputPadder((H, W))
        self.prev, self.kept = None, [None, None]

    def _refine(self, f1, f2, flow_init):
        if isinstance(self.model, raft.RAFT):
            return self.model.refine(f1, f2, iters=self.iters, flow_init=flow_init, test_mode=True)
        up = self.model.refine(f1, f2, iters=self.iters, flow_init=flow_init, last_only=True)[-1]
        return self.model.flow_low[-1], up

    @torch.no_grad()
    def push(self, frame):
        feat = self.model.encode_frame(raft_video.frame_ingest(frame, self.padder._pad))
        prev, self.prev = self.prev, feat
        if prev is None:
            return None
        ups = []
        for i, (f1, f2) in enumerate(((prev, feat), (feat, prev))):
            low, up = self._refine(f1, f2, self.kept[i])
            self.kept[i] = raft_video.forward_interpolate(low)
            ups.append(self.padder.unpad(up))
        valid, valid_bw = raft_video.flow_consistency(ups[0], ups[1])
        return raft_video.FlowFrame(None, ups[0], raft_video.flow_to_image(ups[0]), None, None, ups[1], valid, valid_bw)


result["per_frame"] = {}
for name in args.models.split(","):
    model = build(name)
    S = raft_video.FlowStream
    arms = {"one_graph": S(model, iters=args.steps).push, "one_eager": S(model, iters=args.steps, graph=False).push,
            "two_loops": TwoLoops(model, args.steps).push,
            "both_eager": S(model, iters=args.steps, graph=False, bidirectional=True).push,
            "both_graph": S(model, iters=args.steps, bidirectional=True).push}
    # every arm on the same two frames, cold: the forward flow against one_graph's, the backward flow and the masks against
    # two_loops'.  Over `steps` iterations of seeded (untrained) weights the last-bit differences of the split-K convolutions'
    # float atomics grow (tools/raftstream_bench.py), so only a gross difference stops the run
    first = {}
    for arm, push in arms.items():
        push(frames[0])
        r = push(frames[1])
        first[arm] = {k: getattr(r, k).clone() for k in ("flow_up", "flow_up_bw", "valid", "valid_bw") if getattr(r, k) is not None}
    scale = float(first["one_graph"]["flow_up"].abs().max())
    check = {arm: round(float((first[arm]["flow_up"] - first["one_graph"]["flow_up"]).abs().max()) / scale, 8) for arm in arms}
    scale_bw = float(first["two_loops"]["flow_up_bw"].abs().max())
    for arm in ("both_eager", "both_graph"):
        check[arm + "_backward_vs_two_loops"] = round(float((first[arm]["flow_up_bw"] - first["two_loops"]["flow_up_bw"]).abs().max()) / scale_bw, 8)
        check[arm + "_mask_bytes_differing_from_two_loops"] = int((first[arm]["valid"] != first["two_loops"]["valid"]).sum()
                                                                  + (first[arm]["valid_bw"] != first["two_loops"]["valid_bw"]).sum())
    check["valid_share"] = [round(float(first["both_graph"][k].float().mean()), 4) for k in ("valid", "valid_bw")]
    if max(check[a] for a in arms) > 1e-2:
        raise SystemExit("raftbidir_bench: %s: the arms disagree: %r" % (name, check))
    times = {k: [] for k in arms}
    for arm, push in arms.items():
        window(push, args.warmup)
    for _ in range(args.repeats):                               # alternated
        for arm, push in arms.items():
            times[arm].append(window(push, args.frames))
    med = {k: statistics.median(v) for k, v in times.items()}
    ratio = lambda a, b: round(med[a] / med[b], 4)
    result["per_frame"][name] = dict({k: spread(v) for k, v in times.items()}, first_pair_relative_difference=check,
                                     both_graph_over_one_graph=ratio("both_graph", "one_graph"),
                                     both_eager_over_one_eager=ratio("both_eager", "one_eager"),
                                     both_eager_over_two_loops=ratio("both_eager", "two_loops"),
                                     both_graph_over_two_loops=ratio("both_graph", "two_loops"))
    del arms, model

line = json.dumps(result)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
