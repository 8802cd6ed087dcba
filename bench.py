"""VO training-step throughput on MI355X (BASELINE.json metric: frames/s of 3-frame 640x480 snippets).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python bench.py --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A step = zero_grad -> DepthNet + 2x PoseNet forward -> fused 4-scale view-synthesis loss -> backward
-> [bucketed RCCL gradient all-reduce] -> Adam, on one batch of synthetic triplets already resident in
HBM.  Default workload: BASELINE.json configs[2]/[3] per GPU (batch 12, 4 scales,
ResNet-18, fp32); `--config c2` selects configs[1] (batch 4, single scale).  Weak scaling: the
per-GPU batch is fixed, `value` is the whole-job frames/s = 3 * B * N / t_step (max over ranks).  The Adam pass runs at
lr 0 (TIMED_LR): the same work, but every step computes from the seeded weights, so runs are comparable output for output.

A plain run only sets up, warms up, times the K steps, writes the last timed step's outputs when `--dump-outputs DIR`
is given (dump_outputs below) and prints one JSON line.  `ms_per_step` is the mean over the K timed steps (what `value`
is computed from); `median_ms_per_step` is the median of the K per-step intervals taken from events recorded on the main
stream (BASELINE.md section 2 defines the metric on the median of >= 50 steps: the default K).

`--full` adds everything else, after the timed region unless stated: `loss_check` (the first-step loss against the
committed oracle value, tests/golden/bench_loss.json; checked before the warm-up), `roofline` (dominant hand-written kernel
class; its launches are HIP-event timed over 5 further SINGLE-STREAM steps -- the timed steps overlap four streams, where
an event pair would measure how long a kernel shared the chip), `measured_peaks`, and at N=1 `cpu_baseline` (the
oracle's PyTorch-CPU restatement of the same step at the same batch), `stock_caller` (the literal vo/train.py:173-199
sequence: per-parameter torch.optim.Adam, zero_grad(set_to_none=True), five .detach().cpu() per step) and
`other_configs` (configs[1], the bf16 mode, configs[0] inference, configs[4] Depth-Anything-V2).  The `--no-*` switches
drop single legs of a `--full` run.
"""
import argparse
import json
import os
import sys
import time

if int(os.environ.get("WORLD_SIZE", "1")) > 1 and os.environ.get("DVS_BENCH_REHEARSE") != "1":
    # One rank per GPU: the step uses four compute streams and the all-reduce a fifth.  HIP maps a process's streams onto
    # GPU_MAX_HW_QUEUES hardware queues (default 4) and streams that share a queue serialise, so give the all-reduce a queue
    # of its own (4 / 6 / 8 queues measured neutral for the single-GPU step, gpurun_out sweep).  Set
    # before torch loads the HIP runtime, which reads its flags once.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "6")

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H, W = 480, 640
HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
MFMA_F32_PEAK_TFLOPS = 157.3    # dense fp32 MFMA peak
# compulsory loss-chain traffic per sample (fp32, ideally fused)
CHAIN_FWD_BYTES = {4: 45.87e6, 1: 12.29e6}
CONFIGS = {"c3": dict(batch=12, num_scales=4, name="configs[2]/[3]: full 4-scale photometric+smoothness loss, batch 12 per GPU, ResNet-18"),
           "c2": dict(batch=4, num_scales=1, name="configs[1]: VO train step, batch 4, single-scale loss, ResNet-18")}


def train_config(batch, num_scales):
    return {"Train": dict(num_source=1, batch_size=batch, img_h=H, img_w=W, smoothness_ratio=0.001,
                          auto_mask=True, ssim_ratio=0.85, min_depth=0.1, max_depth=10.0, use_compile=False)}


# The timed steps run the fused Adam pass with lr 0: the kernel still reads and writes every weight and moment and the
# data-gradient packs are still refreshed, so a step's work is unchanged, but the weights stay the seeded ones.  Every step
# therefore computes from the same inputs, and two runs differ only by one step's rounding (float atomics), not by a
# trajectory of Adam updates that amplifies it (Adam moves a weight whose tiny gradient changes sign by a whole lr).
TIMED_LR = 0.0


def build_gpu(batch, num_scales, device, rank, comm=None, lr=1e-4):
    from deep_visual_slam_amd import dp, synth
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.learner_new import MonodepthTrainer
    from deep_visual_slam_amd.posenet_single import PoseNet
    torch.manual_seed(0)                      # same weights on every rank
    depth_net = DepthNet(18, pretrained=False).to(device).train()
    pose_net = PoseNet(18, pretrained=False, num_input_images=2).to(device).train()
    flat = dp.FlatParams(dp.trainable_parameters(depth_net, pose_net))
    trainer = MonodepthTrainer(depth_net, pose_net, train_config(batch, num_scales), device)
    trainer.num_scales = num_scales
    hook_streams = ({id(p): trainer.pose_stream for p in pose_net.parameters()} if trainer.pose_stream is not None else None)
    sync = dp.GradSync(flat, hook_streams=hook_streams, comm=comm)
    opt = dp.FusedAdam(flat, lr=lr)
    sample = synth.throughput_sample(batch, H, W, rank=rank, device=device)
    return trainer, flat, sync, opt, sample


def train_step(trainer, sync, opt, sample):
    """vo/train.py:173-199 train_mono_step: forward, backward, all-reduce, Adam (+ fused zero_grad); returns (outputs, losses)."""
    outputs, losses = trainer.process_batch(sample)
    losses["loss"].backward()
    sync.finish()
    opt.step(grad_scale=sync.grad_scale, zero_grad=True)
    return outputs, losses


def gpu_step(trainer, sync, opt, sample):
    """train_step's losses only (the warm-up, the --full legs, and the tools that import this file)."""
    return train_step(trainer, sync, opt, sample)[1]


DUMP_LIMIT_BYTES = 64 << 20
DUMP_WHOLE_MAX = 1 << 22           # an output with more elements is written as a fixed seeded sample of DUMP_SAMPLE of them
DUMP_SAMPLE = 1 << 21


def _seeded_sample(t, n, seed):
    """`n` elements of `t` (flattened) at sorted positions drawn without replacement from numpy's default_rng(seed): the same
    positions for the same numel, run after run."""
    import numpy as np
    idx = np.sort(np.random.default_rng(seed).choice(t.numel(), size=n, replace=False))
    return t.reshape(-1)[torch.from_numpy(idx).to(t.device)]


def dump_outputs(path, outputs, losses):
    """--dump-outputs DIR: what the timed path handed its caller in the last timed step, one DIR/<name>.npy per array --
    the losses (float64 scalars: loss, loss_0 ... loss_{S-1}) and the DepthNet / PoseNet entries of `outputs` (disp_<s>,
    axisangle_0_<f>, translation_0_<f>, cam_T_cam_0_<f>; float32; the lazy view-synthesis entries are not materialised).
    An output of more than DUMP_WHOLE_MAX elements (a --batch override) is written as <name>_sample: DUMP_SAMPLE of its
    elements at seeded positions.  The inputs are seeded and the weights fixed (TIMED_LR), so two runs differ only by the
    rounding of the step's float atomics."""
    import numpy as np
    arrays = {k.replace("/", "_"): v.detach().double() for k, v in losses.items()}
    for i, (k, v) in enumerate(sorted(dict.items(outputs), key=lambda kv: str(kv[0]))):    # no materialisation
        name = "_".join(str(p) for p in k) if isinstance(k, tuple) else str(k)
        v = v.detach().float()
        if v.numel() > DUMP_WHOLE_MAX:
            name, v = name + "_sample", _seeded_sample(v, DUMP_SAMPLE, 1 + i)
        arrays[name] = v
    arrays = {k: v.cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("bench.py: --dump-outputs would write %d bytes (limit %d)" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)


def build_stock(batch, num_scales, device, rank):
    """What the UNCHANGED reference caller constructs (vo/train.py:64-117): plain modules, one torch.optim.Adam over
    list(depth_net.parameters()) + list(pose_net.parameters()); no arena, no gradient sinks, no fused optimiser."""
    from deep_visual_slam_amd import synth
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.learner_new import MonodepthTrainer
    from deep_visual_slam_amd.posenet_single import PoseNet
    torch.manual_seed(0)
    depth_net = DepthNet(18, pretrained=False).to(device).train()
    pose_net = PoseNet(18, pretrained=False, num_input_images=2).to(device).train()
    opt = torch.optim.Adam(list(depth_net.parameters()) + list(pose_net.parameters()), lr=1e-4)
    trainer = MonodepthTrainer(depth_net, pose_net, train_config(batch, num_scales), device)
    trainer.num_scales = num_scales
    sample = synth.throughput_sample(batch, H, W, rank=rank, device=device)
    return trainer, opt, sample


def stock_step(trainer, opt, sample):
    """vo/train.py:173-199 train_mono_step, line for line (non-AMP branch)."""
    opt.zero_grad(set_to_none=True)
    outputs, losses = trainer.process_batch(sample)
    total_loss = losses["loss"]
    total_loss.backward()
    opt.step()
    total_loss = total_loss.detach()
    for key in losses:
        losses[key] = losses[key].detach().cpu()
    return total_loss, outputs, losses


def fresh_process_config(config, steps, warmup, extra=()):
    """`python bench.py --full --config <config>` with only the loss check of the `--full` legs, as a CHILD process (never an
    exec: this process has initialised the GPU); returns the
    child's JSON line, or None when it cannot run (under a profiler's preload, or on any failure -- the in-process figure stays)."""
    import subprocess
    import sys
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", ""):
        return None
    cmd = [sys.executable, os.path.abspath(__file__), "--config", config, "--steps", str(steps), "--warmup", str(warmup),
           "--full", "--no-cpu-baseline", "--no-other-configs", "--no-kernel-timing", "--no-stock-caller"] + list(extra)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        for line in reversed(r.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
    except Exception:
        pass
    return None


def time_stock(batch, num_scales, device, rank, steps, warmup):
    trainer, opt, sample = build_stock(batch, num_scales, device, rank)
    for _ in range(warmup):
        stock_step(trainer, opt, sample)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        stock_step(trainer, opt, sample)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"value": 3.0 * batch / dt, "unit": "frames/s", "ms_per_step": dt * 1e3, "steps": steps,
            "sequence": "vo/train.py:173-199 unchanged: optimizer.zero_grad(set_to_none=True); process_batch; backward; "
                        "torch.optim.Adam.step(); losses[k].detach().cpu() x5 (a host sync every step)"}


def loss_check(trainer, sample, config):
    """First-step loss of the seeded bench workload (rank 0) against the committed oracle value."""
    path = os.path.join(ROOT, "tests", "golden", "bench_loss.json")
    try:
        with open(path) as f:
            ref = json.load(f)[config]["losses"]
    except (OSError, KeyError, ValueError):
        return None
    B = sample[("target_image", 0)].shape[0]
    trainer._noise = torch.zeros(trainer.num_scales, B, 2, H, W, device=sample[("target_image", 0)].device)
    with torch.no_grad():
        was = [m.training for m in (trainer.depth_net, trainer.pose_net)]
        # training-mode forward without autograd; the BatchNorm running statistics it moves are restored below
        state = [{k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
                 for m in (trainer.depth_net, trainer.pose_net)]
        _, losses = trainer.process_batch(sample)
        got = {k: float(v) for k, v in losses.items()}
        for m, st in zip((trainer.depth_net, trainer.pose_net), state):
            m.load_state_dict(st, strict=False)
        assert was == [True, True]
    trainer._noise = None
    trainer._step = 0
    worst = max(abs(got[k] - ref[k]) / abs(ref[k]) for k in ref)
    from deep_visual_slam_amd import _lib
    tol = 2e-4 if _lib.precision() == "fp32" else 3e-2       # bf16 mode: operand rounding, its own tolerance (tests/test_bf16_gpu.py)
    return {"gpu": got["loss"], "oracle": ref["loss"], "worst_rel_err": worst, "tolerance": tol, "ok": worst < tol,
            "source": "tests/golden/bench_loss.json (oracle networks + loss chain, PyTorch-CPU fp32, tie-break noise 0)"}


def measured_peaks(device):
    """The two roofline denominators measured on THIS box in THIS run (boxes differ by ~10 %): HBM by a
    1 GiB device-to-device copy of 16 bytes per lane (2 GiB of traffic), fp32 MFMA by v_mfma_f32_32x32x2_f32 from registers on
    every SIMD (dvs_peak_probe_*); best of 5 launches each, HIP events on the launch stream."""
    import ctypes as C
    from deep_visual_slam_amd import _lib
    l = _lib.lib()
    st = _lib.stream()

    def best_ms(fn, n=5):
        fn()
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return min(ts)

    nbytes = 1 << 30
    src = torch.empty(nbytes // 4, device=device, dtype=torch.float32).normal_()
    dst = torch.empty_like(src)
    ms = best_ms(lambda: _lib.check(l.dvs_peak_probe_copy(src.data_ptr(), dst.data_ptr(), nbytes, st), "dvs_peak_probe_copy"))
    hbm = 2.0 * nbytes / (ms * 1e-3) / 1e9
    del src, dst
    flops = C.c_double()
    scratch = torch.zeros(16, device=device)
    ms = best_ms(lambda: _lib.check(l.dvs_peak_probe_mfma(scratch.data_ptr(), 8192, C.byref(flops), st), "dvs_peak_probe_mfma"))
    mfma = flops.value / (ms * 1e-3) / 1e12
    return {"hbm_copy_GBps": hbm, "mfma_f32_TFLOPs": mfma,
            "how": "1 GiB float4 device copy (2 GiB traffic) and register-fed v_mfma_f32_32x32x2_f32 on every SIMD, best of 5, "
                   "same process and box as the timed region; spec peaks stay the denominators of `frac`"}


def pmc_traffic(config, kernel):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC passes over this same command
    (tools/profile_bench.sh: FETCH_SIZE and WRITE_SIZE in separate passes, FETCH_SIZE doubled as
    MI355X_MICROARCH.md prescribes for gfx950).  Counters cannot be read from inside the timed run, so the
    number travels as profiles/traffic_<config>.json; null when that file is absent."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "traffic_%s.json" % config)
    try:
        with open(path) as f:
            k = json.load(f)["kernels"][kernel]
        return {"traffic": k["hbm_bytes_per_launch"], "traffic_unit": "bytes/launch (PMC)",
                "traffic_source": "profiles/traffic_%s.json" % config}
    except (OSError, KeyError, ValueError):
        return {"traffic": None}


def cpu_baseline(batch, num_scales, steps=2, warmup=1):
    """The reference's step on host cores: oracle networks + oracle loss chain + torch.optim.Adam."""
    from deep_visual_slam_amd import synth
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.posenet_single import PoseNet
    from oracle import loss_chain as OL, networks as ON
    # the GPU box gives one GPU's share of the host (16 cores); os.cpu_count() reports the whole machine
    cores = min(len(os.sched_getaffinity(0)), 16)
    torch.set_num_threads(cores)
    torch.manual_seed(0)
    sd_d = {k: v.clone().requires_grad_(v.is_floating_point() and ".fc." not in k and "running" not in k)
            for k, v in DepthNet(18, pretrained=False).state_dict().items()}
    sd_p = {k: v.clone().requires_grad_(v.is_floating_point() and ".fc." not in k and "running" not in k)
            for k, v in PoseNet(18, pretrained=False, num_input_images=2).state_dict().items()}
    params = [v for v in list(sd_d.values()) + list(sd_p.values()) if v.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-4)
    sample = synth.throughput_sample(batch, H, W)
    tgt, left, right = sample[("target_image", 0)], sample[("source_left", 0)], sample[("source_right", 0)]

    def step():
        opt.zero_grad(set_to_none=True)
        upd_d, upd_p = {}, {}
        disp = ON.depthnet(tgt, sd_d, train=True, update=upd_d)
        aa_l, t_l = ON.posenet(torch.cat([left, tgt], 1), sd_p, train=True, update=upd_p)
        aa_r, t_r = ON.posenet(torch.cat([tgt, right], 1), sd_p, train=True, update=upd_p)
        noise = [torch.randn(batch, 2, H, W) for _ in range(num_scales)]
        _, losses = OL.loss_chain(sample, [disp[("disp", s)] for s in range(num_scales)], (aa_l, t_l, aa_r, t_r),
                                  noise, num_scales=num_scales)
        losses["loss"].backward()
        opt.step()
        return float(losses["loss"])

    for _ in range(warmup):
        step()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    dt = (time.perf_counter() - t0) / steps
    return {"value": 3.0 * batch / dt, "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": "%d timed + %d warm-up train steps of the same workload at batch %d (%d-scale loss), "
                      "oracle/networks.py + oracle/loss_chain.py on PyTorch-CPU fp32, %.2f s/step"
                      % (steps, warmup, batch, num_scales, dt)}


def inference_side(device, with_cpu):
    """BASELINE.json configs[0] on the GPU: depth-only forward of one 640x480 frame (eval() + no_grad, the inference
    path of deep_visual_slam_amd/inference.py), and the whole per-frame work of vo/predict.py:63-86 (PoseNet on the
    frame pair + pose matrix + DepthNet + depth), eager and as a HIP-graph replay; the CPU oracle's eval-mode DepthNet
    on the same frame beside it."""
    from deep_visual_slam_amd import inference
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.posenet_single import PoseNet
    from deep_visual_slam_amd.layers import transformation_from_parameters, disp_to_depth
    torch.manual_seed(0)
    dn, pn = DepthNet(18, pretrained=False).to(device), PoseNet(18, pretrained=False, num_input_images=2).to(device)
    inference.prepare(dn, pn, scales=(0,))
    g = torch.Generator().manual_seed(1234)
    tgt, pair = torch.rand(1, 3, H, W, generator=g).to(device), torch.rand(1, 6, H, W, generator=g).to(device)

    def depth_only(depth, pose):
        return depth(tgt)[("disp", 0)]

    def frame(depth, pose):
        aa, t = pose(pair)
        T = transformation_from_parameters(aa[:, 0], t[:, 0], invert=False)
        _, d = disp_to_depth(depth(tgt)[("disp", 0)], 0.1, 10.0)
        return T, d

    def timeit(fn, depth, pose, n=100):
        with torch.no_grad():
            for _ in range(10):
                fn(depth, pose)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn(depth, pose)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    res = {"workload": "configs[0]: depth-only forward, one 640x480 frame, ResNet-18 encoder + DepthDecoder (eval, batch 1)",
           "unit": "frames/s"}
    t = timeit(depth_only, dn, pn)
    res["value"] = 1.0 / t
    res["ms_per_frame"] = t * 1e3
    t = timeit(frame, dn, pn)
    gd, gp = inference.Graphed(dn, tgt), inference.Graphed(pn, pair)
    tg = timeit(frame, gd, gp)
    fp_e = inference.FramePredictor(dn, pn, tgt, pair, graph=False)
    fp_g = inference.FramePredictor(dn, pn, tgt, pair, graph=True)
    t2 = timeit(lambda d, p: fp_e(tgt, pair), None, None)
    t2g = timeit(lambda d, p: fp_g(tgt, pair), None, None)
    res["predict_frame"] = {"workload": "PoseNet(pair) + pose matrix + DepthNet(frame) + depth, as vo/predict.py:63-86",
                            "eager_frames_per_s": 1.0 / t, "graph_frames_per_s": 1.0 / tg,
                            "eager_ms": t * 1e3, "graph_ms": tg * 1e3,
                            "two_stream_eager_ms": t2 * 1e3, "two_stream_graph_ms": t2g * 1e3,
                            "two_stream_graph_frames_per_s": 1.0 / t2g,
                            "note": "two_stream_*: inference.FramePredictor (PoseNet and DepthNet side by side)"}
    if with_cpu:
        from oracle import networks as ON
        cores = min(len(os.sched_getaffinity(0)), 16)
        torch.set_num_threads(cores)
        sd = {k: v.detach().cpu() for k, v in dn.state_dict().items()}
        x = tgt.cpu()
        with torch.no_grad():
            ON.depthnet(x, sd, train=False)
            t0 = time.perf_counter()
            for _ in range(3):
                ON.depthnet(x, sd, train=False)
            tc = (time.perf_counter() - t0) / 3
        res["cpu_baseline"] = {"value": 1.0 / tc, "unit": "frames/s", "cores": cores, "kind": "port",
                               "sample": "3 timed + 1 warm-up eval-mode DepthNet forwards of the same frame, oracle/networks.py "
                                         "on PyTorch-CPU fp32, %.3f s/frame" % tc}
    return res


def dav2_side(device, with_cpu, batches=(1, 8)):
    """BASELINE.json configs[4]: Depth-Anything-V2 ViT-S (DINOv2 encoder + DPT head) forward at 518x518 on the MI355X path
    (deep_visual_slam_amd/depth_anything_v2.py: token GEMMs on the implicit-GEMM engine, flash attention on the fp32
    matrix cores), seeded random weights; per-kernel-class HIP-event times give the MFMA rooflines of the attention kernel
    and of the GEMM / convolution launches.  CPU beside it: the oracle restatement of the same forward."""
    from deep_visual_slam_amd import dp
    from deep_visual_slam_amd.depth_anything_v2 import DepthAnythingV2
    torch.manual_seed(0)
    net = DepthAnythingV2(encoder="vits", features=64, out_channels=[48, 96, 192, 384]).to(device).eval()
    res = {"workload": "configs[4]: Depth-Anything-V2 ViT-S forward, 518x518 (N = 1370 tokens, 12 blocks, 6 heads of 64), DPT head",
           "unit": "frames/s", "dtype": "f32", "batches": {}}
    for B in batches:
        x = torch.randn(B, 3, 518, 518, device=device)
        with torch.no_grad():
            for _ in range(3):
                net(x)
            torch.cuda.synchronize()
            n = 20
            t0 = time.perf_counter()
            for _ in range(n):
                net(x)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            dp.profile_enable(True)
            for _ in range(3):
                net(x)
            torch.cuda.synchronize()
            prof = dp.profile_read()
            dp.profile_enable(False)
        entry = {"value": B / dt, "ms_per_forward": dt * 1e3}
        for k, name in (("attention_fwd_kernel", "attention"), ("conv_fwd_kernel", "gemm_and_conv")):
            if k in prof:
                ms, cnt, fl = prof[k]
                ach = fl / (ms * 1e-3) / 1e12
                entry[name] = {"ms_per_forward": ms / 3, "launches_per_forward": cnt / 3, "algorithmic_gflop_per_forward": fl / 3e9,
                               "roofline": {"bound": "mfma", "achieved": ach, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                                            "frac": ach / MFMA_F32_PEAK_TFLOPS}}
        if B == 1:
            # batch 1 issues ~130 launches of 5-40 us: replayed from a HIP graph the frame is no longer bound by issue
            from deep_visual_slam_amd import inference
            gnet = inference.Graphed(net, x)
            with torch.no_grad():
                for _ in range(3):
                    gnet(x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    gnet(x)
                torch.cuda.synchronize()
            entry["graph_ms_per_forward"] = (time.perf_counter() - t0) / n * 1e3
            entry["graph_value"] = 1e3 / entry["graph_ms_per_forward"]
            del gnet
        res["batches"]["batch_%d" % B] = entry
    res["value"] = res["batches"]["batch_%d" % batches[-1]]["value"]
    # the same forward with the token GEMMs / DPT convolutions in the opt-in bf16 mode (include/dvslam.h dvs_set_precision; the
    # attention kernel stays fp32): a separately labelled figure with the deviation of its output, never `value`
    from deep_visual_slam_amd import _lib as _dvs_lib
    if _dvs_lib.precision() == "fp32":
        Bb = batches[-1]
        xb = torch.randn(Bb, 3, 518, 518, device=device)
        with torch.no_grad():
            y32 = net(xb).float().clone()
            try:
                _dvs_lib.set_precision("bf16")
                for _ in range(3):
                    y16 = net(xb)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(20):
                    net(xb)
                torch.cuda.synchronize()
                dtb = (time.perf_counter() - t0) / 20
            finally:
                _dvs_lib.set_precision("fp32")
        res["bf16_mode"] = {"batch": Bb, "value": Bb / dtb, "ms_per_forward": dtb * 1e3,
                            "dtype": "bf16 operands x fp32 accumulate in the token GEMMs, attention products and convolutions; fp32 softmax, LayerNorm, GELU (opt-in mode)",
                            "rel_max_diff_of_depth_vs_fp32": float((y16.float() - y32).abs().max() / y32.abs().max())}
    # the trainable path (autograd on): forward + backward of a scalar loss, batch 4
    Bt = 4
    net.train()
    xt = torch.randn(Bt, 3, 518, 518, device=device)

    def train_pass():
        net.zero_grad(set_to_none=True)
        net(xt).mean().backward()

    for _ in range(2):
        train_pass()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        train_pass()
    torch.cuda.synchronize()
    dtt = (time.perf_counter() - t0) / 5
    dp.profile_enable(True)
    for _ in range(2):
        train_pass()
    torch.cuda.synchronize()
    prof = dp.profile_read()
    dp.profile_enable(False)
    tr = {"batch": Bt, "ms_per_forward_backward": dtt * 1e3, "value": Bt / dtt}
    for k in ("attention_fwd_kernel", "attention_bwd_kernel", "conv_fwd_kernel", "conv_dgrad_kernel", "conv_wgrad_kernel"):
        if k in prof:
            ms, cnt, fl = prof[k]
            tr[k] = {"ms": ms / 2, "launches": cnt / 2, "tflops": fl / (ms * 1e-3) / 1e12}
    res["train"] = tr
    net.eval()
    if with_cpu:
        from oracle import depth_anything as OD
        cores = min(len(os.sched_getaffinity(0)), 16)
        torch.set_num_threads(cores)
        sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
        xc = torch.randn(1, 3, 518, 518)
        with torch.no_grad():
            OD.depth_anything_v2(xc, sd)
            t0 = time.perf_counter()
            for _ in range(3):
                OD.depth_anything_v2(xc, sd)
            tc = (time.perf_counter() - t0) / 3
        res["cpu_baseline"] = {"value": 1.0 / tc, "unit": "frames/s", "cores": cores, "kind": "port",
                               "sample": "3 timed + 1 warm-up forwards of one 518x518 frame, oracle/depth_anything.py on PyTorch-CPU fp32, "
                                         "%.3f s/frame" % tc}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch override")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=None, help="batch of the CPU baseline (default: the bench batch)")
    ap.add_argument("--no-stock-caller", action="store_true", help="skip the unchanged-caller (vo/train.py sequence) side measurement")
    ap.add_argument("--no-loss-check", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the configs[1] side measurement")
    ap.add_argument("--no-kernel-timing", action="store_true",
                    help="skip the per-launch HIP-event steps after the timed region (no roofline object in the output)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"],
                    help="bf16: the opt-in mode of the implicit-GEMM convolutions (include/dvslam.h dvs_set_precision; bf16 operands, "
                         "fp32 accumulate) -- a separately labelled measurement, never the headline")
    ap.add_argument("--serialize", action="store_true",
                    help="run the timed region on one stream too (what the rocprofv3 per-kernel passes use)")
    ap.add_argument("--full", action="store_true",
                    help="also the loss check, the per-kernel roofline, the measured peaks, the CPU baseline, the stock caller and the "
                         "other configurations (the --no-* switches drop single legs); a plain run only times the K steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (losses, network outputs, a seeded sample of the updated "
                         "weights) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    cfg = CONFIGS[args.config]
    batch = args.batch or cfg["batch"]
    num_scales = cfg["num_scales"]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d"
                         % (args.gpus, world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    # rehearsal of the N > 1 code path on a one-GPU box: DVS_BENCH_REHEARSE=1 puts every rank on cuda:0 and carries the
    # all-reduce over gloo (the numbers mean nothing then; the driver's multi-GPU runs use RCCL, one GPU per rank)
    rehearse = os.environ.get("DVS_BENCH_REHEARSE") == "1"
    if rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)

    import __graft_entry__ as entry
    if rank == 0:
        entry.build()
    if world > 1:
        dist.barrier()
    from deep_visual_slam_amd import dp
    if args.precision != "fp32":
        from deep_visual_slam_amd import _lib as _dvs_lib
        _dvs_lib.set_precision(args.precision)

    comm = None
    # N > 1: the gradient buckets go through this repo's own RCCL C-ABI (include/dvslam_rccl.h, dp.RcclComm: a communicator on a
    # stream -- hardware queue -- of its own); DVS_ALLREDUCE=torch is the explicit switch back to torch.distributed's process group
    comm_note = None
    if world > 1 and os.environ.get("DVS_ALLREDUCE", "rccl") == "rccl" and not rehearse:
        # self-test before anything is timed: a 1 M-float all-reduce through the communicator must give world_size everywhere;
        # if the communicator cannot be built or answers wrongly on ANY rank, every rank falls back to torch.distributed (the
        # line says so in config.allreduce) rather than losing the scaling run
        ok = 1
        try:
            comm = dp.RcclComm(device)
            probe = torch.ones(1 << 20, device=device)
            comm.all_reduce_(probe)
            comm.wait()
            torch.cuda.synchronize()
            ok = int(bool((probe == float(world)).all()))
        except Exception as e:                    # noqa: BLE001 -- reported, not swallowed
            ok, comm_note = 0, "%s: %s" % (type(e).__name__, e)
        flag = torch.tensor([ok], device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag) == 0:
            comm = None
            comm_note = "direct RCCL communicator failed its self-test on some rank (%s): torch.distributed carries the buckets" % (comm_note or "this rank was fine")
    trainer, flat, sync, opt, sample = build_gpu(batch, num_scales, device, rank, comm=comm, lr=TIMED_LR)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def set_concurrency(on):
        """Multi-stream execution (PoseNet stream, weight-gradient side streams) on / off."""
        from deep_visual_slam_amd import gradsink
        torch.cuda.synchronize()
        gradsink.enable_side_streams(on)
        trainer.pose_stream = pose_stream if on else None

    pose_stream = trainer.pose_stream
    if args.serialize:
        set_concurrency(False)
    check = None
    if args.full and rank == 0 and not args.no_loss_check and args.batch is None:
        check = loss_check(trainer, sample, args.config)
        if check is not None and not check["ok"]:
            raise SystemExit("bench.py: first-step loss %.8f differs from the oracle's %.8f (rel %.2e): refusing to time a "
                             "wrong result" % (check["gpu"], check["oracle"], check["worst_rel_err"]))
    for _ in range(args.warmup):
        gpu_step(trainer, sync, opt, sample)
    barrier()
    # timed region: K steps, nothing else (no per-launch events; one event record per step on the main stream for the
    # median, which costs no synchronisation)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        outputs, losses = train_step(trainer, sync, opt, sample)
        marks[i + 1].record()
        if i + 1 < args.steps:
            outputs = None                    # as in gpu_step: only the last step's outputs outlive the step (--dump-outputs)
    barrier()
    dt = time.perf_counter() - t0
    intervals = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    median_ms = intervals[len(intervals) // 2] if len(intervals) % 2 else 0.5 * (intervals[len(intervals) // 2 - 1] + intervals[len(intervals) // 2])
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, outputs, losses)
    del outputs
    # per-kernel durations for the roofline: HIP events around every launch of the library, over further steps
    # of the same loop run on ONE stream -- with DepthNet, PoseNet and the weight gradients overlapping on four
    # streams an event pair measures how long a kernel shared the chip, not how long it needs
    prof, prof_steps = {}, 0
    if args.full and not args.no_kernel_timing:
        set_concurrency(False)
        gpu_step(trainer, sync, opt, sample)
        barrier()
        dp.profile_enable(True)
        prof_steps = max(1, min(args.steps, 5))
        for _ in range(prof_steps):
            gpu_step(trainer, sync, opt, sample)
        barrier()
        prof = dp.profile_read()
        dp.profile_enable(False)
        set_concurrency(not args.serialize)
    loss_val = float(losses["loss"].detach())

    t = torch.tensor([dt], device=device, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t)
    ms_per_step = dt / args.steps * 1e3
    value = 3.0 * batch * world * args.steps / dt

    if rank == 0:
        # roofline of the dominant hand-written kernel inside the timed region
        per_kernel = {k: (ms / n, n) for k, (ms, n, _) in prof.items()}
        per_step = {k: ms / prof_steps for k, (ms, n, _) in prof.items()}
        dom = max(prof, key=lambda k: prof[k][0]) if prof else None      # most time inside the timed region
        roof = None
        if dom in ("chain_fwd_kernel", "chain_bwd_kernel"):
            nbytes = CHAIN_FWD_BYTES[num_scales] * batch      # fwd and bwd move the same compulsory bytes
            avg_s = per_kernel[dom][0] * 1e-3
            ach = nbytes / avg_s / 1e9
            roof = {"kernel": dom, "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": ach / HBM_PEAK_GBPS, "traffic": None, "avg_launch_ms": per_kernel[dom][0],
                    "algorithmic_bytes_per_launch": nbytes}
        elif dom is not None and dom.startswith("conv_"):
            # the conv kernels run once per layer with different shapes: achieved = sum of the launches'
            # algorithmic flops (2*M*N*K, counted inside the library) / sum of their HIP-event durations
            ms, n, flops = prof[dom]
            ach = flops / (ms * 1e-3) / 1e12
            roof = {"kernel": dom, "bound": "mfma", "achieved": ach, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": ach / MFMA_F32_PEAK_TFLOPS, "traffic": None, "avg_launch_ms": ms / n,
                    "launches_per_step": n / prof_steps, "algorithmic_flops_per_step": flops / prof_steps}
        all_conv = {k: v for k, v in prof.items() if k.startswith("conv_")}
        conv_summary = None
        if all_conv:
            conv_summary = {k: {"ms_per_step": v[0] / prof_steps, "tflops": v[2] / (v[0] * 1e-3) / 1e12}
                            for k, v in all_conv.items()}
        if roof is not None:
            roof["measured"] = ("HIP events on the launch stream, %d single-stream steps after the timed region "
                                "(the timed steps overlap four streams)" % prof_steps)
            roof["flops_counted"] = ("algorithmic = direct-convolution flops 2*M*N*K; the stride-1 3x3 BasicBlock convolutions (26 of "
                                     "the 53 timed scopes of each conv slot at configs[2]) and, in the weight-gradient slot, the eight "
                                     "decoder Conv3x3 layers with 32-channel blocks run Winograd F(2x2,3x3), which executes 2.25x "
                                     "fewer MFMA flops than counted (DVS_WINOGRAD=0 / DVS_WINOGRAD_WGRAD=0 / "
                                     "DVS_WINOGRAD_DECODER_WGRAD=0 time the direct kernels)")
            roof.update(pmc_traffic(args.config, roof["kernel"]))
        peaks = measured_peaks(device) if args.full else None
        if roof is not None:
            roof["peak_measured"] = peaks["mfma_f32_TFLOPs"] if roof["bound"] == "mfma" else peaks["hbm_copy_GBps"]
            roof["frac_of_measured"] = roof["achieved"] / roof["peak_measured"]
        # the loss chain against the HBM roofline (45.87 MB per sample and direction
        # for 4 scales): algorithmic bytes / kernel time of the same single-stream steps
        chain = None
        if "chain_fwd_kernel" in per_step and "chain_bwd_kernel" in per_step:
            nbytes = CHAIN_FWD_BYTES[num_scales] * batch
            chain = {"bound": "hbm", "peak": HBM_PEAK_GBPS, "peak_measured": peaks["hbm_copy_GBps"], "unit": "GB/s",
                     "algorithmic_bytes_per_direction": nbytes}
            for name in ("chain_fwd_kernel", "chain_bwd_kernel"):
                ach = nbytes / (per_step[name] * 1e-3) / 1e9
                chain[name] = {"ms_per_step": per_step[name], "achieved": ach, "frac": ach / HBM_PEAK_GBPS,
                               "frac_of_measured": ach / peaks["hbm_copy_GBps"], **pmc_traffic(args.config, name)}
        out = {"metric": "VO training-step frames/sec (3-frame 640x480 snippets)", "value": value,
               "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": ms_per_step, "median_ms_per_step": median_ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f32" if args.precision == "fp32" else "bf16 operands x fp32 accumulate in the implicit-GEMM convolutions, f32 elsewhere (opt-in mode, NOT the headline precision)",
               "data": "synthetic",
               "config": {"workload": cfg["name"], "per_gpu_batch": batch, "global_batch": batch * world,
                          "num_scales": num_scales, "image": "%dx%d" % (W, H),
                          "parallelism": "dp%d" % world,
                          "outputs": "lazy (the per-scale view-synthesis tensors of `outputs` are materialised on first access, "
                                     "SURVEY.md section 8d; config Train.materialize_outputs times the eager variant)",
                          "streams": "single" if args.serialize else "depth | pose | 2x weight-gradient",
                          "optimizer": "fused Adam pass at lr %g: every step computes from the seeded weights" % TIMED_LR,
                          "allreduce": (None if world == 1 else ("rccl-direct (include/dvslam_rccl.h)" if comm is not None else "torch.distributed " + dist.get_backend()
                                                                      + (" -- " + comm_note if comm_note else ""))),
                          "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "default (4)")},
               "loss": loss_val}
        if args.full:
            out.update({"loss_check": check,
                        "kernels_ms_per_step": {k: round(v, 4) for k, v in per_step.items()},
                        "conv_kernels": conv_summary,
                        "roofline": roof, "roofline_chain": chain, "measured_peaks": peaks})
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.cpu_batch or batch, num_scales)
        if args.full and world == 1 and args.config == "c3" and not args.no_other_configs:
            # BASELINE.json configs[1] (batch 4, single-scale loss) beside the headline workload: same code path,
            # same timing discipline, reported for reference -- `value` above is the batch-12 4-scale step
            del trainer, flat, sync, opt, sample, losses, pose_stream
            import gc
            from deep_visual_slam_amd import gradsink
            torch.cuda.synchronize()
            gradsink.reset_streams()             # the first trainer's streams must not linger (hardware queues are few)
            gc.collect()
            torch.cuda.empty_cache()
            if not args.no_stock_caller:
                out["stock_caller"] = time_stock(batch, num_scales, device, rank, min(args.steps, 20), min(args.warmup, 5))
                torch.cuda.synchronize()
                gradsink.reset_streams()
                gc.collect()
                torch.cuda.empty_cache()
            c2 = CONFIGS["c2"]
            tr2, _, sync2, opt2, sample2 = build_gpu(c2["batch"], c2["num_scales"], device, rank, lr=TIMED_LR)
            check2 = loss_check(tr2, sample2, "c2") if not args.no_loss_check else None
            for _ in range(args.warmup):
                gpu_step(tr2, sync2, opt2, sample2)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                gpu_step(tr2, sync2, opt2, sample2)
            torch.cuda.synchronize()
            dt2 = time.perf_counter() - t1
            out["other_configs"] = {"configs[1]": {"workload": c2["name"], "value": 3.0 * c2["batch"] * args.steps / dt2,
                                                   "unit": "frames/s", "ms_per_step": dt2 / args.steps * 1e3,
                                                   "per_gpu_batch": c2["batch"], "num_scales": c2["num_scales"],
                                                   "loss_check": check2,
                                                   "process": "this process, after the configs[2] trainer and the stock caller"}}
            del tr2, sync2, opt2, sample2
            torch.cuda.synchronize()
            gradsink.reset_streams()
            gc.collect()
            torch.cuda.empty_cache()
            if not args.no_stock_caller:
                out["other_configs"]["configs[1]"]["stock_caller"] = time_stock(c2["batch"], c2["num_scales"], device, rank,
                                                                                 min(args.steps, 20), min(args.warmup, 5))
            torch.cuda.synchronize()
            gradsink.reset_streams()
            gc.collect()
            torch.cuda.empty_cache()
            # configs[1] is host-bound, and a process that has already built (and dropped) two trainers issues it ~2 ms per step
            # slower than a fresh one (HIP hands later streams hardware queues that earlier, destroyed streams still map to):
            # what a user who trains configs[1] gets is the fresh-process figure, so it is measured that way too -- the same
            # file, `--config c2`, as a child process while this one idles -- and both figures are reported.
            fresh = fresh_process_config("c2", args.steps, args.warmup)
            if fresh is not None:
                c1 = out["other_configs"]["configs[1]"]
                c1["in_process"] = {"value": c1["value"], "ms_per_step": c1["ms_per_step"], "process": c1["process"]}
                c1.update(value=fresh["value"], ms_per_step=fresh["ms_per_step"], median_ms_per_step=fresh.get("median_ms_per_step"),
                          loss_check=fresh.get("loss_check"), process="fresh child process: python bench.py --config c2")
            # the opt-in bf16 mode of the convolutions on the headline workload (same file, `--precision bf16`, child process):
            # a separately labelled leg, never `value`
            if args.precision == "fp32":
                bf = fresh_process_config("c3", args.steps, args.warmup, ("--precision", "bf16"))
                if bf is not None:
                    out["other_configs"]["bf16_mode"] = {
                        "workload": bf["config"]["workload"], "value": bf["value"], "unit": bf["unit"], "ms_per_step": bf["ms_per_step"],
                        "median_ms_per_step": bf.get("median_ms_per_step"), "dtype": bf["dtype"], "loss_check": bf.get("loss_check"),
                        "speedup_vs_value": out["ms_per_step"] / bf["ms_per_step"],
                        "process": "fresh child process: python bench.py --precision bf16",
                        "note": "include/dvslam.h dvs_set_precision(1): forward / data / weight gradient of the implicit-GEMM "
                                "convolutions on v_mfma_f32_32x32x16_bf16; Winograd off; stems, thin layers, heads, BatchNorm, loss "
                                "chain, Adam in fp32; tolerances in tests/test_bf16_gpu.py"}
            out["other_configs"]["configs[0]"] = inference_side(device, not args.no_cpu_baseline)
            out["other_configs"]["configs[4]"] = dav2_side(device, not args.no_cpu_baseline)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
