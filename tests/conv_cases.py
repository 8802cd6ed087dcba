"""One tiny convolution case per launch sequence of tests/golden/conv_routes.json.

conv_routes.json pins WHICH kernels every product layer runs, in every mode (tests/test_conv_routes_cpu.py).  With the
deterministic mode off it holds 386 distinct launch sequences; this module derives, for each of them, one small case that
runs the same sequence, so that tests/test_conv_sequences_gpu.py can check the NUMBERS each sequence produces against fp64.

  shrink(layer)            the small shapes of a layer of test_conv_routes_cpu.LAYERS (channels and options stay)
  forced_costs(a, b)       conv.wino_pays / conv.wino_dec_wgrad_pays as constants: at a tiny size the cost models would
                           always say "direct", and one of the two alone misses the sequences that pair a direct forward
                           with a Winograd weight gradient
  thin_* / dma_launch      the C entry points' own choice by shape (thin kernels, LDS-DMA split-K), as plain arithmetic
  refused(...)             the one launch the C entry point refuses (and conv.supported() excludes)
  reference(...)           the fp64 torch composition of a case
  record() / load()        tests/golden/conv_small_cases.json: the first case in table order that reaches each sequence
                           (`python tests/conv_cases.py --record`)

A plain module (imported like guard), not a conftest.
"""
import contextlib
import itertools
import json
import os
import sys

import pytest
import torch

import test_conv_routes_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = os.path.join(ROOT, "tests", "golden", "conv_small_cases.json")
BATCH = 2
COSTS = tuple(itertools.product((False, True), repeat=2))           # (wino_pays, wino_dec_wgrad_pays)
BK = 32                                                             # csrc/conv_common.h: channels of one K stage
SPLITK_TILES = 320                                                  # csrc/conv_fwd.hip launch_dma: fewer tiles split K

# ---------------------------------------------------------------------------------------------- the shrink rule
# Full-resolution (H, W) of the small case.  The thin decoder kernels (csrc/conv_thin.hip) choose by width, so the layers they
# take keep a width of the same class as the product's: 96 -> 32 on 64-column segments, 64 -> 32 on a ragged last segment
# (160 = 2 x 64 + 32 columns there, 96 = 64 + 32 here; 80 would lose the row-ring weight gradient, which needs W % 32 == 0),
# 32 -> 16 at W % 64 == 0 and 16 -> 16 at W % 128 == 0; all need H >= 8 and even sizes under an upsample.
THIN_HW = {"dec7": (8, 64), "dec6": (8, 96), "thin32": (8, 64), "thin16": (8, 128)}
PLAIN_HW = (10, 32)
STEM_HW = (22, 38)


def small_hw(layer):
    if layer.startswith("ragged"):
        return None
    if layer == "stem":
        return STEM_HW
    return THIN_HW.get(layer.split("_")[0], PLAIN_HW)


def shrink(layer, hw=None):
    """The layer's configuration with small spatial sizes: x at hw (half of it under an upsample), the skip at hw."""
    cfg = dict(R.LAYERS[layer])
    hw = hw or small_hw(layer)
    if hw is None:
        return cfg
    h, w = hw
    if cfg["x2"] is None:
        cfg["x"] = (cfg["x"][0], h, w)
    else:
        cfg["x"] = (cfg["x"][0], h // 2, w // 2)
        if isinstance(cfg["x2"], tuple):
            cfg["x2"] = (cfg["x2"][0], h, w)
    return cfg


@contextlib.contextmanager
def forced_costs(wino_pays, dec_wgrad_pays):
    """The two cost models of conv.py answer with these constants (each independently of the other)."""
    from deep_visual_slam_amd import conv
    saved = conv.wino_pays, conv.wino_dec_wgrad_pays
    conv.wino_pays = lambda *a: bool(wino_pays)
    conv.wino_dec_wgrad_pays = lambda *a: bool(dec_wgrad_pays)
    try:
        yield
    finally:
        conv.wino_pays, conv.wino_dec_wgrad_pays = saved


def case_id(layer, batch, precision, switch, grads, sink):
    return "%s|b%d|%s|det0|%s|%s|sink%d" % (layer, batch, precision, switch, grads, int(sink))


def entry_cfg(e):
    """The small configuration an entry of the JSON names."""
    cfg = dict(R.LAYERS[e["layer"]])
    cfg["x"] = tuple(e["x"])
    cfg["x2"] = tuple(e["x2"]) if isinstance(e["x2"], list) else e["x2"]
    return cfg


def run_entry(mp, e):
    """The launch log of an entry at its small shape (recorders instead of launches, no GPU)."""
    with forced_costs(e["wino_pays"], e["dec_wgrad_pays"]):
        return R.run_case(mp, entry_cfg(e), e["batch"], e["precision"], False, e["switch"], e["grads"], bool(e["sink"]))[0]


def entry_id(e):
    return "%s-%s-%s-%s-s%d-c%d%d%s" % (e["layer"], e["precision"], e["switch"], e["grads"], e["sink"], e["wino_pays"],
                                        e["dec_wgrad_pays"], "-unsplit" if e["double"] else "")


def load():
    with open(SMALL) as f:
        return json.load(f)["cases"]


def golden_det0():
    """case id -> log of every deterministic-off case of conv_routes.json."""
    return {cid: log for cid, (log, _) in R.expand_golden().items() if "|det0|" in cid}


# ---------------------------------------------------------------------------------------------- the C entry points' dispatch
def _logical(cfg, batch):
    """(B, Cin, H, W, c1, up) of the gathered full-resolution input."""
    c1, h, w = cfg["x"]
    up = cfg["x2"] is not None
    c2 = cfg["x2"][0] if isinstance(cfg["x2"], tuple) else 0
    return batch, c1 + c2, (2 * h if up else h), (2 * w if up else w), c1, up


def _thin_common(cfg):
    return cfg["w"][2] == 3 and cfg["stride"] == 1 and cfg["reflect_pad"] == 1 and not cfg["planar"]


def thin_fwd(cfg, batch):
    """csrc/conv_thin.hip thin_fwd: the template instance it launches, or None (no statistics, no residual)."""
    B, ci, H, W, c1, up = _logical(cfg, batch)
    co = cfg["w"][0]
    if not _thin_common(cfg) or cfg["stats"] or co != 16 or H < 8 or (up and (c1 != ci or (H | W) & 1)):
        return None
    if ci == 16 and W % 128 == 0:
        return "thin_fwd<16,128>"
    if ci == 32 and W % 64 == 0:
        return "thin_fwd<32,64>"
    return None


def thin_wgrad(cfg, batch):
    """csrc/conv_thin.hip thin_wgrad_shape."""
    B, ci, H, W, c1, up = _logical(cfg, batch)
    co = cfg["w"][0]
    if not _thin_common(cfg) or H < 8 or (up and (H | W) & 1) or c1 & 3:
        return None
    for o, i, m in ((32, 96, 32), (32, 64, 32), (16, 32, 64), (16, 16, 128)):
        if (co, ci) == (o, i) and W % m == 0:
            return "thin_wgrad<%d,%d,%d>" % (o, i, m)
    return None


def thin_dgrad(cfg, batch, residual=False):
    """csrc/conv_thin.hip thin_dgrad as dvs_conv2d_dgrad reaches it (reflection pad, no residual)."""
    B, ci, H, W, c1, up = _logical(cfg, batch)
    co, split = cfg["w"][0], (c1 if up else 0)
    if not _thin_common(cfg) or residual or H < 8 or (split and (H | W) & 1):
        return None
    if co == 16 and ci == 16 and split == 16 and W % 128 == 0:
        return "thin_dgrad<16,1,128>"
    if co == 16 and ci == 32 and split == 0 and W % 64 == 0:
        return "thin_dgrad<16,2,64>"
    if co == 32 and ci % 48 == 0 and ci <= 192 and split % 16 == 0 and W % 64 == 0:
        return "thin_dgrad<32,3,64,w1>"
    if co == 32 and ci % 32 == 0 and ci <= 128 and split % 16 == 0 and (W % 64 == 0 or (W % 16 == 0 and W > 64)):
        return "thin_dgrad<32,2,64>" + ("" if W % 64 == 0 else " ragged")
    return None


def _tile(M, N, mode_dgrad, stats, k1x1):
    """csrc/conv_fwd.hip launch_mode: (BM, BN) of the implicit-GEMM tile for M rows and N columns."""
    if N > 64:
        t64 = -(-M // 64) * -(-N // 128)
        t128 = -(-M // 128) * -(-N // 128)
        rounds = t128 / 512.0
        full = -(-t128 // 512)
        tail_waste = rounds <= 3.2 and (full - rounds) / full > 0.2
        if not mode_dgrad and ((stats and t64 < 160) or (k1x1 and t64 < 224)):
            return 64, 64
        return (64, 128) if (t128 < 448 or tail_waste) else (128, 128)
    return (128, 64) if N > 32 else (128, 32)


def dma_launch(cfg, batch, precision, what, act_fused=False):
    """How csrc/conv_fwd.hip launches the direct forward (what="fwd"), the direct data gradient ("dgrad": act_fused says whether
    the activation derivative rides in its gather) or the padded-domain one ("padded") of this layer: None when the launch is not
    the LDS-DMA kernel (bf16 mode, planar input, a thin kernel, a gather with arithmetic), else {"tiles", "ksplit"}: the tile count
    and whether launch_dma splits K (deterministic mode off)."""
    B, ci, H, W, c1, up = _logical(cfg, batch)
    co, _, kh, kw = cfg["w"]
    stride, pad = cfg["stride"], (cfg["reflect_pad"] or cfg["padding"])
    if precision == "bf16" or cfg["planar"] or kh > 3:
        return None
    if what == "fwd":
        if thin_fwd(cfg, batch) or ci % BK:
            return None
        Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
        M, N, K, stats = B * Ho * Wo, co, ci, bool(cfg["stats"] & 3)
        dgrad = False
    else:
        # GEMM rows = input pixels, N = input channels, reduction over the output channels
        if co % BK:
            return None
        if what == "padded":
            H, W = H + 2, W + 2                                  # the reflection-padded input, zero padding, no split
        elif act_fused or cfg["reflect_pad"] or up or thin_dgrad(cfg, batch, cfg["passthrough"]):
            return None                                          # dma_eligible<IN_DGRAD>: dact == 0, zero padding, no split
        if ci == 96:
            return None                                          # launch_mode's 128 x 96 tile is register-staged
        M, N, K, stats, dgrad = B * H * W, ci, co, False, True
        if stride == 2:
            return None                                          # parity classes: never split, out of this rule's scope
    bm, bn = _tile(M, N, dgrad, stats, kh == 1)
    tiles = -(-M // bm) * -(-N // bn)
    return {"tiles": tiles, "ksplit": (not stats) and tiles < SPLITK_TILES and K // BK >= 2 and N % 4 == 0}


def direct_launches(cfg, log):
    """[(what, act_fused)] of the direct forward / data-gradient launches a log holds."""
    out = []
    for call in log.split(" "):
        name, _, args = call.partition("(")
        kv = dict(a.split("=") for a in args.rstrip(")").split(",")) if args else {}
        if name == "conv2d_forward":
            out.append(("fwd", False))
        elif name == "conv2d_dgrad":
            out.append(("padded" if kv["prepadded"] == "1" else "dgrad", kv["act"] != "-"))
        elif name == "conv2d_dgrad_padded" and kv["wino"] == "0" and kv["p16"] == "0":
            out.append(("padded", False))
    return out


def splitk_forms(cfg, batch, precision, log):
    """["fwd:split", "padded:unsplit", ...]: one item per LDS-DMA launch of a log at this size, in launch order (deterministic
    mode off); empty when the log has no such launch."""
    out = []
    for what, fused in direct_launches(cfg, log):
        d = dma_launch(cfg, batch, precision, what, fused)
        if d is not None:
            out.append("%s:%s" % (what, "split" if d["ksplit"] else "unsplit"))
    return out


def thin_forms(cfg, batch, log):
    """The thin-kernel instances the C entry points pick for the direct launches of this log (fp32 and bf16 alike: the thin
    kernels sit in front of the precision switch)."""
    names = {c.partition("(")[0]: c for c in log.split(" ")}
    out = []
    if "conv2d_forward" in names:
        out.append(thin_fwd(cfg, batch))
    if "conv2d_dgrad" in names and "prepadded=1" not in names["conv2d_dgrad"]:
        out.append(thin_dgrad(cfg, batch, "res_none=0" in names["conv2d_dgrad"]))
    if "conv2d_wgrad" in names:
        out.append(thin_wgrad(cfg, batch))
    return out


def refused(cfg, log):
    """The message dvs_conv2d_fwd refuses this case with, or None.  The direct kernels' upsample + concat gather takes the two
    sources in whole 32-channel stages (csrc/conv_fwd.hip: C1 % 32 == 0 unless nothing is concatenated); conv.supported() says the
    same, nn_ops.conv2d asks it first, so the product never gets there -- but conv.conv2d plans such a launch for the ragged
    concat layer of the route table, whose recorded sequences with a direct forward therefore cannot produce a number."""
    if "conv2d_forward(" in log and isinstance(cfg["x2"], tuple) and cfg["x"][0] % BK:
        return "upsample+concat needs C1 % 32 == 0"
    return None


# ---------------------------------------------------------------------------------------------- the fp64 reference
def reference(cfg, x, w, b, x2):
    """fp64 torch composition of the layer: [upsample2x(x) (+ concat x2)] -> [reflect pad] -> conv -> act.  x, w, b, x2: fp64
    tensors (x2: None, "up" or the skip)."""
    from test_guard_kernels_gpu import _ref_conv
    refl = bool(cfg["reflect_pad"])
    p = cfg["reflect_pad"] or cfg["padding"]
    if cfg["x2"] is None:
        return _ref_conv(x, w, b, cfg["stride"], p, refl, cfg["act"])
    return _ref_conv(x2 if isinstance(x2, torch.Tensor) else None, w, b, cfg["stride"], p, refl, cfg["act"], xa=x)


# ---------------------------------------------------------------------------------------------- recording
def _full_size_twin(golden, layer, precision, switch, grads, sink, log):
    """The first full-size case of the same layer and mode with this log, or None."""
    for b in R.BATCHES:
        cid = case_id(layer, b, precision, switch, grads, sink)
        if golden.get(cid) == log:
            return cid
    return None


def _entry(layer, cfg, precision, switch, grads, sink, costs, twin, log, double=False):
    return {"layer": layer, "x": list(cfg["x"]), "x2": list(cfg["x2"]) if isinstance(cfg["x2"], tuple) else cfg["x2"],
            "batch": BATCH, "precision": precision, "switch": switch, "grads": grads, "sink": int(sink),
            "wino_pays": int(costs[0]), "dec_wgrad_pays": int(costs[1]), "stands_for": twin,
            "splitk": splitk_forms(cfg, BATCH, precision, log), "double": int(double), "refused": refused(cfg, log)}


LADDER = sorted(itertools.product((16, 32, 48, 64, 96, 128, 160, 192, 256), (32, 64, 96, 128, 160, 192, 256, 320)),
                key=lambda hw: (hw[0] * hw[1], hw))


def _full_form_cfg(layer, precision, log, twin_batch):
    """The smallest size of the ladder at which the log's launches take the forms of the full-size layer (thin-kernel instances
    and split-K), or None."""
    full = R.LAYERS[layer]
    want = thin_forms(full, twin_batch, log), splitk_forms(full, twin_batch, precision, log)
    for hw in LADDER:
        cfg = shrink(layer, hw)
        if (thin_forms(cfg, BATCH, log), splitk_forms(cfg, BATCH, precision, log)) == want:
            return cfg
    return None


def record():
    golden = golden_det0()
    mp = pytest.MonkeyPatch()
    seen, cases = {}, []
    reached = {}                    # log -> [(weight size of the layer, layer, mode...)]: who can stand for it
    for layer in R.LAYERS:
        cfg = shrink(layer)
        for costs in COSTS:
            for precision in R.PRECISIONS:
                for switch, grads, sink in R.SUB:
                    with forced_costs(*costs):
                        log = R.run_case(mp, cfg, BATCH, precision, False, switch, grads, sink)[0]
                    twin = _full_size_twin(golden, layer, precision, switch, grads, sink, log)
                    if twin is None:
                        continue        # a sequence the full-size layer never runs in this mode: stands for nothing
                    co, ci, k = cfg["w"][:3]
                    reached.setdefault(log, []).append((co * ci * k * k, layer, precision, switch, grads, sink, costs))
                    if log not in seen:
                        seen[log] = len(cases)
                        cases.append(_entry(layer, cfg, precision, switch, grads, sink, costs, twin, log))
    # the unsplit-K doubles: sequences with an LDS-DMA launch that splits K at the tiny size and, with 320 tiles or more, does not
    # at the product's size at batch 12 -- a second entry on the cheapest layer (both channel counts <= 128) that reaches it
    doubles = []
    for log, idx in seen.items():
        if not any(f.endswith(":split") for f in cases[idx]["splitk"]):
            continue
        for _, layer, precision, switch, grads, sink, costs in sorted(reached[log], key=lambda c: c[:2]):
            full, cid = R.LAYERS[layer], case_id(layer, 12, precision, switch, grads, sink)
            forms = splitk_forms(full, 12, precision, log)
            if golden.get(cid) != log or max(full["w"][:2]) > 128 or not any(f.endswith(":unsplit") for f in forms):
                continue
            cfg = _full_form_cfg(layer, precision, log, 12)
            if cfg is not None:
                doubles.append(_entry(layer, cfg, precision, switch, grads, sink, costs, cid, log, double=True))
                break
    cases += doubles
    missing = sorted(set(golden.values()) - set(seen))
    with open(SMALL, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]}\n")
    print("recorded %d cases for %d of %d sequences (+ %d unsplit-K doubles), %d unreachable, %d bytes"
          % (len(cases), len(seen), len(set(golden.values())), len(doubles), len(missing), os.path.getsize(SMALL)))
    for log in missing:
        print("  unreachable:", log)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if "--record" in sys.argv:
        record()
    else:
        print(__doc__)
