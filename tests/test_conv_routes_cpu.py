"""Which kernel every convolution runs on, pinned without a GPU.

conv.conv2d(...) and its backward are driven on CPU tensors with the launch layer replaced by recorders: every conv* wrapper
and every dvs_* entry point appends its name and its routing arguments to a log instead of launching.  The expected logs, the
gradients that come back as None and the shapes live in tests/golden/conv_routes.json, recorded once
(`python tests/test_conv_routes_cpu.py --record`) and never regenerated: a change of conv.py that sends one layer of one
network to another kernel, in any mode, fails here.

The cases are the table below (LAYERS x BATCHES x PRECISIONS x DETERMINISTIC x SWITCHES x GRADS x SINKS), not anything derived
from the code under test.
"""
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_routes.json")
CL = torch.channels_last
SLOTTED = 4             # conv.STATS_SLOTTED, spelled out: the table does not read the module under test


def _layer(x, w, bias=False, stride=1, padding=0, reflect_pad=0, act=None, x2=None, planar=False, stats=0, passthrough=False):
    """x: (C, H, W) of the first operand; w: (Cout, Cin, k, k); x2: None, "up" (upsample only) or the skip's (C, H, W)."""
    return dict(x=x, w=w, bias=bias, stride=stride, padding=padding, reflect_pad=reflect_pad, act=act, x2=x2, planar=planar,
                stats=stats, passthrough=passthrough)


def _layers():
    """Every distinct convolution configuration of the product networks at 480 x 640."""
    L = {"stem": _layer((3, 480, 640), (64, 3, 7, 7), stride=2, padding=3, planar=True, stats=2 | SLOTTED)}
    # ResNet-18 BasicBlock 3x3 layers: stride 1 at the four widths, stride 2 into layers 2-4
    res = [("l1", 64, 64, 120, 160, 1), ("l2", 128, 128, 60, 80, 1), ("l3", 256, 256, 30, 40, 1), ("l4", 512, 512, 15, 20, 1),
           ("l2s", 64, 128, 120, 160, 2), ("l3s", 128, 256, 60, 80, 2), ("l4s", 256, 512, 30, 40, 2)]
    for name, ci, co, h, w, s in res:
        for st in (0, 1 | SLOTTED, 2 | SLOTTED):
            L["%s_st%d" % (name, st & 3)] = _layer((ci, h, w), (co, ci, 3, 3), stride=s, padding=1, stats=st)
        if s == 1:
            L["%s_st2_pt" % name] = _layer((ci, h, w), (co, ci, 3, 3), stride=s, padding=1, stats=2 | SLOTTED, passthrough=True)
    L["l1_st0_pt"] = _layer((64, 120, 160), (64, 64, 3, 3), padding=1, passthrough=True)
    # the 1x1 stride-2 downsample branches
    for name, ci, co, h, w in [("ds2", 64, 128, 120, 160), ("ds3", 128, 256, 60, 80), ("ds4", 256, 512, 30, 40)]:
        L[name] = _layer((ci, h, w), (co, ci, 1, 1), stride=2, stats=2 | SLOTTED)
        L[name + "_pt"] = _layer((ci, h, w), (co, ci, 1, 1), stride=2, stats=2 | SLOTTED, passthrough=True)
    # the decoder's Conv3x3 levels, (Cin, Cout, H, W) of upconv_4_0 ... upconv_1_1 (tests/test_hostlogic_cpu.py's `dec` list), each
    # as a plain layer, with the nearest-2x upsample in the gather, and with upsample + skip concat (coarse channels first)
    dec = [(512, 256, 15, 20), (512, 256, 30, 40), (256, 128, 30, 40), (256, 128, 60, 80), (128, 64, 60, 80), (128, 64, 120, 160),
           (64, 32, 120, 160), (96, 32, 240, 320)]
    for i, (ci, co, h, w) in enumerate(dec):
        c1 = 32 if ci == 96 else ci // 2
        hh, wh = h // 2, w // 2
        kw = dict(bias=True, reflect_pad=1, act="elu")
        L["dec%d" % i] = _layer((ci, h, w), (co, ci, 3, 3), **kw)
        L["dec%d_up" % i] = _layer((ci, hh, wh), (co, ci, 3, 3), x2="up", **kw)
        L["dec%d_skip" % i] = _layer((c1, hh, wh), (co, ci, 3, 3), x2=(ci - c1, 2 * hh, 2 * wh), **kw)
    # the thin 32- and 16-channel decoder layers
    L["thin32"] = _layer((32, 240, 320), (16, 32, 3, 3), bias=True, reflect_pad=1, act="elu")
    L["thin32_up"] = _layer((32, 120, 160), (16, 32, 3, 3), bias=True, reflect_pad=1, act="elu", x2="up")
    L["thin16"] = _layer((16, 480, 640), (16, 16, 3, 3), bias=True, reflect_pad=1, act="elu")
    L["thin16_up"] = _layer((16, 240, 320), (16, 16, 3, 3), bias=True, reflect_pad=1, act="elu", x2="up")
    L["thin16_noact"] = _layer((16, 480, 640), (16, 16, 3, 3), bias=True, reflect_pad=1)
    # PoseNet: squeeze 1x1, then bias + ReLU 3x3 layers
    L["pose_squeeze"] = _layer((512, 15, 20), (256, 512, 1, 1), bias=True, act="relu")
    L["pose0"] = _layer((512, 15, 20), (256, 512, 3, 3), bias=True, padding=1, act="relu")
    L["pose1"] = _layer((256, 15, 20), (256, 256, 3, 3), bias=True, padding=1, act="relu")
    # ragged shapes that fail every fast path
    L["ragged_skip"] = _layer((72, 3, 2), (80, 128, 3, 3), bias=True, reflect_pad=1, act="elu", x2=(56, 6, 4))
    L["ragged"] = _layer((72, 3, 2), (80, 72, 3, 3), bias=True, padding=1)
    return L


LAYERS = _layers()
BATCHES = (1, 2, 4, 12)
PRECISIONS = ("fp32", "bf16")
DETERMINISTIC = (False, True)
SWITCH_DEFAULTS = {"_WINO": True, "_WINO_FORCE": False, "_P16": True, "_WGRAD_ORDERED": False, "_PREACT": True, "_PADDED": True}
SWITCHES = ("base",) + tuple(SWITCH_DEFAULTS)          # base, then each switch flipped once
GRADS = ("all", "no_x", "no_w", "no_b")                # needs_input_grad variants: input without grad, frozen weight, no bias grad
SINKS = (False, True)                                  # gradient sinks attached (with a pre-existing .grad)
SUB = list(itertools.product(SWITCHES, GRADS, SINKS))  # the order of one group's code string in the golden file
CODES = "".join(chr(c) for c in range(35, 127) if chr(c) != "\\")

WRAPPERS = ("conv2d_forward", "conv3x3_wino", "conv3x3_p16", "conv3x3_wino_gen", "conv3x3_p16_gen", "conv2d_dgrad",
            "conv2d_dgrad_padded", "conv3x3_wino_wgrad", "conv3x3_p16_wgrad", "conv3x3_wino_wgrad_gen", "conv3x3_p16_wgrad_gen",
            "conv2d_wgrad")


# ---------------------------------------------------------------------------------------------- the recording launch layer
def _fmt(v):
    if v is None:
        return "-"
    if isinstance(v, bool):
        return str(int(v))
    return str(v)


def _empty(shape):
    return torch.empty(tuple(shape), memory_format=CL) if len(shape) == 4 else torch.empty(tuple(shape))


def _gather_hw(x, x2):
    """Logical input (channels, H, W) of a gather: x alone, 2x-upsampled, or upsampled and concatenated with the skip."""
    c, h, w = x.shape[1:]
    if x2 is None:
        return c, h, w
    return c + (x2.shape[1] if isinstance(x2, torch.Tensor) else 0), 2 * h, 2 * w


class Recorder:
    """Stand-ins for conv.py's wrappers (same signatures): log the name and the routing arguments, return torch.empty of the
    shape the kernel would have produced."""

    def __init__(self):
        self.log = []

    def note(self, name, **kw):
        self.log.append("%s(%s)" % (name, ",".join("%s=%s" % (k, _fmt(v)) for k, v in kw.items())))

    def conv2d_forward(self, x, weight, bias=None, stride=1, pad=0, reflect=False, act=None, x2=None, in_scale=None, in_shift=None,
                       in_relu=False, nchw_planar=False, stats=None, stat_groups=1, residual=None, stat_slots=1):
        self.note("conv2d_forward", act=act, reflect=reflect, res_none=residual is None, stat_slots=stat_slots, stat_groups=stat_groups)
        _, h, w = _gather_hw(x, x2)
        co, _, kh, kw_ = weight.shape
        return _empty((x.shape[0], co, (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw_) // stride + 1))

    def _plain(self, name, x, weight, flip, residual, stat_slots, stat_groups):
        self.note(name, flip=flip, res_none=residual is None, stat_slots=stat_slots, stat_groups=stat_groups)
        return _empty((x.shape[0], weight.shape[1 if flip else 0]) + tuple(x.shape[2:]))

    def conv3x3_wino(self, x, weight, stats=None, stat_groups=0, flip=False, residual=None, bias=None, relu=False, stat_slots=1):
        return self._plain("conv3x3_wino", x, weight, flip, residual, stat_slots, stat_groups)

    def conv3x3_p16(self, x, weight, stats=None, stat_groups=0, flip=False, residual=None, stat_slots=1):
        return self._plain("conv3x3_p16", x, weight, flip, residual, stat_slots, stat_groups)

    def _gen(self, name, x, x2, weight, act, reflect, full, flip):
        self.note(name, flip=flip, full=full, act=act, reflect=reflect)
        _, h, w = _gather_hw(x, x2)
        return _empty((x.shape[0], weight.shape[1 if flip else 0], h + 2 * full, w + 2 * full))

    def conv3x3_wino_gen(self, x, x2, weight, bias=None, act=None, reflect=True, full=False, flip=False):
        return self._gen("conv3x3_wino_gen", x, x2, weight, act, reflect, full, flip)

    def conv3x3_p16_gen(self, x, x2, weight, bias=None, act=None, reflect=True, full=False, flip=False, dact_y=None, dact=None):
        return self._gen("conv3x3_p16_gen", x, x2, weight, act, reflect, full, flip)

    @staticmethod
    def _dx(x_shape, split_c1):
        B, C, H, W = x_shape
        if split_c1:
            return _empty((B, split_c1, H // 2, W // 2)), (_empty((B, C - split_c1, H, W)) if split_c1 < C else None)
        return _empty(x_shape)

    def conv2d_dgrad(self, dy, weight, x_shape, stride, pad, reflect, y_out=None, act=None, split_c1=0, prepadded=False, residual=None):
        self.note("conv2d_dgrad", split_c1=split_c1, act=act, prepadded=prepadded, reflect=reflect, res_none=residual is None)
        return self._dx(x_shape, split_c1)

    def conv2d_dgrad_padded(self, dz, weight, x_shape, split_c1=0, wino=False, p16=False, y_out=None, act=None):
        self.note("conv2d_dgrad_padded", wino=wino, p16=p16, split_c1=split_c1, act=act)
        return self._dx(x_shape, split_c1)

    def _wgrad(self, name, weight_shape, dw_out, pooled):
        self.note(name, dw_none=dw_out is None, pooled=pooled)
        return None if dw_out is not None else _empty(weight_shape)

    def conv3x3_wino_wgrad(self, x, dy, weight_shape, dw_out=None, pooled=False):
        return self._wgrad("conv3x3_wino_wgrad", weight_shape, dw_out, pooled)

    def conv3x3_p16_wgrad(self, x, dy, weight_shape, dw_out=None, pooled=False):
        return self._wgrad("conv3x3_p16_wgrad", weight_shape, dw_out, pooled)

    def _wgrad_b(self, name, weight_shape, dw_out, db_out, want_bias, pooled, act, **more):
        self.note(name, act=act, dw_none=dw_out is None, db_none=db_out is None, want_bias=want_bias, pooled=pooled, **more)
        return (None if dw_out is not None else _empty(weight_shape),
                None if db_out is not None or not want_bias else _empty((weight_shape[0],)))

    def conv3x3_wino_wgrad_gen(self, x, x2, dy, weight_shape, dw_out=None, pooled=False, y_out=None, act=None, want_bias=False, db_out=None):
        return self._wgrad_b("conv3x3_wino_wgrad_gen", weight_shape, dw_out, db_out, want_bias, pooled, act)

    def conv3x3_p16_wgrad_gen(self, x, x2, dy, weight_shape, dw_out=None, pooled=False, y_out=None, act=None, want_bias=False, db_out=None):
        return self._wgrad_b("conv3x3_p16_wgrad_gen", weight_shape, dw_out, db_out, want_bias, pooled, act)

    def conv2d_wgrad(self, x, dy, weight_shape, stride, pad, reflect, want_bias, y_out=None, act=None, x2=None, in_scale=None,
                     in_shift=None, in_relu=False, nchw_planar=False, pooled=False, dw_out=None, db_out=None):
        return self._wgrad_b("conv2d_wgrad", weight_shape, dw_out, db_out, want_bias, pooled, act, reflect=reflect)


class FakeLib:
    """libdvslam_hip.so: every dvs_* entry point records its name and reports success."""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        if not name.startswith("dvs_"):
            raise AttributeError(name)

        def call(*args):
            self._rec.log.append(name)
            return 0
        return call


# ---------------------------------------------------------------------------------------------- one case
def _shapes(ts):
    return " ".join("-" if t is None else "x".join(map(str, t.shape)) for t in ts)


def _noted(into, grads):
    """Keep the shapes only: a second reference to a gradient would make autograd copy it instead of adopting it."""
    into.append(_shapes(grads[:4]))
    return grads


def run_case(mp, cfg, batch, precision, deterministic, switch, grads, sinks):
    """(call log, shapes of the forward outputs | shapes of the returned gradients, '-' for None) of one forward + backward."""
    from deep_visual_slam_amd import _lib, conv, gradsink
    rec = Recorder()
    fake = FakeLib(rec)
    with mp.context() as m:
        for name in WRAPPERS:
            m.setattr(conv, name, getattr(rec, name))
        m.setattr(_lib, "lib", lambda: fake)
        m.setattr(_lib, "stream", lambda: None)
        m.setattr(gradsink, "cur_stream", lambda: None)
        m.setattr(gradsink, "_enabled", False)          # the inline weight-gradient branch (side streams need a GPU)
        m.setattr(_lib, "_precision", precision)
        m.setattr(_lib, "_deterministic", deterministic)
        for name, default in SWITCH_DEFAULTS.items():
            m.setattr(conv, name, (not default) if name == switch else default)
        returned = []
        real_backward = conv._Conv2d.backward
        m.setattr(conv._Conv2d, "backward", staticmethod(lambda ctx, *g: _noted(returned, real_backward(ctx, *g))))

        planar = cfg["planar"]
        x_grad = grads != "no_x" and not planar          # the planar image input has no gradient path
        x = torch.empty((batch,) + cfg["x"]) if planar else _empty((batch,) + cfg["x"])
        x.requires_grad_(x_grad)
        x2 = cfg["x2"]
        if isinstance(x2, tuple):
            x2 = _empty((batch,) + x2).requires_grad_(x_grad)
        weight = torch.nn.Parameter(_empty(cfg["w"]), requires_grad=grads != "no_w")
        bias = torch.nn.Parameter(torch.empty(cfg["w"][0]), requires_grad=grads != "no_b") if cfg["bias"] else None
        if sinks:
            for p in (weight, bias):
                if p is not None and p.requires_grad:
                    p.grad = torch.empty_like(p)
                    gradsink.attach(p, p.grad)
        out = conv.conv2d(x, weight, bias, cfg["stride"], cfg["padding"], cfg["reflect_pad"], cfg["act"],
                          x2=x2 if isinstance(x2, torch.Tensor) else None, upsample=x2 == "up" if isinstance(x2, str) else False,
                          planar_norm=(torch.empty(3), torch.empty(3)) if planar else None, want_stats=cfg["stats"],
                          passthrough=cfg["passthrough"])
        out = out if isinstance(out, tuple) else (out,)
        rec.log.append("|")
        heads = [out[0]] + ([out[-1]] if cfg["passthrough"] else [])      # y and, with passthrough, the alias of x
        heads = [t for t in heads if t.requires_grad]
        if heads:
            torch.autograd.backward(heads, [torch.empty_like(t) for t in heads])
        return " ".join(rec.log), _shapes(out) + " | " + (returned[0] if returned else "")


def case_ids(layer):
    for b, p, d in itertools.product(BATCHES, PRECISIONS, DETERMINISTIC):
        for sw, g, s in SUB:
            yield "%s|b%d|%s|det%d|%s|%s|sink%d" % (layer, b, p, d, sw, g, s), (b, p, d, sw, g, s)


def run_layer(mp, layer):
    return {cid: run_case(mp, LAYERS[layer], *args) for cid, args in case_ids(layer)}


# ---------------------------------------------------------------------------------------------- the golden file
# {"logs": [...], "shapes": [...], "groups": {"<layer>|b<batch>": {"outcomes": ["<log index>.<shape index>", ...],
#                                                                 "cases": {"<precision>|det<0/1>": one CODES character per SUB entry}}}}
def expand_golden():
    """case id -> (call log, shapes)."""
    with open(GOLDEN) as f:
        g = json.load(f)
    want = {}
    for group, ent in g["groups"].items():
        outcomes = [tuple(int(i) for i in o.split(".")) for o in ent["outcomes"]]
        for mode, codes in ent["cases"].items():
            assert len(codes) == len(SUB)
            for (sw, gr, s), ch in zip(SUB, codes):
                li, si = outcomes[CODES.index(ch)]
                want["%s|%s|%s|%s|sink%d" % (group, mode, sw, gr, s)] = (g["logs"][li], g["shapes"][si])
    return want


def record():
    logs, shapes, groups = {}, {}, {}
    mp = pytest.MonkeyPatch()
    for layer in LAYERS:
        for cid, res in run_layer(mp, layer).items():
            parts = cid.split("|")
            ent = groups.setdefault("|".join(parts[:2]), {"outcomes": {}, "cases": {}})
            key = "%d.%d" % (logs.setdefault(res[0], len(logs)), shapes.setdefault(res[1], len(shapes)))
            mode = "|".join(parts[2:4])
            ent["cases"][mode] = ent["cases"].get(mode, "") + CODES[ent["outcomes"].setdefault(key, len(ent["outcomes"]))]
    for ent in groups.values():
        ent["outcomes"] = list(ent["outcomes"])
    with open(GOLDEN, "w") as f:
        json.dump({"logs": list(logs), "shapes": list(shapes), "groups": groups}, f, separators=(",", ":"))
        f.write("\n")
    print("recorded %d cases, %d distinct logs, %d bytes" % (sum(len(c) for e in groups.values() for c in e["cases"].values()), len(logs),
                                                             os.path.getsize(GOLDEN)))


# ---------------------------------------------------------------------------------------------- the tests
_WANT = None


def _want():
    global _WANT
    if _WANT is None:
        _WANT = expand_golden()
    return _WANT


@pytest.mark.parametrize("layer", list(LAYERS))
def test_routes_match_the_recorded_ones(layer, monkeypatch):
    want = _want()
    got = run_layer(monkeypatch, layer)         # a case that raises fails the test
    missing = [cid for cid in got if cid not in want]
    assert not missing, "cases without a recorded expectation: %s" % missing[:5]
    wrong = ["%s\n   got  %s\n   want %s" % (cid, got[cid], want[cid]) for cid in got if got[cid] != want[cid]]
    assert not wrong, "%d of %d cases changed route:\n%s" % (len(wrong), len(got), "\n".join(wrong[:10]))


def test_the_table_is_complete_and_reaches_every_kernel_family():
    want = _want()
    ids = [cid for layer in LAYERS for cid, _ in case_ids(layer)]
    assert len(ids) == len(set(ids)) == len(LAYERS) * len(BATCHES) * len(PRECISIONS) * len(DETERMINISTIC) * len(SUB)
    assert set(ids) == set(want)                         # no case dropped, none recorded that the table no longer has
    calls = {c.split("(")[0] for log, _ in want.values() for c in log.split(" ")}
    for name in WRAPPERS + ("dvs_act_bwd",):
        assert name in calls, "%s is reached by no case" % name


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if "--record" in sys.argv:
        record()
    else:
        print(__doc__)
