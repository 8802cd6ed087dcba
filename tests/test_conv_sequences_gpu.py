"""The numbers behind every launch sequence of tests/golden/conv_routes.json.

tests/test_conv_routes_cpu.py proves WHICH kernels conv.conv2d and its backward call for every product layer, precision mode,
switch, needs_input_grad variant and sink setting; the value tests elsewhere ask for all gradients at once with every switch at
its default.  Here each of the 386 deterministic-off sequences runs once on the GPU at a tiny size
(tests/golden/conv_small_cases.json, derived and checked by tests/conv_cases.py and tests/test_conv_small_cases_cpu.py; the
LDS-DMA sequences a second time at a size that does not split K):

  * pass-through spies around the twelve wrappers must log exactly the recorded sequence (a case that silently ran another
    sequence fails there, not in the arithmetic);
  * y, every requested gradient, sink contents and the statistics output are compared with the fp64 torch composition
    (upsample, cat, reflect pad, conv, activation) at the project's tolerances for these families: fp32 mode 2e-5 of the tensor
    max on y and the statistics, 1e-4 on gradients (tests/test_conv_gpu.py); bf16 mode y against fp64 on bf16-rounded operands
    at 2e-5, gradients against fp64 at 1e-2 (test_p16_decoder_layers);
  * the nine sequences of the ragged concat layer that begin with a direct forward are refused by dvs_conv2d_fwd (its gather
    takes the two sources in whole 32-channel stages; conv.supported() keeps the product away from them): the refusal is asserted;
  * a parameter that needs no gradient ends with .grad None, all operands sit between guard bands, all outputs are finite;
  * fp32 mode: every gradient agrees with the base-switch / all-gradients run of the same layer, inputs and cost-model setting
    to 1e-4 of the tensor max (the two kernels compute the same fp32 sum in another order).
"""
import inspect
import re
import threading

import pytest
import torch

import conv_cases as C
import guard
import test_conv_routes_cpu as R
from test_guard_kernels_gpu import _cl, r16

pytestmark = pytest.mark.gpu
CASES = C.load()
TOL = {"fp32": (2e-5, 1e-4), "bf16": (2e-5, 1e-2)}          # (y and statistics, gradients)
SELF_TOL = 1e-4

# what each spy logs: the Recorder's fields of tests/test_conv_routes_cpu.py, from the real wrappers' bound arguments
_PLAIN = ("flip", "res_none", "stat_slots", "stat_groups")
_GEN = ("flip", "full", "act", "reflect")
_WG = ("dw_none", "pooled")
_WGB = ("act", "dw_none", "db_none", "want_bias", "pooled")
FIELDS = {"conv2d_forward": ("act", "reflect", "res_none", "stat_slots", "stat_groups"),
          "conv3x3_wino": _PLAIN, "conv3x3_p16": _PLAIN, "conv3x3_wino_gen": _GEN, "conv3x3_p16_gen": _GEN,
          "conv2d_dgrad": ("split_c1", "act", "prepadded", "reflect", "res_none"),
          "conv2d_dgrad_padded": ("wino", "p16", "split_c1", "act"),
          "conv3x3_wino_wgrad": _WG, "conv3x3_p16_wgrad": _WG, "conv3x3_wino_wgrad_gen": _WGB, "conv3x3_p16_wgrad_gen": _WGB,
          "conv2d_wgrad": _WGB + ("reflect",)}
_NONE_OF = {"res_none": "residual", "dw_none": "dw_out", "db_none": "db_out"}
assert set(FIELDS) == set(R.WRAPPERS)


class Spies:
    """Pass-through wrappers around conv.py's twelve launch wrappers: each outermost call appends the `name(arg=...)` string
    the CPU recorder writes (calls a wrapper makes itself, e.g. conv2d_dgrad_padded's correlation, are its own business)."""

    def __init__(self, conv):
        self.log, self._depth, self._lock = [], 0, threading.Lock()
        self.saved = {n: getattr(conv, n) for n in R.WRAPPERS}
        for name, fn in self.saved.items():
            setattr(conv, name, self._spy(name, fn))

    def _spy(self, name, fn):
        sig = inspect.signature(fn)

        def spy(*args, **kw):
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            a = bound.arguments
            with self._lock:
                if self._depth == 0:
                    vals = [(k, a[_NONE_OF[k]] is None if k in _NONE_OF else a[k]) for k in FIELDS[name]]
                    self.log.append("%s(%s)" % (name, ",".join("%s=%s" % (k, R._fmt(v)) for k, v in vals)))
                self._depth += 1
            try:
                return fn(*args, **kw)
            finally:
                with self._lock:
                    self._depth -= 1
        return spy

    def restore(self, conv):
        for name, fn in self.saved.items():
            setattr(conv, name, fn)


@pytest.fixture
def mode():
    """apply(entry): precision, the six switches and the two cost models as the entry names them; everything restored after the
    test whatever happened."""
    from deep_visual_slam_amd import _lib, conv
    saved = {n: getattr(conv, n) for n in tuple(R.SWITCH_DEFAULTS) + ("wino_pays", "wino_dec_wgrad_pays")}
    precision = _lib.precision()

    def apply(e, switch=None):
        _lib.set_precision(e["precision"])
        switch = e["switch"] if switch is None else switch
        for name, default in R.SWITCH_DEFAULTS.items():
            setattr(conv, name, (not default) if name == switch else default)
        conv.wino_pays = lambda *a: bool(e["wino_pays"])
        conv.wino_dec_wgrad_pays = lambda *a: bool(e["dec_wgrad_pays"])
    try:
        yield apply
    finally:
        for n, v in saved.items():
            setattr(conv, n, v)
        _lib.set_precision(precision)


@pytest.fixture
def spies():
    from deep_visual_slam_amd import conv
    s = Spies(conv)
    try:
        yield s
    finally:
        s.restore(conv)


# ---------------------------------------------------------------------------------------------- operands and the fp64 reference
_REF = {}           # (layer, x shape, x2 shape): operands and fp64 results, computed once and never changed
_BASE = {}          # (layer, x shape, x2 shape, cost models): gradients of the fp32 base-switch / all-gradients run
NORM = (1 / 0.225, -0.45 / 0.225)      # the stem's fused input normalisation (model/resnet_encoder.py:102-103)


def _shape_key(e):
    return e["layer"], tuple(e["x"]), tuple(e["x2"]) if isinstance(e["x2"], list) else e["x2"]


def _reference(e):
    """CPU operands (seeded per layer and shape, He-scaled weights), cotangents, and the fp64 forward with all gradients."""
    key = _shape_key(e)
    if key in _REF:
        return _REF[key]
    cfg, B = C.entry_cfg(e), e["batch"]
    gen = torch.Generator().manual_seed(1000 + list(R.LAYERS).index(e["layer"]))
    co, ci, k, _ = cfg["w"]
    x = torch.rand((B,) + cfg["x"], generator=gen) if cfg["planar"] else torch.randn((B,) + cfg["x"], generator=gen)
    x2 = torch.randn((B,) + cfg["x2"], generator=gen) if isinstance(cfg["x2"], tuple) else cfg["x2"]
    w = torch.randn(cfg["w"], generator=gen) * (2.0 / (ci * k * k)) ** 0.5
    b = torch.randn(co, generator=gen) * 0.1 if cfg["bias"] else None
    leaves = {"x": x, "x2": x2 if isinstance(x2, torch.Tensor) else None, "w": w, "b": b}
    d = {n: t.double().requires_grad_(True) for n, t in leaves.items() if t is not None}

    def forward(xv, wv, bv, x2v):
        if cfg["planar"]:
            xv = xv * NORM[0] + NORM[1]
        return C.reference(cfg, xv, wv, bv, x2v if x2v is not None else x2)

    y64 = forward(d["x"], d["w"], d.get("b"), d.get("x2"))
    cot = torch.randn(y64.shape, generator=gen)
    cot_alias = torch.randn(x.shape, generator=gen) if cfg["passthrough"] else None
    names = [n for n in d if not (cfg["planar"] and n == "x")]
    g64 = dict(zip(names, torch.autograd.grad(y64, [d[n] for n in names], cot.double())))
    if cot_alias is not None:
        g64["x"] = g64["x"] + cot_alias.double()            # the fan-in add inside the data-gradient kernel
    with torch.no_grad():
        if cfg["planar"]:       # the kernel rounds what it stages: the normalised image
            y16 = C.reference(cfg, r16(x * NORM[0] + NORM[1]), r16(w), None, None)
        else:
            y16 = forward(r16(x), r16(w), b.double() if b is not None else None, r16(x2) if isinstance(x2, torch.Tensor) else None)
    ref = _REF[key] = {"cfg": cfg, "leaves": leaves, "x2": x2, "cot": cot, "cot_alias": cot_alias, "y": y64.detach(),
                       "y16": y16, "grads": g64}
    return ref


def _stats_ref(y, groups):
    B = y.shape[0]
    parts = [y[i * B // groups:(i + 1) * B // groups] for i in range(groups)]
    return torch.stack([torch.stack([p.sum((0, 2, 3)), (p * p).sum((0, 2, 3))]) for p in parts])       # [groups][2][C]


def relmax(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    assert torch.isfinite(a).all(), "non-finite output"
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


# ---------------------------------------------------------------------------------------------- one run on the GPU
def _run(dev, ref, grads, sinks):
    """Forward + backward of one case: {"y", "stats", "grads": {leaf: gradient}, "none": leaves that ended without .grad}."""
    from deep_visual_slam_amd import conv, gradsink, zeropool
    cfg, L = ref["cfg"], ref["leaves"]
    planar = cfg["planar"]
    x_grad = grads != "no_x" and not planar
    g = guard.Bands(dev)
    x = g.place(L["x"]) if planar else _cl(g, L["x"])
    x.requires_grad_(x_grad)
    x2 = _cl(g, L["x2"]).requires_grad_(x_grad) if L["x2"] is not None else None
    weight = torch.nn.Parameter(_cl(g, L["w"]), requires_grad=grads != "no_w")
    bias = torch.nn.Parameter(g.place(L["b"]), requires_grad=grads != "no_b") if L["b"] is not None else None
    params = {"w": weight, "b": bias}
    if sinks:
        for p in (weight, bias):
            if p is not None and p.requires_grad:
                full = torch.full(p.shape, 0.5)
                p.grad = _cl(g, full, guard.CANARY) if p.dim() == 4 else g.place(full, guard.CANARY)
                gradsink.attach(p, p.grad)
    cot = _cl(g, ref["cot"])
    cot_alias = _cl(g, ref["cot_alias"]) if ref["cot_alias"] is not None else None
    norm = tuple(g.place(torch.full((3,), v)) for v in NORM) if planar else None
    with guard.allocations(conv, zeropool) as rec:
        out = conv.conv2d(x, weight, bias, cfg["stride"], cfg["padding"], cfg["reflect_pad"], cfg["act"], x2=x2,
                          upsample=ref["x2"] == "up" if isinstance(ref["x2"], str) else False, planar_norm=norm,
                          want_stats=cfg["stats"], passthrough=cfg["passthrough"])
        out = out if isinstance(out, tuple) else (out,)
        heads = [(out[0], cot)] + ([(out[-1], cot_alias)] if cfg["passthrough"] else [])
        heads = [(t, c) for t, c in heads if t.requires_grad]
        torch.autograd.backward([t for t, _ in heads], [c for _, c in heads])
        gradsink.join()
        torch.cuda.synchronize()
    assert rec.count >= 1, rec.count
    g.check()
    res = {"y": out[0].detach(), "stats": out[1].detach() if cfg["stats"] & 3 else None, "grads": {}, "none": []}
    for name, t in (("x", x), ("x2", x2), ("w", weight), ("b", bias)):
        if t is None:
            continue
        if t.grad is None:
            res["none"].append(name)
        else:
            res["grads"][name] = (t.grad - 0.5) if sinks and name in params else t.grad
    return res


_GOLDEN = None


def _golden():
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = C.golden_det0()
    return _GOLDEN


@pytest.mark.parametrize("e", CASES, ids=[C.entry_id(e) for e in CASES])
def test_sequence_values(gpu_device, mode, spies, e):
    ref = _reference(e)
    cfg = ref["cfg"]
    mode(e)
    want_log = [c for c in _golden()[e["stands_for"]].split(" ") if c != "|" and not c.startswith("dvs_")]
    if e["refused"]:
        # conv.supported() is False for these operands (tests/test_conv_small_cases_cpu.py), the product raises before planning; the
        # sequence exists in the route table only.  Called directly, the C entry point must refuse the forward launch by name.
        from deep_visual_slam_amd import _lib
        with pytest.raises(_lib.DvsError, match=re.escape(e["refused"])):
            _run(gpu_device, ref, e["grads"], bool(e["sink"]))
        assert spies.log == want_log[:1]
        return
    res = _run(gpu_device, ref, e["grads"], bool(e["sink"]))
    assert spies.log == want_log, "ran another sequence:\n  got  %s\n  want %s" % (" ".join(spies.log), " ".join(want_log))

    tol_y, tol_g = TOL[e["precision"]]
    y_ref = ref["y16"] if e["precision"] == "bf16" else ref["y"]
    figures = {"y": relmax(res["y"], y_ref)}
    if res["stats"] is not None:
        groups = cfg["stats"] & 3
        st = res["stats"].double().cpu()
        st = st.sum(0) if st.dim() == 4 else st
        want = _stats_ref(y_ref, groups)
        figures["stats"] = max(relmax(st.reshape(groups, 2, -1)[:, i], want[:, i]) for i in range(2))
    # which leaves must have a gradient: exactly run_case's requires_grad
    planar = cfg["planar"]
    asked = {"x": e["grads"] != "no_x" and not planar, "x2": e["grads"] != "no_x" and ref["leaves"]["x2"] is not None,
             "w": e["grads"] != "no_w", "b": e["grads"] != "no_b" and cfg["bias"]}
    for name, want in asked.items():
        if ref["leaves"][name] is None:
            continue
        assert (name in res["grads"]) == want, "%s: .grad %s" % (name, "missing" if want else "present on a frozen leaf")
        if want:
            figures["d" + name] = relmax(res["grads"][name], ref["grads"][name])
    print("%s: %s" % (C.entry_id(e), " ".join("%s=%.2e" % kv for kv in figures.items())))
    for name, err in figures.items():
        assert err < (tol_y if name in ("y", "stats") else tol_g), (name, err)

    if e["precision"] == "fp32":
        key = _shape_key(e) + (e["wino_pays"], e["dec_wgrad_pays"])
        if key not in _BASE:
            if (e["switch"], e["grads"], e["sink"]) == ("base", "all", 0):
                _BASE[key] = res["grads"]
            else:
                mode(e, switch="base")
                _BASE[key] = _run(gpu_device, ref, "all", False)["grads"]
        for name, got in res["grads"].items():
            err = relmax(got, _BASE[key][name])
            assert err < SELF_TOL, ("against the base / all-gradients run", name, err)
