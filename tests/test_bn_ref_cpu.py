"""tests/bn_ref.py judged on the CPU: the fp64 restatement against fp64 autograd, the recorded K against the fp32 restatement, the
checker against planted errors (it must reject every one of them on a well-conditioned channel), and the share of elements
whose ReLU mask the forward bound leaves undecided."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn_ref as R

CASES = [(B, C, H, W, G, slots, seed) for B, C, H, W, G, slots, seeds in R.SHAPES for seed in seeds]
ids = lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# ------------------------------------------------------------------------------------------------- restatement vs autograd
def _class0(B, C, H, W, G, seed, res_bn):
    gen = torch.Generator().manual_seed(seed)
    d = dict(y=torch.randn(B, C, H, W, generator=gen, dtype=torch.float64), dz=torch.randn(B, C, H, W, generator=gen, dtype=torch.float64),
             res=torch.randn(B, C, H, W, generator=gen, dtype=torch.float64), count=B // G * H * W)
    d["aff"] = [t.double() for t in R.make_affine(C, seed)]
    d["raff"] = [t.double() for t in R.make_affine(C, seed, 3)] if res_bn else None
    return d


def _stats64(y, G):
    return torch.stack([torch.stack([p.sum((0, 2, 3)), (p * p).sum((0, 2, 3))]) for p in y.chunk(G, 0)])


def _module(aff):
    m = nn.BatchNorm2d(aff[0].numel(), eps=R.EPS, momentum=R.MOMENTUM).double().train()
    with torch.no_grad():
        m.weight.copy_(aff[0]); m.bias.copy_(aff[1]); m.running_mean.copy_(aff[2]); m.running_var.copy_(aff[3])
    return m


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_autograd_in_fp64(mode, G):
    """Class 0 only, statistics computed from y in fp64: forward, running statistics (G = 2: two successive module calls) and
    every gradient within 1e-10 relative of F.batch_norm (+ residual, + relu) under autograd."""
    B, C, H, W = 4, 16, 5, 7
    d = _class0(B, C, H, W, G, 11, mode == "res_bn")
    y, res = d["y"].clone().requires_grad_(True), d["res"].clone().requires_grad_(mode in ("residual", "res_bn"))
    m, mr = _module(d["aff"]), (_module(d["raff"]) if mode == "res_bn" else None)
    u = torch.cat([m(p) for p in y.chunk(G, 0)])
    if mode == "residual":
        u = u + res
    elif mode == "res_bn":
        u = u + torch.cat([mr(p) for p in res.chunk(G, 0)])
    z = F.relu(u) if mode != "plain" else u
    leaves = [y, m.weight, m.bias] + ([res] if res.requires_grad else []) + ([mr.weight, mr.bias] if mr is not None else [])
    grads = torch.autograd.grad(z, leaves, d["dz"])

    rt = R.finalize(_stats64(d["res"], G), d["count"], d["raff"][0], d["raff"][1]) if mode == "res_bn" else None
    f = R.forward(d["y"], _stats64(d["y"], G), d["count"], d["aff"][0], d["aff"][1], R.EPS, R.MOMENTUM, d["aff"][2], d["aff"][3],
                  mode != "plain", d["res"] if mode != "plain" and mode != "relu" else None, rt)
    assert rel(f["z"], z.detach()) < 1e-10
    assert rel(f["running_mean"], m.running_mean) < 1e-10 and rel(f["running_var"], m.running_var) < 1e-10
    assert f["G"] == int(m.num_batches_tracked) == G
    b = R.backward(d["dz"], (z.detach() > 0) if mode != "plain" else None, d["y"], f["tab"],
                   d["res"] if res.requires_grad else None, rt)
    names = ["dy", "dgamma", "dbeta"] + (["dres"] if mode == "residual" else []) + (["r_dy", "r_dgamma", "r_dbeta"] if mr is not None else [])
    for nm, g in zip(names, grads):
        assert rel(b[nm], g) < 1e-10, (nm, rel(b[nm], g))
    if mr is not None:
        rr = R.running(rt, R.MOMENTUM, d["raff"][2], d["raff"][3])
        assert rel(rr["running_mean"], mr.running_mean) < 1e-10 and rel(rr["running_var"], mr.running_var) < 1e-10


@pytest.mark.parametrize("B,H,W,G", [(2, 7, 9, 1), (4, 6, 5, 2), (2, 2, 2, 2)])
def test_stem_restatement_equals_autograd_in_fp64(B, H, W, G):
    """relu(bn(y)) -> F.max_pool2d(3, 2, 1) with a cotangent on the pooled map and a second one on z."""
    C = 8
    d = _class0(B, C, H, W, G, 12, False)
    y, m = d["y"].clone().requires_grad_(True), _module(d["aff"])
    z = F.relu(torch.cat([m(p) for p in y.chunk(G, 0)]))
    p = F.max_pool2d(z, 3, 2, 1)
    dpool = torch.randn(p.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    grads = torch.autograd.grad([p, z], [y, m.weight, m.bias], [dpool, d["dz"]])
    f = R.stem_forward(d["y"], _stats64(d["y"], G), d["count"], *d["aff"][:2], R.EPS, R.MOMENTUM, *d["aff"][2:])
    assert rel(f["z"], z.detach()) < 1e-10 and rel(f["pooled"], p.detach()) < 1e-10
    assert rel(f["running_var"], m.running_var) < 1e-10
    b = R.stem_backward(dpool, f["idx"], d["dz"], z.detach() > 0, d["y"], f["tab"])
    for nm, g in zip(("dy", "dgamma", "dbeta"), grads):
        assert rel(b[nm], g) < 1e-10, (nm, rel(b[nm], g))


def test_first_maximum_in_scan_order():
    z = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    z[0, 0, 0, 1] = z[0, 0, 1, 0] = 2.0
    pooled, idx = R.max_pool(z)
    assert pooled[0, 0, 0, 0] == 2.0 and int(idx[0, 0, 0, 0]) == 5          # window (0, 0): taps 5 = (0, 1) and 7 = (1, 0) tie
    assert int(idx[0, 0, 1, 0]) == 3                                         # window (0, 1): row -1 is outside, (0, 1) is tap 3
    assert int(idx[0, 1, 1, 0]) == 0                                         # window (1, 1): (1, 1) .. (2, 2), all zero: the first


# ------------------------------------------------------------------------------------------------------------- calibration
def test_recorded_K_is_four_times_the_recorded_ratio():
    for fam, k in R.K.items():
        ks, ms = (k, R.MEASURED[fam]) if isinstance(k, tuple) else ((k,), (R.MEASURED[fam],))
        for kv, mv in zip(ks, ms):
            assert kv == pytest.approx(max(16.0, 4 * mv), rel=2e-3), (fam, kv, mv)
    assert R.K["fwd"][0] <= R.K["fwd"][1] and R.K["bwd"][0] <= R.K["bwd"][1]


def _calibrate(c, fwd, bwd_of):
    ref, f32 = fwd(torch.float64), fwd(torch.float32)
    worst = R.check_items(R.forward_items(R.fwd_tensors(f32), ref), c["count"], c["classes"], c["rclasses"])
    mask = f32["z"] > 0 if c["relu"] else None
    rb = bwd_of(ref, f32, mask, torch.float64, "seq")
    for order in ("seq", "pair64"):
        worst = max(worst, R.check_items(R.backward_items(bwd_of(f32, f32, mask, torch.float32, order), rb), c["count"], c["classes"],
                                         c["rclasses"], order + " "))
    return worst


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_fp32_restatement_passes_with_the_recorded_K(case, mode):
    c = R.make_case(*case, mode)
    worst = _calibrate(c, lambda dt: R.run_forward(c, dt), lambda t, f, mask, dt, order: R.run_backward(c, t, mask, dt, order))
    assert worst <= 1.0


@pytest.mark.parametrize("shape", R.STEM_SHAPES, ids=ids)
def test_fp32_stem_restatement_passes_with_the_recorded_K(shape):
    c = R.stem_case(*shape)
    worst = _calibrate(c, lambda dt: R.stem_forward(*c["args"], dtype=dt),
                       lambda t, f, mask, dt, order: R.stem_backward(c["dpool"], f["idx"], c["dz"], mask, c["y"], t["tab"], dt, order))
    assert worst <= 1.0


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_fp32_sums_pass_with_the_recorded_K(case):
    B, C, H, W, G, slots, seed = case
    for order in ("seq", "pair64"):
        for r in R.sum_ratios(R.make_y(B, C, H, W, seed), G, order):
            assert float(r.max()) <= R.K["sum"]


# ----------------------------------------------------------------------------------------------------------------- mutants
def _rejections(items, count, classes, rclasses=None):
    """{(quantity, class)} of the regular, well-conditioned channels on which check_channels would fail."""
    out = set()
    for name, g, r, kap, sc, fam, tk in items:
        over = R.channel_ratios(g, r, kap, sc) / R.tier_K(fam, tk, count)
        cls = rclasses if (name.startswith("r_") and rclasses is not None) else classes
        reg = R.regular(tk, count).expand_as(over) if tk is not None else torch.ones_like(over, dtype=torch.bool)
        for k in R.WELL:
            if bool(((over > 1) & reg)[:, cls == k].any()):
                out.add((name, k))
    return out


def _neighbour(t):
    """Every channel's result written to its neighbour within the 4-channel vector (c ^ 1)."""
    return t[:, torch.arange(t.shape[1]) ^ 1]


S16, S64G2, S128 = (2, 16, 5, 7, 1, 1, 0), (2, 64, 9, 10, 2, 17, 3), (4, 128, 3, 5, 2, 24, 4)
MUTANTS = [
    # name, case, mode, where the error is planted ("fwd" / "bwd": the restatement's mutant flag; else a function of the outputs)
    ("no_eps", S16, "relu", "fwd"), ("eps1e-6", S16, "relu", "fwd"), ("unbiased_norm", S16, "plain", "fwd"),
    ("biased_running", S16, "plain", "fwd"), ("count+1", S16, "residual", "fwd"), ("momentum_once", S64G2, "relu", "fwd"),
    ("group0_table", S64G2, "relu", "fwd"), ("res_identity", S128, "res_bn", "fwd"), ("mask_ge", S16, "relu", "mask"),
    ("no_xhat_term", S16, "relu", "bwd"), ("swap_affine", S16, "plain", "bwd"), ("neighbour", S128, "relu", "z"),
    ("slots16", S64G2, "plain", "fwd"),
]


@pytest.mark.parametrize("mutant,case,mode,where", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_checker_rejects_mutant(mutant, case, mode, where):
    """The fp32 restatement with one planted error must fail check_channels on at least one channel of a well-conditioned class
    (0-3) of the regular tier; without the error the same run passes (the calibration tests)."""
    c = R.make_case(*case, mode)
    ref = R.run_forward(c)
    f32 = R.run_forward(c, torch.float32, mutant if where == "fwd" else None)
    got = R.fwd_tensors(f32)
    if where == "z":
        got["z"] = _neighbour(got["z"])
    rej = _rejections(R.forward_items(got, ref), c["count"], c["classes"], c["rclasses"])
    if where in ("bwd", "mask"):
        assert not rej, rej                                          # the forward is untouched
        mask = f32["z"] > 0
        rb = R.run_backward(c, ref, mask if c["relu"] else None)
        bad = (f32["z"] >= 0) if where == "mask" else (mask if c["relu"] else None)
        b32 = R.run_backward(c, f32, bad, torch.float32, "seq", mutant if where == "bwd" else None)
        rej = _rejections(R.backward_items(b32, rb), c["count"], c["classes"], c["rclasses"])
    print("mutant %-15s rejected on %s" % (mutant, sorted(rej)))
    assert rej, "mutant %s passed the checker" % mutant


def test_mutants_cover_the_list():
    assert len({m[0] for m in MUTANTS}) == 13


# ----------------------------------------------------------------------------------------------------- undecided elements
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_few_elements_are_left_undecided(case, mode):
    """Channels with kappa <= 1e3: at most 1e-3 of the elements have |z64| below the forward bound (their ReLU mask is open)."""
    c = R.make_case(*case, mode)
    share, decided = R.undecided(R.run_forward(c), c["count"])
    assert share <= 1e-3, share


@pytest.mark.parametrize("shape", R.STEM_SHAPES, ids=ids)
def test_few_stem_elements_are_left_undecided(shape):
    c = R.stem_case(*shape)
    share, decided = R.undecided(R.stem_forward(*c["args"]), c["count"])
    assert share <= 1e-3, share
