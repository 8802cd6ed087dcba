"""SmallRAFT's update block on the GPU (raft_update.py / csrc/gru.hip) against tests/raft_update_ref.py in fp64: the four gate
entry points alone through the C ABI, the 7x7 four-channel convolution alone, one step, three chained steps, the hoisted context
term, and the fixture the reference's own SmallUpdateBlock produced."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import raft_update_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
CL = torch.channels_last
FIXTURE = "raft_update_h20_p36_5x7.npz"


# ---- G1: the gate kernels alone ---------------------------------------------------------------------------------------------
def tile_pixels(hidden):
    """T: a workgroup of csrc/gru.hip is 256 threads of 4 channels each over the flat [P][hidden] index space, so it covers
    1024 / hidden pixels (rounded up here): P = T - 1 is one workgroup, T and T + 1 spill into a second one."""
    return -(-1024 // hidden)


def gate_formulas(t, hd):
    """The issue's formulas on a dict of operands of one dtype (the association of the sums is the header's)."""
    o = {}
    o["z"] = torch.sigmoid((t["a_h"][:, :hd] + t["a_x"][:, :hd]) + t["c"][:, :hd])
    o["r"] = torch.sigmoid((t["a_h"][:, hd:] + t["a_x"][:, hd:2 * hd]) + t["c"][:, hd:2 * hd])
    o["rh"] = o["r"] * t["h"]
    return o


def blend_formulas(t, z, hd):
    o = {"q": torch.tanh((t["a_q"] + t["a_x"][:, 2 * hd:]) + t["c"][:, 2 * hd:])}
    o["h_new"] = (1 - z) * t["h"] + z * o["q"]
    return o


def blend_bwd_formulas(g, z, q, h):
    return {"dq": g * z * (1 - q * q), "dz": g * (q - h) * z * (1 - z), "dh_a": g * (1 - z)}


def gates_bwd_formulas(d_rh, h, r, dh_a):
    return {"dr": d_rh * h * r * (1 - r), "dh": dh_a + d_rh * r}


def gate_operands(P, hd, seed, sigma=3.0):
    gen = torch.Generator().manual_seed(seed)
    shapes = {"a_h": 2 * hd, "a_x": 3 * hd, "c": 3 * hd, "a_q": hd, "h": hd, "g": hd, "d_rh": hd}
    return {k: sigma * torch.randn(P, n, generator=gen) for k, n in shapes.items()}


def run_gate_kernels(lib, t, hd, dev):
    """All four entry points on fp32 operands `t`; each backward kernel reads what the forward kernels wrote.  Returns CPU tensors:
    the outputs by the names of the formulas, plus dpre / dah as the kernels assembled them."""
    from deep_visual_slam_amd import _lib
    P = t["h"].shape[0]
    d = {k: v.to(dev).contiguous() for k, v in t.items()}
    new = lambda n: torch.full((P, n), float("nan"), device=dev)
    o = {k: new(hd) for k in ("z", "r", "rh", "q", "h_new", "dq", "dh_a", "dh")}
    o["dpre"], o["dah"] = new(3 * hd), new(2 * hd)
    p = lambda x: x.data_ptr()
    st = _lib.stream()
    _lib.check(lib.dvs_gru_gates_fwd(p(d["a_h"]), p(d["a_x"]), p(d["c"]), p(d["h"]), p(o["z"]), p(o["r"]), p(o["rh"]), P, hd, st), "gates_fwd")
    _lib.check(lib.dvs_gru_blend_fwd(p(d["a_q"]), p(d["a_x"]), p(d["c"]), p(o["z"]), p(d["h"]), p(o["q"]), p(o["h_new"]), P, hd, st),
               "blend_fwd")
    _lib.check(lib.dvs_gru_blend_bwd(p(d["g"]), p(o["z"]), p(o["q"]), p(d["h"]), p(o["dpre"]), p(o["dah"]), p(o["dq"]), p(o["dh_a"]),
                                     P, hd, st), "blend_bwd")
    _lib.check(lib.dvs_gru_gates_bwd(p(d["d_rh"]), p(d["h"]), p(o["r"]), p(o["dh_a"]), p(o["dpre"]), p(o["dah"]), p(o["dh"]), P, hd, st),
               "gates_bwd")
    torch.cuda.synchronize()
    o = {k: v.cpu() for k, v in o.items()}
    o["dz"], o["dr"] = o["dah"][:, :hd], o["dah"][:, hd:]
    return o


def gate_references(t, got, hd):
    """{name: (fp64, fp32)} of every kernel output.  Each kernel is judged on the operands IT read: the backward formulas take the
    fp32 z, q, r, dh_a that the GPU kernels before them wrote, so one kernel's rounding is never charged to the next."""
    res = {}
    for dt in (torch.float64, torch.float32):
        c = {k: v.to(dt) for k, v in t.items()}
        o = gate_formulas(c, hd)
        o.update(blend_formulas(c, got["z"].to(dt), hd))
        o.update(blend_bwd_formulas(c["g"], got["z"].to(dt), got["q"].to(dt), c["h"]))
        o.update(gates_bwd_formulas(c["d_rh"], c["h"], got["r"].to(dt), got["dh_a"].to(dt)))
        for k, v in o.items():
            res.setdefault(k, []).append(v)
    return res


GATE_CASES = [(hd, P) for hd in (4, 20, 96) for P in (tile_pixels(hd) - 1, tile_pixels(hd), tile_pixels(hd) + 1, 1009)]


@pytest.mark.parametrize("hd,P", GATE_CASES, ids=["h%d_P%d" % c for c in GATE_CASES])
def test_gate_kernels_against_the_formulas(gpu_device, hd, P):
    """Operands N(0, 3^2): a good share of the gates saturates.  Bound per output: 3 x the error of the same formulas in torch fp32
    on the CPU against fp64, floor 2 ulp of the tensor's max.  Two runs agree bit for bit."""
    from deep_visual_slam_amd import _lib
    t = gate_operands(P, hd, seed=100 * hd + P)
    got = run_gate_kernels(_lib.lib(), t, hd, gpu_device)
    again = run_gate_kernels(_lib.lib(), t, hd, gpu_device)
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), "%s differs between two runs" % k
    ref = gate_references(t, got, hd)
    for k, (r64, r32) in ref.items():
        assert torch.isfinite(got[k]).all(), k
        err, b = float((got[k].double() - r64).abs().max()), R.bound(r64, r32)
        print("hd %d P %d %s: max |err| %.3e, bound %.3e" % (hd, P, k, err, b))
        assert err <= b, (k, err, b)
    # the assembled matrices are copies of those outputs, every column written
    assert torch.equal(got["dpre"], torch.cat([got["dah"], got["dq"]], 1))
    assert torch.isfinite(got["dpre"]).all()


def test_saturated_gates_are_exact(gpu_device):
    """Every pre-activation is +100 or -100 (a_h = +-100, a_x = c = 0, a_q = +-100).  z, r, q, h' must be finite and EQUAL the fp64
    result rounded to fp32: 1, the subnormal sigmoid(-100) = 27 * 2^-149, and +-1 (an (e^2x - 1) / (e^2x + 1) tanh gives inf / inf).
    rh = r * h is the one output with two roundings in any fp32 evaluation: where r is that subnormal its 1.7 % rounding error
    reaches the product, so rh is held to the exactly rounded product of the (exact) fp32 r and h instead."""
    from deep_visual_slam_amd import _lib
    hd, P = 20, 103
    gen = torch.Generator().manual_seed(9)
    sign = lambda n: torch.where(torch.rand(P, n, generator=gen) < 0.5, -100.0, 100.0)
    t = gate_operands(P, hd, seed=10, sigma=1.0)
    t.update({"a_h": sign(2 * hd), "a_x": torch.zeros(P, 3 * hd), "c": torch.zeros(P, 3 * hd), "a_q": sign(hd)})
    got = run_gate_kernels(_lib.lib(), t, hd, gpu_device)
    c = {k: v.double() for k, v in t.items()}
    want = gate_formulas(c, hd)
    want.update(blend_formulas(c, want["z"], hd))
    for k in ("z", "r", "q", "h_new"):
        assert torch.isfinite(got[k]).all(), k
        assert torch.equal(got[k], want[k].float()), k
    assert set(got["q"].unique().tolist()) == {-1.0, 1.0}
    assert set(got["z"].unique().tolist()) == {27 * 2.0 ** -149, 1.0}
    assert torch.isfinite(got["rh"]).all()
    assert torch.equal(got["rh"], (got["r"].double() * c["h"]).float())
    for k in ("dq", "dh_a", "dh", "dpre", "dah"):
        assert torch.isfinite(got[k]).all(), k
    # the backward outputs that are exact there: 1 - q^2 = 0 everywhere, 1 - z = 0 where z = 1 (and exactly 1 beside the
    # subnormal z), 1 - r = 0 where r = 1
    one_z, one_r = got["z"] == 1, got["r"] == 1
    assert one_z.any() and (~one_z).any() and one_r.any() and (~one_r).any()
    assert torch.equal(got["dq"], torch.zeros(P, hd))
    assert torch.equal(got["dz"][one_z], torch.zeros(int(one_z.sum())))
    assert torch.equal(got["dr"][one_r], torch.zeros(int(one_r.sum())))
    assert torch.equal(got["dh_a"], torch.where(one_z, torch.zeros(()), t["g"]))
    assert torch.equal(got["dh"][one_r], (got["dh_a"].double() + c["d_rh"])[one_r].float())


def test_conv_gru_with_a_conv_q_that_returns_no_gradient(gpu_device):
    """raft_update.conv_gru is public and takes any conv_q.  One whose result does not depend on r * h hands no gradient to the
    gates node; the z and q columns that the blend node wrote must still reach a_h, a_x, c and h."""
    from deep_visual_slam_amd import raft_update
    hd, B, H, W = 20, 1, 3, 5
    gen = torch.Generator().manual_seed(4)
    shapes = {"a_h": 2 * hd, "a_x": 3 * hd, "c": 3 * hd, "h": hd, "a_q": hd, "g": hd}
    t = {k: torch.randn(B, n, H, W, generator=gen) for k, n in shapes.items()}
    names = ("a_h", "a_x", "c", "h")
    r64 = {k: v.double().requires_grad_(k in names) for k, v in t.items()}
    z = torch.sigmoid(r64["a_h"][:, :hd] + r64["a_x"][:, :hd] + r64["c"][:, :hd])
    q = torch.tanh(r64["a_q"] + r64["a_x"][:, 2 * hd:] + r64["c"][:, 2 * hd:])
    want = (1 - z) * r64["h"] + z * q
    want_g = torch.autograd.grad(want, [r64[k] for k in names], r64["g"])
    d = {k: v.to(gpu_device).contiguous(memory_format=CL).requires_grad_(k in names) for k, v in t.items()}
    got = raft_update.conv_gru(d["a_h"], d["a_x"], d["c"], d["h"], lambda rh: d["a_q"])
    got_g = torch.autograd.grad(got, [d[k] for k in names], d["g"])
    R.check_rel("h_new", got, want.detach())
    for k, a, b in zip(names, got_g, want_g):
        R.check_rel("d/" + k, a, b)


# ---- G2: the 7x7 convolution of the 4-channel padded flow, alone ------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 16, 17)], ids=["b2_5x7", "b1_16x17"])
def test_convf1_on_the_general_route(gpu_device, shape):
    """7x7, pad 3, Cin = 4 (Ktot = 196), ReLU: y, dx, dW, db against fp64 at the project's convolution tolerances.  The input and
    the filter are random in all four channels, which covers the zero-padded use."""
    from deep_visual_slam_amd import conv
    B, H, W = shape
    gen = torch.Generator().manual_seed(77)
    x, w, b = torch.randn(B, 4, H, W, generator=gen), torch.randn(64, 4, 7, 7, generator=gen) / 14.0, torch.randn(64, generator=gen) * 0.1
    dy = torch.randn(B, 64, H, W, generator=gen)
    r = [t.double().requires_grad_(True) for t in (x, w, b)]
    y64 = F.relu(F.conv2d(r[0], r[1], r[2], padding=3))
    g64 = torch.autograd.grad(y64, r, dy.double())
    d = [t.to(gpu_device).requires_grad_(True) for t in (x.contiguous(memory_format=CL), w.contiguous(memory_format=CL), b)]
    y = conv.conv2d(d[0], d[1], d[2], padding=3, act="relu")
    g = torch.autograd.grad(y, d, dy.to(gpu_device))
    R.check_rel("y", y, y64.detach())
    for name, got, want in zip(("d/x", "d/W", "d/b"), g, g64):
        R.check_rel(name, got, want)


# ---- G3 .. G6: the block -------------------------------------------------------------------------------------------------------
def make_block(hidden, planes, weights, dev):
    from deep_visual_slam_amd import raft_update
    levels, radius = {196: (4, 3), 36: (4, 1), 324: (4, 4)}[planes]
    block = raft_update.SmallUpdateBlock(hidden_dim=hidden, corr_levels=levels, corr_radius=radius)
    block.load_state_dict(weights)
    return block.to(dev)


def run_block(block, x, cot, dev, corr_cl=False):
    """raft_update_ref.run's dict from the GPU block."""
    for p in block.parameters():
        p.grad = None
    d = {k: v.to(dev).requires_grad_(True) for k, v in x.items()}
    corr = d["corr"].contiguous(memory_format=CL) if corr_cl else d["corr"]
    cot = [(a.to(dev), b.to(dev)) for a, b in cot]
    outs, loss = R.chain(lambda *a: block(*a)[::2], d["net"], d["inp"], corr, d["flow"], cot)
    names = list(R.INPUTS) + [k for k, _ in block.named_parameters()]
    grads = torch.autograd.grad(loss, [d[k] for k in R.INPUTS] + list(block.parameters()))
    torch.cuda.synchronize()
    res = {"d/" + n: g.detach().cpu() for n, g in zip(names, grads)}
    for k, (n, dl) in enumerate(outs):
        res["net%d" % k], res["delta%d" % k] = n.detach().cpu(), dl.detach().cpu()
    return res


STEP_CASES = [("h96_b2_5x7_nchw", 96, 196, 2, 5, 7, False), ("h96_b1_16x17_cl", 96, 196, 1, 16, 17, True),
              ("h20_b3_7x5_nchw", 20, 36, 3, 7, 5, False)]


@pytest.fixture(scope="module")
def step_refs():
    """name -> (weights, inputs, cotangents of 3 steps, fp64 one-step result): computed once, never modified."""
    out = {}
    for name, hd, planes, B, H, W, _ in STEP_CASES:
        weights = R.make_weights(hd, planes, seed=hd + H)
        x, cot = R.make_case(hd, planes, B, H, W, seed=3 * hd + W, steps=3)
        out[name] = (weights, x, cot, R.run(weights, x, cot[:1], torch.float64))
    return out


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_one_step(gpu_device, step_refs, case):
    """net, delta_flow and the gradients of the four inputs and of every parameter: 2e-5 of the tensor's max on outputs, 1e-4 on
    gradients."""
    name, hd, planes = case[:3]
    weights, x, cot, ref = step_refs[name]
    got = run_block(make_block(hd, planes, weights, gpu_device), x, cot[:1], gpu_device, corr_cl=case[6])
    assert sorted(got) == sorted(ref)
    for k in sorted(ref):
        R.check_rel(name + " " + k, got[k], ref[k])


def test_three_chained_steps(gpu_device, step_refs):
    """One inp, gradient through all three calls.  Bound per tensor: the larger of the one-step tolerance and 3 x the restatement's
    own fp32-vs-fp64 error on the same chain."""
    name, hd, planes = STEP_CASES[0][:3]
    weights, x, cot, _ = step_refs[name]
    ref = R.reference(weights, x, cot)
    block = make_block(hd, planes, weights, gpu_device)
    calls = []
    inner = block._context_conv
    block._context_conv = lambda *a: calls.append(1) or inner(*a)
    got = run_block(block, x, cot, gpu_device)
    assert len(calls) == 1                                          # one hoisted term serves the three calls, under autograd too
    r64, r32 = ref[torch.float64], ref[torch.float32]
    assert sorted(got) == sorted(r64)
    for k in sorted(r64):
        R.check_rel(name + " x3 " + k, got[k], r64[k], extra=3.0 * float((r32[k].double() - r64[k]).abs().max()))


def test_hoist_is_real_and_safe(gpu_device, step_refs):
    name, hd, planes = STEP_CASES[2][:3]
    weights, x, cot, _ = step_refs[name]
    from deep_visual_slam_amd import nn_ops
    block = make_block(hd, planes, weights, gpu_device)
    calls = []
    inner = block._context_conv
    block._context_conv = lambda *a: calls.append(1) or inner(*a)              # pass-through spy on the module's own helper
    d = {k: v.to(gpu_device) for k, v in x.items()}

    def agrees(what):
        with torch.no_grad():
            net, none, delta = block(d["net"], d["inp"], d["corr"], d["flow"])
        assert none is None
        w64 = {k: v.detach().double().cpu() for k, v in block.state_dict().items()}
        n64, d64 = R.update_block(w64, *(d[k].double().cpu() for k in R.INPUTS))
        R.check_rel(what + " net0", net, n64)
        R.check_rel(what + " delta0", delta, d64)

    for _ in range(3):
        agrees("same inp")
    assert len(calls) == 1
    d["inp"].mul_(2)                                                            # same object, new version
    agrees("inp.mul_(2)")
    assert len(calls) == 2
    with torch.no_grad():
        block.gru.convz.weight.mul_(0.5)
    agrees("convz.weight changed in place")
    assert len(calls) == 3
    version = block.gru.convr.bias._version
    block.gru.convr.bias.data.add_(0.25)                                        # a write behind torch's back, as dp.FusedAdam's:
    assert block.gru.convr.bias._version == version                             # no version counter moves, the writer announces it
    nn_ops.bump_generation()
    agrees("after bump_generation")
    assert len(calls) == 4
    agrees("unchanged")
    assert len(calls) == 4
    d["inp"] = d["inp"].clone()                                                 # equal values, another object
    agrees("fresh inp object")
    assert len(calls) == 5
    # under grad: forward -> backward -> forward with the same inp object; the gradient's arrival dropped the entry
    inp = d["inp"].requires_grad_(True)
    grads = []
    for _ in range(2):
        net, _, delta = block(d["net"], inp, d["corr"], d["flow"])
        loss = (net * cot[0][0].to(gpu_device)).sum() + (delta * cot[0][1].to(gpu_device)).sum()
        grads.append(torch.autograd.grad(loss, [inp] + list(block.parameters())))
    torch.cuda.synchronize()
    assert len(calls) == 7
    for k, (a, b) in enumerate(zip(*grads)):                                    # (weight gradients may be summed with atomics)
        R.check_rel("d/second pass %d" % k, b, a.double().cpu())


def test_fixture_through_the_gpu_block(gpu_device):
    """What the reference's own SmallUpdateBlock recorded (hidden 20, 36 planes, B=2, 5x7): one step at the one-step tolerances, the
    three-step chain at the chain's rule with the reference's recorded fp32 error.  Weight gradients stored as (sum, sum of |.|)
    are held to 1e-4 of the recorded sum of |.|, which the per-element tolerance implies a fortiori."""
    rec = load_golden(FIXTURE)
    hidden, levels, radius, B, H, W, seed = (int(v) for v in rec["meta/config"])
    planes = levels * (2 * radius + 1) ** 2
    weights = R.make_weights(hidden, planes, seed)
    for k, v in weights.items():
        assert np.array_equal(R.checksum(v), rec["w/cs/" + k]), "make_weights changed: " + k
    x = {k: torch.from_numpy(rec["in/" + k]) for k in R.INPUTS}
    cot = [(torch.from_numpy(rec["in/dnet%d" % k]), torch.from_numpy(rec["in/ddelta%d" % k])) for k in range(3)]
    block = make_block(hidden, planes, weights, gpu_device)
    for prefix, steps in (("s1/", 1), ("s3/", 3)):
        got = run_block(block, x, cot[:steps], gpu_device)
        seen = 0
        for key in sorted(rec):
            if not key.startswith(prefix) or key.startswith(prefix + "err/"):
                continue
            name = key[len(prefix):]
            if name.startswith("cs/"):
                have, want = R.checksum(got[name[3:]]), rec[key]
                err, b = float(np.abs(have - want).max()), R.GRAD_TOL * float(want[1])
                print("%s: |err| %.3e, bound %.3e" % (key, err, b))
                assert err <= b, (key, err, b)
            else:
                R.check_rel(key, got[name], torch.from_numpy(rec[key]))
            seen += 1
        assert seen == 2 * steps + 4 + len(weights)
