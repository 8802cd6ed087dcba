"""CPU-side checks of the full-size RAFT: the restatement tests/raft_basic_ref.py against the fixture that the reference's own RAFT
produced, the module's state-dict keys and strict loading, the split shift-stacked SepConvGRU against the concatenated one in
fp64, the argument checks of the new dvs_convex_up_* / dvs_shift_stack_* entries (they fail before any launch), every input error,
and the drop-in shims."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import raft_basic_ref as R
from conftest import ROOT, load_golden

FIXTURE = "raft_basic_b2_128x136.npz"
DROPIN = os.path.join(ROOT, "deep-visual-slam_amd", "dropin")
NEW = ["dvs_convex_up_workspace", "dvs_convex_up_fwd", "dvs_convex_up_bwd", "dvs_shift_stack_fwd", "dvs_shift_stack_bwd"]
PARAMETERS = 5257536        # of the reference's RAFT(small=False)


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_restatement_reproduces_the_reference_fixture(rec, mode):
    """The fp32 restatement against the reference's recorded fp32 run, in both BatchNorm modes: 3 x the recorded
    reference-fp32-vs-restatement-fp64 error, floor 2 ulp of the tensor's max; gradient checksums within the larger of 3 x the
    recorded difference and GRAD_TOL of the sum of |.| (tests/test_raft_cpu.py's rule); in train mode the BatchNorm buffers the
    forward leaves behind, against the reference's."""
    B, H, W, iters, seed = (int(v) for v in rec["meta/config"])
    w = R.make_weights(seed)
    for k, v in w.items():
        assert np.allclose(R.checksum(v), rec["w/cs/" + k], rtol=1e-12, atol=0), "make_weights no longer draws the fixture's " + k
    im1, im2 = (torch.from_numpy(rec["in/image%d" % i]).float() / 255 for i in (1, 2))
    cot = [torch.from_numpy(rec["in/cot%d" % k]).float() for k in range(iters)]
    torch.set_num_threads(1)
    got = R.run_raft(w, im1, im2, cot, torch.float32, iters, None, mode == "train")
    for k in range(iters):
        for name in ("low%d" % k, "flow%d" % k):
            want = rec["ref32/%s/%s" % (mode, name)]
            b = max(3.0 * float(rec["err/%s/%s" % (mode, name)]), R.ulp_floor(float(np.abs(want).max())))
            err = float(np.abs(got[name].numpy().astype(np.float64) - want).max())
            print("%s %s: max |err| %.3e, bound %.3e" % (mode, name, err, b))
            assert err <= b, (name, err, b)
    seen = 0
    for key in (k[2:] for k in got if k.startswith("d/")):
        want = rec["ref32/%s/cs/d/%s" % (mode, key)]
        b = max(3.0 * float(rec["err/%s/cs/d/%s" % (mode, key)].max()), R.GRAD_TOL * float(want[1]))
        err = np.abs(R.checksum(got["d/" + key]) - want)
        assert np.all(err <= b), (key, err, b)
        seen += 1
    assert seen == len([k for k in R.parameter_keys(w) if ".downsample.1." not in k])
    if mode == "train":
        stats = [k for k in got if k.startswith("stats/")]
        assert len(stats) == 3 * 15                                  # 15 BatchNorms (norm3 is not counted again as downsample.1)
        for k in stats:
            want = rec["ref32/train/" + k]
            if k.endswith("num_batches_tracked"):
                assert int(got[k]) == int(want) == 4
                continue
            b = max(3.0 * float(rec["err/train/stats"]), R.ulp_floor(float(np.abs(want).max())))
            assert float(np.abs(got[k].numpy().astype(np.float64) - want).max()) <= b, k


def test_state_dict_is_the_reference_s(rec):
    """Keys, order, shapes and parameter count; a reference-shaped state dict loads with strict=True and arrives."""
    from deep_visual_slam_amd import raft
    model = raft.RAFT({"small": False})
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in rec["meta/keys"]]
    for k, shape in zip(rec["meta/keys"], rec["meta/shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(s) for s in shape if s), k
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.state_keys()
    assert sum(p.numel() for p in model.parameters()) == PARAMETERS
    w = R.make_weights(1)
    model.load_state_dict(w, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, w[k]), k
    # norm3 is downsample.1: one module, one parameter, two names (extractor.py:44-45)
    blk = model.cnet.layer2[0]
    assert blk.downsample[1] is blk.norm3
    assert not any("norm" in k for k in sd if k.startswith("fnet."))
    assert model.hidden_dim == model.context_dim == 128 and model.corr_radius == 4 and model.corr_levels == 4


def test_args_forms_and_module_tree():
    from types import SimpleNamespace

    from deep_visual_slam_amd import raft, raft_corr, raft_encoder, raft_update
    for args in ({"small": False}, SimpleNamespace(small=False, alternate_corr=True), {}):
        m = raft.RAFT(args)
        assert isinstance(m.fnet, raft_encoder.BasicEncoder) and m.fnet.norm_fn == "instance"
        assert isinstance(m.cnet, raft_encoder.BasicEncoder) and m.cnet.norm_fn == "batch"
        assert isinstance(m.update_block, raft_update.BasicUpdateBlock)
    assert m.alternate_corr is False and raft.RAFT(SimpleNamespace(alternate_corr=True)).alternate_corr is True
    assert raft_corr.AlternateCorrBlock is raft.AlternateCorrBlock
    m.train()
    m.freeze_bn()
    bns = [x for x in m.modules() if isinstance(x, torch.nn.BatchNorm2d)]
    assert len(bns) == 15 and not any(b.training for b in bns) and m.training and m.cnet.training


def test_from_module_shares_the_parameters():
    from deep_visual_slam_amd import raft_update
    from deep_visual_slam_amd._lib import DvsError
    a = raft_update.BasicUpdateBlock()
    b = raft_update.BasicUpdateBlock.from_module(a)
    assert [k for k, _ in b.named_parameters()] == [k for k, _ in a.named_parameters()] == [k for k, _ in R.update_keys()]
    assert all(p is q for p, q in zip(a.parameters(), b.parameters()))
    with pytest.raises(DvsError, match="not a BasicUpdateBlock"):
        raft_update.BasicUpdateBlock.from_module(raft_update.SmallUpdateBlock())
    with pytest.raises(DvsError, match="hidden_dim=96"):
        raft_update.BasicUpdateBlock(hidden_dim=96)


# ---- the algebra the implementation rests on --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 1, 2), (1, 2, 1)], ids=["b2_5x7", "b1_1x2", "b1_2x1"])
def test_split_shift_stacked_gru_is_the_concatenated_one(shape):
    """fp64, both passes: the filters cut by input block, every contraction a 1x1 convolution over the shift-stack, against
    F.conv2d with the full (1,5) / (5,1) filters over the concatenation.  1e-13 relative (DESIGN.md section 17 measured 4e-16 for
    the small block); extents 1 and 2 put most of the window outside the map."""
    B, H, W = shape
    w = {k: v.double() for k, v in R.make_update_weights(3).items()}
    x, _ = R.make_update_case(B, H, W, 1)
    x = {k: v.double() for k, v in x.items()}
    motion = R.motion_encoder(w, x["flow"], x["corr"])
    a = R.sep_conv_gru(w, x["net"], torch.cat([x["inp"], motion], 1))
    b = R.sep_conv_gru_split(w, x["net"], x["inp"], motion)
    err = float((a - b).abs().max() / a.abs().max())
    print("relative difference %.3e" % err)
    assert err <= 1e-13


@pytest.mark.parametrize("axis", [0, 1])
def test_module_s_stacked_filter_is_the_restatement_s(axis):
    """raft_update.stacked_filter / split_gru_filters (differentiable re-layouts, no kernel) against the restatement, and a
    (1,5) / (5,1) convolution against the 1x1 convolution over the shift-stack; gradients land on the original filter."""
    from deep_visual_slam_amd import raft_update
    gen = torch.Generator().manual_seed(5 + axis)
    wt = torch.randn(8, 12, *((1, 5) if axis == 0 else (5, 1)), generator=gen, dtype=torch.float64).requires_grad_(True)
    x = torch.randn(2, 12, 4, 3, generator=gen, dtype=torch.float64)
    assert torch.equal(raft_update.stacked_filter(wt), R.stacked_filter(wt))
    want = F.conv2d(x, wt, padding=(0, 2) if axis == 0 else (2, 0))
    got = F.conv2d(R.shift_stack(x, axis), raft_update.stacked_filter(wt))
    assert float((got - want).detach().abs().max()) <= 1e-13 * float(want.detach().abs().max())
    cot = torch.randn(want.shape, generator=gen, dtype=torch.float64)
    g_want, = torch.autograd.grad(want, wt, cot)
    g_got, = torch.autograd.grad(got, wt, cot)
    assert float((g_got - g_want).abs().max()) <= 1e-13 * float(g_want.abs().max())


def test_upsample_restatement_is_the_reference_s_formula():
    """raft_basic_ref.upsample_flow (a gather of nine shifted copies) against raft.py:170-181 written with F.unfold, fp64."""
    flow, mask, _ = R.convex_case(2, 5, 7, 3)
    flow, mask = flow.double(), mask.double()
    N, _, h, w = flow.shape
    m = torch.softmax(mask.view(N, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(N, 2, 9, 1, 1, h, w)
    want = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * h, 8 * w)
    got = R.upsample_flow(flow, mask)
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    assert float((R.upsample_flow(flow, 4 * mask, 0.25) - want).abs().max()) <= 1e-14 * float(want.abs().max())


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


def test_new_symbols_are_exported_and_declared(built):
    l = built.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvslam.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(l, name) and name in built.exported_symbols(), name
        assert re.search(r"\b" + name + r"\s*\(", src), name
    assert built.ABI_VERSION == 12 and l.dvs_abi_version() == 12            # additive: the version stays


def test_bad_arguments_fail_before_any_launch(built):
    l = built.lib()
    fake = 1 << 20                                                  # aligned, never dereferenced: every call fails on the host
    err = lambda: l.dvs_last_error()
    fwd = lambda flow=fake, mask=fake, out=fake, N=2, h=4, w=5, s=0.25: l.dvs_convex_up_fwd(flow, mask, out, N, h, w, s, None)
    bwd = lambda dout=fake, flow=fake, mask=fake, dflow=fake, dmask=fake, ws=fake, nb=1 << 30, N=2, h=4, w=5, s=0.25: \
        l.dvs_convex_up_bwd(dout, flow, mask, dflow, dmask, ws, nb, N, h, w, s, None)
    for name in ("flow", "mask", "out"):
        assert fwd(**{name: None}) < 0 and b"dvs_convex_up_fwd: null" in err()
        assert fwd(**{name: fake + 4}) < 0 and b"misaligned" in err()
    for name in ("dout", "flow", "mask", "dflow", "dmask", "ws"):
        if name in ("dout", "flow", "mask", "ws"):                  # dflow or dmask alone may be NULL: that gradient is skipped
            assert bwd(**{name: None}) < 0 and b"dvs_convex_up_bwd: null" in err()
        assert bwd(**{name: fake + 8}) < 0 and b"misaligned" in err()
    assert bwd(dflow=None, dmask=None) < 0 and b"both NULL" in err()
    assert bwd(dmask=None, ws=None) < 0 and b"dflow needs the workspace" in err()
    assert bwd(dflow=None, ws=None, N=0) < 0 and b"N=0" in err()    # without dflow no workspace is asked for
    for call in (fwd, bwd):
        assert call(N=0) < 0 and b"N=0" in err()
        assert call(N=70000) < 0 and b"N=70000" in err()
        assert call(h=0) < 0 and b"positive" in err()
        assert call(w=-1) < 0 and b"positive" in err()
        assert call(h=8192, w=8192) < 0 and b"2^31" in err()
        assert call(s=float("nan")) < 0 and b"finite" in err()
        assert call(s=float("inf")) < 0 and b"finite" in err()
    assert bwd(nb=2 * 4 * 5 * 18 * 4 - 1) < 0 and b"workspace" in err()
    assert l.dvs_convex_up_workspace(2, 4, 5) == 2 * 4 * 5 * 18 * 4
    assert l.dvs_convex_up_workspace(0, 4, 5) == 0 and l.dvs_convex_up_workspace(1, 8192, 8192) == 0
    for fn, who in ((l.dvs_shift_stack_fwd, b"dvs_shift_stack_fwd"), (l.dvs_shift_stack_bwd, b"dvs_shift_stack_bwd")):
        call = lambda a=fake, b=fake, N=2, H=3, W=4, C=8, axis=0: fn(a, b, N, H, W, C, axis, None)
        assert call(a=None) < 0 and who + b": null" in err()
        assert call(b=None) < 0 and who + b": null" in err()
        assert call(a=fake + 4) < 0 and b"misaligned" in err()
        assert call(b=fake + 8) < 0 and b"misaligned" in err()
        assert call(N=0) < 0 and b"positive" in err()
        assert call(H=0) < 0 and b"positive" in err()
        assert call(W=-3) < 0 and b"positive" in err()
        assert call(C=0) < 0 and b"multiple of 4" in err()
        assert call(C=6) < 0 and b"multiple of 4" in err()
        assert call(axis=2) < 0 and b"axis=2" in err()
        assert call(axis=-1) < 0 and b"axis=-1" in err()


# ---- input errors -----------------------------------------------------------------------------------------------------------------
def test_input_errors(built):
    from deep_visual_slam_amd import raft, raft_encoder, raft_update
    E = built.DvsError
    with pytest.raises(E, match="norm_fn='group'"):
        raft_encoder.BasicEncoder(128, "group")
    with pytest.raises(E, match="dropout"):
        raft_encoder.BasicEncoder(128, "batch", dropout=0.5)
    with pytest.raises(E, match="output_dim"):
        raft_encoder.BasicEncoder(126, "batch")
    with pytest.raises(E, match="norm_fn='batch'"):
        raft_encoder.SmallEncoder(128, "batch")                     # the small encoder keeps its own rule
    for norm in ("instance", "batch", "none"):
        with pytest.raises(E, match="no CPU path"):
            raft_encoder.BasicEncoder(128, norm)(torch.zeros(1, 3, 32, 32))
    with pytest.raises(E, match="two image batches"):
        raft_encoder.BasicEncoder(128, "none")([torch.zeros(1, 3, 32, 32)] * 3)
    with pytest.raises(E, match="upsample_flow: flow: GPU tensors only.*no CPU path"):
        raft.upsample_flow(torch.zeros(1, 2, 4, 4), torch.zeros(1, 576, 4, 4))
    with pytest.raises(E, match="shift_stack: GPU tensors only.*no CPU path"):
        raft_update.shift_stack(torch.zeros(1, 8, 4, 4), 0)
    with pytest.raises(E, match="a \\(1,5\\) or \\(5,1\\) filter"):
        raft_update.stacked_filter(torch.zeros(4, 4, 3, 3))
    block = raft_update.BasicUpdateBlock()
    with pytest.raises(E, match="BasicUpdateBlock: net: GPU tensors only.*no CPU path"):
        block(torch.zeros(1, 128, 4, 4), torch.zeros(1, 128, 4, 4), torch.zeros(1, 324, 4, 4), torch.zeros(1, 2, 4, 4))
    with pytest.raises(E, match="small=True.*SmallRAFT"):
        raft.RAFT({"small": True})
    with pytest.raises(E, match="mixed_precision"):
        raft.RAFT({"small": False, "mixed_precision": True})
    with pytest.raises(E, match="dropout"):
        raft.RAFT({"small": False, "dropout": 0.1})
    with pytest.raises(E, match="args are required") as info:
        raft.RAFT(None)
    assert isinstance(info.value, NotImplementedError) and isinstance(info.value, E)
    model = raft.RAFT({"small": False})
    with pytest.raises(E, match="RAFT: image1: GPU tensors only.*no CPU path"):
        model(torch.zeros(1, 3, 128, 136), torch.zeros(1, 3, 128, 136))


def test_module_checks_shapes_without_a_device():
    """RAFT._check is SmallRAFT's (one function): the size rules through a stand-in that has the attributes it reads."""
    from deep_visual_slam_amd import raft
    from deep_visual_slam_amd._lib import DvsError

    class Fake(torch.Tensor):
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Fake)
    model = raft.RAFT({})
    assert type(model)._check is raft.SmallRAFT._check
    model._check(fake(1, 3, 128, 136), fake(1, 3, 128, 136), 12, None)
    with pytest.raises(DvsError, match="RAFT: image1: fp32 only"):
        model._check(fake(1, 3, 128, 136, dtype=torch.float16), fake(1, 3, 128, 136, dtype=torch.float16), 12, None)
    with pytest.raises(DvsError, match="multiples of 8"):
        model._check(fake(1, 3, 132, 136), fake(1, 3, 132, 136), 12, None)
    with pytest.raises(DvsError, match="at least 128x128"):
        model._check(fake(1, 3, 120, 136), fake(1, 3, 120, 136), 12, None)
    with pytest.raises(DvsError, match="iters=0"):
        model._check(fake(1, 3, 128, 136), fake(1, 3, 128, 136), 0, None)
    with pytest.raises(DvsError, match="flow_init"):
        model._check(fake(1, 3, 128, 136), fake(1, 3, 128, 136), 12, torch.zeros(1, 2, 16, 16))


SHIMS = """
import sys
from model.raft.core.raft import RAFT, BasicUpdateBlock, upsample_flow
from model.raft.core.extractor import BasicEncoder, SmallEncoder
import deep_visual_slam_amd.raft as a, deep_visual_slam_amd.raft_encoder as b, deep_visual_slam_amd.raft_update as c
assert RAFT is a.RAFT and BasicEncoder is b.BasicEncoder and SmallEncoder is b.SmallEncoder and BasicUpdateBlock is c.BasicUpdateBlock
assert upsample_flow is a.upsample_flow
model = RAFT({'small': False})
assert type(model.fnet) is BasicEncoder and type(model.update_block) is BasicUpdateBlock
print("SHIMS-OK")
"""


def test_dropin_shims_resolve_to_this_package():
    env = dict(os.environ)
    env["PYTHONPATH"] = DROPIN
    r = subprocess.run([sys.executable, "-c", SHIMS], capture_output=True, text=True, env=env, cwd="/tmp", timeout=300)
    assert "SHIMS-OK" in r.stdout, r.stdout + r.stderr
