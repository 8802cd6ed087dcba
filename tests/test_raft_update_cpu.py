"""CPU-side checks of SmallRAFT's update block: the restatement tests/raft_update_ref.py against the fixture that the
reference's own SmallUpdateBlock produced (and against that block itself where the reference tree is present), the argument checks
of the four dvs_gru_* entries (they fail before any launch), and the module's parameters and input errors."""
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import raft_update_ref as R
from conftest import ROOT, load_golden

NEW = ["dvs_gru_gates_fwd", "dvs_gru_blend_fwd", "dvs_gru_blend_bwd", "dvs_gru_gates_bwd"]
NPTR = {"dvs_gru_gates_fwd": 7, "dvs_gru_blend_fwd": 7, "dvs_gru_blend_bwd": 8, "dvs_gru_gates_bwd": 7}
FIXTURE = "raft_update_h20_p36_5x7.npz"
REFERENCE = "/root/reference/model"


def _fixture_case(rec):
    hidden, levels, radius, B, H, W, seed = (int(v) for v in rec["meta/config"])
    planes = levels * (2 * radius + 1) ** 2
    weights = R.make_weights(hidden, planes, seed)
    for k, v in weights.items():
        assert np.array_equal(R.checksum(v), rec["w/cs/" + k]), \
            "make_weights no longer draws the fixture's %s: the generator changed, not the block" % k
    x = {k: torch.from_numpy(rec["in/" + k]) for k in R.INPUTS}
    cot = [(torch.from_numpy(rec["in/dnet%d" % k]), torch.from_numpy(rec["in/ddelta%d" % k])) for k in range(3)]
    return weights, x, cot


def _compare(prefix, rec, got):
    """Every recorded tensor / checksum of one run against `got` (raft_update_ref.run's dict): 3 x the reference's own recorded
    fp32-vs-fp64 error of that tensor, floor 2 ulp (fp32) of its max."""
    seen = 0
    for key in sorted(rec):
        if not key.startswith(prefix) or key.startswith(prefix + "err/"):
            continue
        name = key[len(prefix):]
        want = np.asarray(rec[key])
        err_ref = np.asarray(rec[prefix + "err/" + name])
        have = R.checksum(got[name[3:]]) if name.startswith("cs/") else got[name].double().numpy()
        assert have.shape == want.shape, (key, have.shape, want.shape)
        b = np.maximum(3.0 * err_ref, R.ulp_floor(float(np.abs(want).max())))
        err = np.abs(have - want)
        print("%s: max |err| %.3e, bound %.3e" % (key, float(err.max()), float(np.max(b))))
        assert np.all(err <= b), (key, float(err.max()), float(np.max(b)))
        seen += 1
    return seen


def test_restatement_reproduces_the_reference_fixture():
    rec = load_golden(FIXTURE)
    weights, x, cot = _fixture_case(rec)
    n_params = len(weights)
    for prefix, steps in (("s1/", 1), ("s3/", 3)):
        got = R.run(weights, x, cot[:steps], torch.float64)
        assert _compare(prefix, rec, got) == 2 * steps + 4 + n_params


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="reference tree not present")
def test_restatement_is_the_reference_block_at_raft_small_size():
    """hidden_dim=96, 196 planes, B=1, 5x7: the reference's SmallUpdateBlock in fp64 and fp32 gives the truth and the bound."""
    spec = importlib.util.spec_from_file_location("_reference_raft_update", os.path.join(REFERENCE, "raft", "core", "update.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)                                 # (it imports torch only; nothing lands in sys.modules)
    SmallUpdateBlock = module.SmallUpdateBlock
    weights = R.make_weights(96, 196, 5)
    x, cot = R.make_case(96, 196, 1, 5, 7, 6, steps=3)
    res = {}
    for dt in (torch.float64, torch.float32):
        block = SmallUpdateBlock(SimpleNamespace(corr_levels=4, corr_radius=3), hidden_dim=96)
        block.load_state_dict(weights)
        block = block.to(dt)
        xs = {k: v.clone().to(dt).requires_grad_(True) for k, v in x.items()}
        outs, loss = R.chain(lambda *a: block(*a)[::2], xs["net"], xs["inp"], xs["corr"], xs["flow"], cot)
        loss.backward()
        r = {"d/" + k: v.grad for k, v in xs.items()}
        r.update({"d/" + k: p.grad for k, p in block.named_parameters()})
        for k, (n, d) in enumerate(outs):
            r["net%d" % k], r["delta%d" % k] = n.detach(), d.detach()
        res[dt] = r
    got = R.run(weights, x, cot, torch.float64)
    assert sorted(got) == sorted(res[torch.float64])
    for k, v in got.items():
        b = R.bound(res[torch.float64][k], res[torch.float32][k])
        err = float((v - res[torch.float64][k]).abs().max())
        assert err <= b, (k, err, b)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


def test_new_symbols_are_exported_and_declared(built):
    l = built.lib()
    src = open(os.path.join(ROOT, "include", "dvslam.h")).read()
    assert "update.py:23-31" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert hasattr(l, name), name
        assert name in built.exported_symbols(), name
        assert re.search(r"\b" + name + r"\s*\(", src), name


def test_bad_arguments_fail_before_any_launch(built):
    l = built.lib()
    fake = 1 << 20                                                  # aligned, never dereferenced: every call fails on the host
    for name in NEW:
        fn, n = getattr(l, name), NPTR[name]
        assert fn(*([None] * n), 16, 96, None) < 0 and b"null" in l.dvs_last_error(), name
        for k in range(n):                                          # any single null pointer
            args = [fake] * n
            args[k] = None
            assert fn(*args, 16, 96, None) < 0 and b"null" in l.dvs_last_error(), (name, k)
        assert fn(*([fake] * n), 16, 6, None) < 0 and b"multiple of 4" in l.dvs_last_error(), name
        assert fn(*([fake] * n), 16, 0, None) < 0 and b"hidden=0" in l.dvs_last_error(), name
        assert fn(*([fake] * n), 16, -4, None) < 0 and b"hidden=-4" in l.dvs_last_error(), name
        assert fn(*([fake] * n), 0, 96, None) < 0 and b"P=0" in l.dvs_last_error(), name
        assert fn(*([fake + 4] + [fake] * (n - 1)), 16, 96, None) < 0 and b"misaligned" in l.dvs_last_error(), name


def test_parameters_are_the_reference_s(built):
    from deep_visual_slam_amd import raft_update
    rec = load_golden(FIXTURE)
    block = raft_update.SmallUpdateBlock(hidden_dim=20, corr_levels=4, corr_radius=1)
    sd = block.state_dict()
    assert list(sd) == [str(k) for k in rec["meta/keys"]]
    for k, shape in zip(rec["meta/keys"], rec["meta/shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(s) for s in shape if s), k
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.state_keys(20, 36)
    block.load_state_dict(R.make_weights(20, 36, 1))                # strict: no key missing, none unexpected
    big = raft_update.SmallUpdateBlock()
    assert tuple(big.gru.convz.weight.shape) == (96, 242, 3, 3) and big.cor_planes == 196


def test_from_module_shares_the_parameters(built):
    from deep_visual_slam_amd import raft_update
    src = raft_update.SmallUpdateBlock(hidden_dim=20, corr_levels=4, corr_radius=1)
    duck = SimpleNamespace(encoder=src.encoder, gru=src.gru, flow_head=src.flow_head)      # anything of that shape
    block = raft_update.SmallUpdateBlock.from_module(duck)
    assert block.hidden_dim == 20 and block.cor_planes == 36
    theirs, mine = dict(src.named_parameters()), dict(block.named_parameters())
    assert list(theirs) == list(mine) and all(mine[k] is theirs[k] for k in theirs)
    with pytest.raises(built.DvsError, match="not a SmallUpdateBlock"):
        raft_update.SmallUpdateBlock.from_module(torch.nn.Linear(2, 2))
    src.flow_head.conv1 = torch.nn.Conv2d(20, 64, 3, padding=1)
    with pytest.raises(built.DvsError, match="flow_head.conv1"):
        raft_update.SmallUpdateBlock.from_module(src)


def test_input_errors(built):
    from deep_visual_slam_amd import raft_update
    with pytest.raises(built.DvsError, match="multiple of 4"):
        raft_update.SmallUpdateBlock(hidden_dim=96, corr_levels=2, corr_radius=1)       # 18 planes
    with pytest.raises(built.DvsError, match="hidden_dim=6"):
        raft_update.SmallUpdateBlock(hidden_dim=6)
    block = raft_update.SmallUpdateBlock(hidden_dim=20, corr_levels=4, corr_radius=1)
    x, _ = R.make_case(20, 36, 1, 5, 7, 0)
    with pytest.raises(built.DvsError, match="no CPU path"):
        block(x["net"], x["inp"], x["corr"], x["flow"])
