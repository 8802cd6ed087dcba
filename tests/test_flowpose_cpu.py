"""CPU-side checks of FlowPoseNet: the restatement tests/flowpose_ref.py against the fixture that the reference's own FlowPoseNet
produced, the module's state-dict keys, the constructor's checkpoint rules, the drop-in import, the argument checks of the
dvs_pool_fc_* entries (they fail before any launch) and the input errors."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import flowpose_ref as P
import raft_ref as R
from conftest import ROOT, load_golden

FIXTURE = "flowposenet_b2_128x136.npz"
DROPIN = os.path.join(ROOT, "deep-visual-slam_amd", "dropin")
NEW = ["dvs_pool_fc_slice_pixels", "dvs_pool_fc_workspace", "dvs_pool_fc_fwd", "dvs_pool_fc_bwd"]


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


# ---- reference agreement -----------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_fixture(rec):
    """The fp32 restatement against the reference's recorded fp32 run (B=2, 128x136, 12 iterations): the outputs within
    max(3 x the recorded reference-fp32-vs-restatement-fp64 difference, 2 ulp of the max), the gradient checksums by the rule of
    test_raft_cpu.py."""
    B, H, W, iters, seed = (int(v) for v in rec["meta/config"])
    w = P.make_weights(seed)
    for k, v in w.items():
        assert np.allclose(R.checksum(v), rec["w/cs/" + k], rtol=1e-12, atol=0), "make_weights no longer draws the fixture's " + k
    images = torch.from_numpy(rec["in/images"]).float() / 255
    cot = [torch.from_numpy(rec["in/cot_" + n]).float() for n in ("aa", "t")]
    torch.set_num_threads(1)
    got = P.run_net(w, images, cot, torch.float32, iters)
    for name in ("aa", "t"):
        want = rec["ref32/" + name]
        b = max(3.0 * float(rec["err/" + name]), R.ulp_floor(float(np.abs(want).max())))
        err = float(np.abs(got[name].numpy().astype(np.float64) - want).max())
        print("%s: max |err| %.3e, bound %.3e" % (name, err, b))
        assert err <= b, (name, err, b)
    for key in (str(k) for k in rec["meta/keys"]):
        want = rec["ref32/cs/d/" + key]
        # both entries sum the same element errors, so both are held to the larger of the two recorded differences, or 1e-4 of the
        # sum of |.|
        b = max(3.0 * float(rec["err/cs/d/" + key].max()), R.GRAD_TOL * float(want[1]))
        err = np.abs(R.checksum(got["d/" + key]) - want)
        assert np.all(err <= b), (key, err, b)


def test_state_dict_is_the_reference_s(rec):
    from deep_visual_slam_amd.posenet_single import FlowPoseNet
    model = FlowPoseNet(raft_checkpoint=None)
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in rec["meta/keys"]]
    for k, shape in zip(rec["meta/keys"], rec["meta/shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(s) for s in shape if s), k
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == P.state_keys()
    assert len(sd) == 114 and sum(1 for k in sd if k.startswith("flow_net.")) == 106
    assert sum(v.numel() for v in sd.values()) == sum(p.numel() for p in model.parameters()) == P.PARAMETERS == 1119224
    FlowPoseNet(raft_checkpoint=None).load_state_dict(P.make_weights(1), strict=True)
    for i in (0, 2, 4):
        assert model.pose_cnn[i].weight.is_contiguous(memory_format=torch.channels_last)
    assert model.pose_scale == 0.01 and model.supports_pairs and model.iters == 12 and not model.flow_net.alternate_corr
    assert FlowPoseNet(None, iters=5, alternate_corr=True).flow_net.alternate_corr


# ---- constructor and dropin --------------------------------------------------------------------------------------------------
def test_missing_checkpoint_is_a_file_not_found_a_dvs_and_a_not_implemented_error(tmp_path, monkeypatch):
    from deep_visual_slam_amd._lib import DvsError
    from deep_visual_slam_amd.posenet_single import FlowPoseNet, NoRaftCheckpoint
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NoRaftCheckpoint, match=re.escape("./raft-small.pth")) as e:
        FlowPoseNet()
    assert isinstance(e.value, FileNotFoundError) and isinstance(e.value, DvsError) and isinstance(e.value, NotImplementedError)
    with pytest.raises(FileNotFoundError, match="elsewhere.pth"):
        FlowPoseNet(os.path.join(str(tmp_path), "elsewhere.pth"))


@pytest.mark.parametrize("prefix", ["", "module."], ids=["plain", "module"])
def test_checkpoint_in_the_working_directory_is_loaded(tmp_path, monkeypatch, prefix):
    from deep_visual_slam_amd.posenet_single import FlowPoseNet
    monkeypatch.chdir(tmp_path)
    w = R.make_weights(5)
    torch.save({prefix + k: v for k, v in w.items()}, "raft-small.pth")
    model = FlowPoseNet()
    sd = model.flow_net.state_dict()
    assert list(sd) == list(w)
    for k, v in w.items():
        assert torch.equal(sd[k], v), k
    torch.save({prefix + k: v for k, v in list(w.items())[1:]}, "raft-small.pth")       # strict: a missing key is an error
    with pytest.raises(RuntimeError, match="Missing key"):
        FlowPoseNet()


SHIM = """
from model.posenet_single import FlowPoseNet, PoseNet, NoRaftCheckpoint
import deep_visual_slam_amd.posenet_single as a
assert FlowPoseNet is a.FlowPoseNet and PoseNet is a.PoseNet and NoRaftCheckpoint is a.NoRaftCheckpoint
try:
    FlowPoseNet()
except FileNotFoundError as e:
    assert "raft-small.pth" in str(e)
    print("SHIM-OK")
"""


def test_dropin_import_resolves_to_this_class(tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = DROPIN
    r = subprocess.run([sys.executable, "-c", SHIM], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert "SHIM-OK" in r.stdout, r.stdout + r.stderr


def test_trainable_parameters_keep_the_regression_layer():
    """dp.trainable_parameters filters module-relative names on ".fc." (torchvision's unused encoder.encoder.fc): FlowPoseNet's
    regression layer is "fc.weight" / "fc.bias", without a leading dot, so it stays in the arena and trains."""
    from deep_visual_slam_amd import dp
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.posenet_single import FlowPoseNet
    names = [n for n, _ in dp.trainable_parameters(DepthNet(18, False), FlowPoseNet(None))]
    assert "1.fc.weight" in names and "1.fc.bias" in names and not any("encoder.fc." in n for n in names)
    assert sum(1 for n in names if n.startswith("1.")) == 114


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
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
    assert built.ABI_VERSION == 12 and l.dvs_abi_version() == 12
    T = l.dvs_pool_fc_slice_pixels()
    assert T >= 64 and T % 64 == 0
    assert l.dvs_pool_fc_workspace(3, 2 * T + 5, 24) == 3 * 3 * 24 * 4
    assert l.dvs_pool_fc_workspace(1, 1, 4) == 16
    for bad in ((0, 10, 8), (70000, 10, 8), (2, 0, 8), (2, -3, 8), (2, 10, 6), (2, 10, 0), (2, 10, 1028)):
        assert l.dvs_pool_fc_workspace(*bad) == 0, bad


def test_bad_arguments_fail_before_any_launch(built):
    l = built.lib()
    fake = 1 << 20                                                  # aligned, never dereferenced: every call fails on the host
    err = lambda: l.dvs_last_error()
    fwd = lambda y=fake, W=fake, b=fake, out=fake, mean=fake, ws=fake, nb=1 << 30, N=2, P=100, C=24, J=6: \
        l.dvs_pool_fc_fwd(y, W, b, out, mean, ws, nb, N, P, C, J, 1, 0.01, None)
    bwd = lambda dout=fake, y=fake, mean=fake, W=fake, dy=fake, dW=fake, db=fake, N=2, P=100, C=24, J=6: \
        l.dvs_pool_fc_bwd(dout, y, mean, W, dy, dW, db, N, P, C, J, 1, 0.01, None)
    for name in ("y", "W", "out", "mean", "ws"):
        assert fwd(**{name: None}) < 0 and b"null" in err(), name
        assert fwd(**{name: fake + 4}) < 0 and b"misaligned" in err(), name
    assert fwd(b=fake + 8) < 0 and b"misaligned" in err()
    for name in ("dout", "y", "mean", "W", "dy", "dW"):
        assert bwd(**{name: None}) < 0 and b"null" in err(), name
        assert bwd(**{name: fake + 4}) < 0 and b"misaligned" in err(), name
    assert bwd(db=fake + 8) < 0 and b"misaligned" in err()
    for call in (fwd, bwd):
        assert call(C=6) < 0 and b"multiple of 4" in err()
        assert call(C=0) < 0 and b"multiple of 4" in err()
        assert call(C=1028) < 0 and b"multiple of 4" in err()
        assert call(J=0) < 0 and b"J=0" in err()
        assert call(J=17) < 0 and b"J=17" in err()
        assert call(N=0) < 0 and b"N=0" in err()
        assert call(N=70000) < 0 and b"N=70000" in err()
        assert call(P=0) < 0 and b"P=0" in err()
        assert call(P=-1) < 0 and b"P=-1" in err()
        assert call(P=1 << 31) < 0 and b"2^31" in err()
    assert fwd(nb=16) < 0 and b"workspace" in err()
    assert fwd(nb=2 * 24 * 4 - 1) < 0 and b"workspace" in err()


# ---- input errors ----------------------------------------------------------------------------------------------------------------
def test_cpu_input_is_refused(built):
    from deep_visual_slam_amd import posenet_single
    model = posenet_single.FlowPoseNet(None)
    with pytest.raises(built.DvsError, match="no CPU path"):
        model(torch.zeros(1, 6, 128, 136))
    with pytest.raises(built.DvsError, match="no CPU path"):
        posenet_single.pool_fc(torch.zeros(1, 8, 4, 4), torch.zeros(6, 8))


def test_module_checks_shapes_without_a_device():
    """The shape and dtype rules are plain Python and are exercised with a stand-in tensor that only claims to be on the GPU;
    SmallRAFT's own size rules are reached through the same stand-in."""
    from deep_visual_slam_amd._lib import DvsError
    from deep_visual_slam_amd.posenet_single import FlowPoseNet

    class Fake(torch.Tensor):
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Fake)
    model = FlowPoseNet(None)
    model._check(fake(2, 6, 128, 136))
    with pytest.raises(DvsError, match="fp32 only"):
        model(fake(2, 6, 128, 136, dtype=torch.float16))
    with pytest.raises(DvsError, match=r"\[B,6,H,W\] expected"):
        model(fake(2, 3, 128, 136))
    with pytest.raises(DvsError, match=r"\[B,6,H,W\] expected"):
        model(fake(6, 128, 136))
    with pytest.raises(DvsError, match="multiples of 8"):
        model(fake(1, 6, 132, 136))
    with pytest.raises(DvsError, match="at least 128x128"):
        model(fake(1, 6, 120, 136))
