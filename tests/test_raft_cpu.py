"""CPU-side checks of SmallRAFT end to end: the restatement tests/raft_ref.py against the fixture that the reference's own SmallRAFT
produced (and against the reference's SmallEncoder where the reference tree is present), the module's state-dict keys, the argument
checks of the new dvs_inorm_* / dvs_upflow8_* entries (they fail before any launch), input errors, and the drop-in shims."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import raft_ref as R
from conftest import ROOT, load_golden

FIXTURE = "raft_small_b1_128x136.npz"
REFERENCE = "/root/reference/model"
DROPIN = os.path.join(ROOT, "deep-visual-slam_amd", "dropin")
NEW = ["dvs_inorm_slice_pixels", "dvs_inorm_workspace", "dvs_inorm_fwd", "dvs_inorm_bwd", "dvs_upflow8_fwd", "dvs_upflow8_bwd"]


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


def test_restatement_reproduces_the_reference_fixture(rec):
    """The fp32 restatement against the reference's recorded fp32 run: 3 x the recorded reference-fp32-vs-restatement-fp64 error,
    floor 2 ulp of the tensor's max (checksums: of the sum of |.|).  The same torch calls in the same order, so the agreement is
    far closer than the bound; no ReLU mask flips between the two."""
    B, H, W, iters, seed = (int(v) for v in rec["meta/config"])
    w = R.make_weights(seed)
    for k, v in w.items():
        assert np.allclose(R.checksum(v), rec["w/cs/" + k], rtol=1e-12, atol=0), "make_weights no longer draws the fixture's " + k
    im1, im2 = (torch.from_numpy(rec["in/image%d" % i]).float() / 255 for i in (1, 2))
    cot = [torch.from_numpy(rec["in/cot%d" % k]).float() for k in range(iters)]
    torch.set_num_threads(1)
    got = R.run_raft(w, im1, im2, cot, torch.float32, iters)
    for k in range(iters):
        for name in ("low%d" % k, "flow%d" % k):
            want = rec["ref32/" + name]
            b = max(3.0 * float(rec["err/" + name]), R.ulp_floor(float(np.abs(want).max())))
            err = float(np.abs(got[name].numpy().astype(np.float64) - want).max())
            print("%s: max |err| %.3e, bound %.3e" % (name, err, b))
            assert err <= b, (name, err, b)
    for key in (str(k) for k in rec["meta/keys"]):
        want = rec["ref32/cs/d/" + key]
        # both entries sum the same element errors; the signed sum's share of them is a matter of cancellation, so both entries are
        # held to the larger of the two recorded differences
        # recorded differences (one sample each, sometimes small by chance), or 1e-4 of the sum of |.|, the fixture rule of
        # test_raft_update_gpu.py
        b = max(3.0 * float(rec["err/cs/d/" + key].max()), R.GRAD_TOL * float(want[1]))
        err = np.abs(R.checksum(got["d/" + key]) - want)
        assert np.all(err <= b), (key, err, b)


def test_state_dict_is_the_reference_s(rec):
    from deep_visual_slam_amd import raft
    sd = raft.SmallRAFT().state_dict()
    assert list(sd) == [str(k) for k in rec["meta/keys"]]
    for k, shape in zip(rec["meta/keys"], rec["meta/shapes"]):
        assert tuple(sd[str(k)].shape) == tuple(int(s) for s in shape if s), k
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.state_keys()
    assert sum(v.numel() for v in sd.values()) == 990162
    raft.SmallRAFT().load_state_dict(R.make_weights(1), strict=True)
    assert not any("norm" in k for k in sd)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="reference tree not present")
@pytest.mark.parametrize("norm", ["instance", "none"])
def test_restatement_is_the_reference_encoder(norm):
    """2x3x40x56 through the reference's SmallEncoder in fp64 and fp32: the restatement's fp64 output within `bound`, its fp32 output
    within the same bound of the reference's fp32 output."""
    spec = importlib.util.spec_from_file_location("_reference_raft_extractor", os.path.join(REFERENCE, "raft", "core", "extractor.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)                                 # (it imports torch only; nothing lands in sys.modules)
    w = R.make_encoder_weights(128, 3)
    x = torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(4)) * 2 - 1
    ref = {}
    for dt in (torch.float64, torch.float32):
        enc = module.SmallEncoder(128, norm)
        enc.load_state_dict(w)
        with torch.no_grad():
            ref[dt] = enc.to(dt)([x[:1].to(dt), x[1:].to(dt)])
        ref[dt] = torch.cat(ref[dt], 0)
    b = R.bound(ref[torch.float64], ref[torch.float32])
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            got = R.small_encoder({k: v.to(dt) for k, v in w.items()}, x.to(dt), norm)
        err = float((got.double() - ref[dt].double()).abs().max())
        print("%s %s: max |err| %.3e, bound %.3e" % (norm, dt, err, b))
        assert err <= b, (norm, dt, err, b)


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
    assert l.dvs_inorm_slice_pixels() == 1024


def test_bad_arguments_fail_before_any_launch(built):
    l = built.lib()
    fake = 1 << 20                                                  # aligned, never dereferenced: every call fails on the host
    err = lambda: l.dvs_last_error()
    fwd = lambda y=fake, res=None, out=fake, tab=fake, ws=fake, nb=1 << 30, N=2, HW=100, C=24, norm=1, relu=1: \
        l.dvs_inorm_fwd(y, res, out, tab, ws, nb, N, HW, C, norm, relu, None)
    bwd = lambda dout=fake, y=fake, out=None, tab=fake, dy=fake, dres=None, ws=fake, nb=1 << 30, N=2, HW=100, C=24, norm=1: \
        l.dvs_inorm_bwd(dout, y, out, tab, dy, dres, ws, nb, N, HW, C, norm, 1, None)
    assert fwd(y=None) < 0 and b"null" in err()
    assert fwd(out=None) < 0 and b"null" in err()
    assert fwd(tab=None) < 0 and b"null" in err()
    assert fwd(ws=None) < 0 and b"null" in err()
    assert fwd(C=6) < 0 and b"multiple of 4" in err()
    assert fwd(C=0) < 0 and b"multiple of 4" in err()
    assert fwd(HW=1) < 0 and b"more than one spatial element" in err()
    assert fwd(HW=1 << 31) < 0 and b"2^31" in err()
    assert fwd(N=0) < 0 and b"N=0" in err()
    assert fwd(N=70000) < 0 and b"N=70000" in err()
    assert fwd(nb=16) < 0 and b"workspace" in err()
    assert fwd(y=fake + 4) < 0 and b"misaligned" in err()
    assert bwd(dout=None) < 0 and b"null" in err()
    assert bwd(dy=None) < 0 and b"null" in err()
    assert bwd(tab=None) < 0 and b"null" in err()
    assert bwd(out=fake) < 0 and b"go together" in err()
    assert bwd(dres=fake) < 0 and b"go together" in err()
    assert bwd(C=10) < 0 and b"multiple of 4" in err()
    assert bwd(HW=1) < 0 and b"more than one spatial element" in err()
    assert bwd(nb=16) < 0 and b"workspace" in err()
    assert l.dvs_inorm_workspace(2, 1, 24) == 0 and l.dvs_inorm_workspace(2, 100, 6) == 0
    assert l.dvs_inorm_workspace(3, 2049, 24) == 3 * 3 * 2 * 24 * 4
    for fn in (l.dvs_upflow8_fwd, l.dvs_upflow8_bwd):
        assert fn(None, fake, 1, 4, 4, 1, None) < 0 and b"null" in err()
        assert fn(fake, None, 1, 4, 4, 1, None) < 0 and b"null" in err()
        assert fn(fake, fake + 8, 1, 4, 4, 1, None) < 0 and b"misaligned" in err()
        assert fn(fake, fake, 0, 4, 4, 1, None) < 0 and b"N=0" in err()
        assert fn(fake, fake, 1, 0, 4, 1, None) < 0 and b"positive" in err()
        assert fn(fake, fake, 1, 4, 4, 2, None) < 0 and b"layout flag" in err()
        assert fn(fake, fake, 1, 8192, 8192, 1, None) < 0 and b"2^31" in err()


def test_input_errors(built):
    from deep_visual_slam_amd import raft, raft_encoder
    E = built.DvsError
    with pytest.raises(E, match="norm_fn='batch'"):
        raft_encoder.SmallEncoder(128, "batch")
    with pytest.raises(E, match="norm_fn='group'"):
        raft_encoder.SmallEncoder(128, "group")
    with pytest.raises(E, match="dropout"):
        raft_encoder.SmallEncoder(128, "instance", dropout=0.5)
    with pytest.raises(E, match="no CPU path"):
        raft_encoder.instance_norm_act(torch.zeros(1, 8, 4, 4))
    with pytest.raises(E, match="no CPU path"):
        raft_encoder.SmallEncoder()(torch.zeros(1, 3, 32, 32))
    with pytest.raises(E, match="no CPU path"):
        raft.upflow8(torch.zeros(1, 2, 4, 4))
    model = raft.SmallRAFT()
    with pytest.raises(E, match="no CPU path"):
        model(torch.zeros(1, 3, 128, 136), torch.zeros(1, 3, 128, 136))
    with pytest.raises(NotImplementedError):
        raft.RAFT(None)
    # shape and dtype errors are raised before any device work: `meta` tensors claim to be on no CPU and carry no data
    if torch.cuda.is_available():
        dev = torch.device("cuda:0")
        z = lambda *s, **kw: torch.zeros(*s, device=dev, **kw)
        model = model.to(dev)
        with pytest.raises(E, match="fp32 only"):
            model(z(1, 3, 128, 136, dtype=torch.float16), z(1, 3, 128, 136, dtype=torch.float16))
        with pytest.raises(E, match="multiples of 8"):
            model(z(1, 3, 132, 136), z(1, 3, 132, 136))
        with pytest.raises(E, match="at least 128x128"):
            model(z(1, 3, 120, 136), z(1, 3, 120, 136))
        with pytest.raises(E, match="more than one spatial element"):
            raft_encoder.instance_norm_act(z(2, 8, 1, 1))


def test_module_checks_shapes_without_a_device():
    """SmallRAFT._check on tensors that only claim to be on the GPU is not possible here; the size rules are plain Python and are
    exercised through it directly with a stand-in that has the attributes it reads."""
    from deep_visual_slam_amd import raft
    from deep_visual_slam_amd._lib import DvsError

    class Fake(torch.Tensor):
        is_cuda = True

    def fake(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype).as_subclass(Fake)
    model = raft.SmallRAFT()
    model._check(fake(1, 3, 128, 136), fake(1, 3, 128, 136), 12, None)
    with pytest.raises(DvsError, match="fp32 only"):
        model._check(fake(1, 3, 128, 136, dtype=torch.float16), fake(1, 3, 128, 136, dtype=torch.float16), 12, None)
    with pytest.raises(DvsError, match="multiples of 8"):
        model._check(fake(1, 3, 132, 136), fake(1, 3, 132, 136), 12, None)
    with pytest.raises(DvsError, match="at least 128x128"):
        model._check(fake(1, 3, 120, 136), fake(1, 3, 120, 136), 12, None)
    with pytest.raises(DvsError, match="flow_init"):
        model._check(fake(1, 3, 128, 136), fake(1, 3, 128, 136), 12, torch.zeros(1, 2, 16, 16))


SHIMS = """
import sys
from model.raft.core.raft import SmallRAFT, RAFT
from model.raft.core.extractor import SmallEncoder
from model.raft.core.raft import SmallUpdateBlock            # (model.raft.core.update itself stays the reference's: test_corr_cpu.py)
import deep_visual_slam_amd.raft as a, deep_visual_slam_amd.raft_encoder as b, deep_visual_slam_amd.raft_update as c
assert SmallRAFT is a.SmallRAFT and RAFT is a.RAFT and SmallEncoder is b.SmallEncoder and SmallUpdateBlock is c.SmallUpdateBlock
print("SHIMS-OK")
"""


def test_dropin_shims_resolve_to_this_package():
    env = dict(os.environ)
    env["PYTHONPATH"] = DROPIN
    r = subprocess.run([sys.executable, "-c", SHIMS], capture_output=True, text=True, env=env, cwd="/tmp", timeout=300)
    assert "SHIMS-OK" in r.stdout, r.stdout + r.stderr
