"""CPU-side checks of what the RAFT family's host layer shares (_raft_host): the cache of operands derived from parameters, on the
real encoders and update blocks (their derivations are plain torch ops and run on CPU parameters), and the one argument check, on
tensors that only claim to be on the GPU (the stand-in of test_raft_cpu.py).  No device, no library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _modules():
    from deep_visual_slam_amd import raft_encoder, raft_update
    return {"small_encoder": lambda: raft_encoder.SmallEncoder(8, "instance"),
            "basic_encoder": lambda: raft_encoder.BasicEncoder(8, "batch"),
            "small_update": lambda: raft_update.SmallUpdateBlock(8, 4, 1),
            "basic_update": lambda: raft_update.BasicUpdateBlock(128, 4, 1)}


def _derived_tensor(w):
    """One derived (non-leaf) tensor among the operands: an encoder's dict of (weight, bias) or an update block's slots."""
    if isinstance(w, dict):
        return next(iter(w.values()))[0]
    return w.m[0]


@pytest.mark.parametrize("kind", ["small_encoder", "basic_encoder", "small_update", "basic_update"])
def test_derived_operands_are_served_until_their_stamp_changes(kind):
    from deep_visual_slam_amd import nn_ops
    m = _modules()[kind]()
    assert m._weights is None and m._context is None
    w = m._derive()
    assert m._derive() is w and m._weights[1] is w                  # a second lookup serves the same object
    with torch.no_grad():
        next(m.parameters()).add_(0.0)                              # an in-place write: the parameter's _version moves
    w2 = m._derive()
    assert w2 is not w and m._derive() is w2
    nn_ops.bump_generation()                                        # a write behind torch's back (dp.FusedAdam)
    w3 = m._derive()
    assert w3 is not w2 and m._derive() is w3
    with torch.no_grad():                                           # the grad mode flips: no graph nodes in there
        w4 = m._derive()
        assert w4 is not w3 and m._derive() is w4
        assert not _derived_tensor(w4).requires_grad
    w5 = m._derive()
    assert w5 is not w4 and _derived_tensor(w5).requires_grad and not _derived_tensor(w5).is_leaf
    next(m.parameters()).requires_grad_(False)                      # requires_grad is part of the stamp
    assert m._derive() is not w5


@pytest.mark.parametrize("kind", ["small_encoder", "basic_encoder", "small_update", "basic_update"])
def test_a_delivered_gradient_drops_the_cache(kind):
    m = _modules()[kind]()
    w = m._derive()
    m._context = ("stands in for hoisted terms",)
    _derived_tensor(w).sum().backward()                             # frees the graph of the derived tensors
    assert m._weights is None and m._context is None
    assert m._derive() is not w


def test_leaf_operands_take_no_hook():
    """A bias that is the parameter itself has no graph to lose: its gradient must not drop the cache."""
    m = _modules()["small_encoder"]()
    w = m._derive()
    bias = w[m.conv2][1]
    assert bias is m.conv2.bias
    bias.sum().backward()
    assert m._weights is not None and m._derive() is w


def test_hoisted_terms_follow_inp_and_the_weights():
    block = _modules()["small_update"]()
    calls = []
    block._context_conv = lambda inp, wt, b: calls.append(1) or F.conv2d(inp, wt, b, padding=1)     # the CPU's convolution
    inp = torch.randn(1, 64, 3, 4)
    w = block._derive()
    c = block._hoisted(inp, w)
    assert block._hoisted(inp, w) is c and len(calls) == 1          # the same tensor object in the same state
    assert block._hoisted(inp.clone(), w) is not c and len(calls) == 2
    c = block._hoisted(inp, w)
    inp.add_(1.0)                                                   # the same object at another version
    assert block._hoisted(inp, w) is not c and len(calls) == 4
    c = block._hoisted(inp, w)
    assert len(calls) == 4 and block._context[2] is c
    with torch.no_grad():
        next(block.parameters()).add_(0.0)
    assert block._derive() is not w and block._context is None      # new weights drop the hoisted terms with them
    w = block._derive()
    c = block._hoisted(inp, w)
    c.sum().backward()                                              # a gradient through the hoisted term drops both slots
    assert block._weights is None and block._context is None


class Fake(torch.Tensor):
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(Fake)


def test_gpu_arg_refuses_and_names_the_caller():
    from deep_visual_slam_amd._lib import DvsError
    from deep_visual_slam_amd._raft_host import gpu_arg
    from deep_visual_slam_amd.raft_corr import NoCpuPath
    is_flow = lambda shape: shape[1] == 2 and min(shape) >= 1
    assert gpu_arg("caller: flow", fake(1, 2, 4, 4), "[N,2,h,w] expected", ok=is_flow) is None
    assert gpu_arg("caller", fake(3)) is None                       # no `want`: any rank
    assert gpu_arg("caller", fake(2, 5, 7), "[2,h,w] or [N,2,h,w] expected", rank=(3, 4)) is None
    for bad in (None, np.zeros((1, 2, 4, 4), np.float32)):
        with pytest.raises(DvsError, match=r"^caller: flow: GPU tensors only \(got .*\); this package has no CPU path$"):
            gpu_arg("caller: flow", bad, "[N,2,h,w] expected")
    with pytest.raises(NoCpuPath, match=r"^caller: GPU tensors only \(got cpu\); this package has no CPU path$") as e:
        gpu_arg("caller", torch.zeros(1, 2, 4, 4), no_cpu=NoCpuPath)
    assert isinstance(e.value, DvsError) and isinstance(e.value, NotImplementedError)
    with pytest.raises(DvsError, match="^caller: GPU tensors only") as e:
        gpu_arg("caller", torch.zeros(1, 2, 4, 4))
    assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(DvsError, match=r"^caller: fp32 only, got torch.float16$") as e:
        gpu_arg("caller", fake(1, 2, 4, 4, dtype=torch.float16), no_cpu=NoCpuPath)
    assert not isinstance(e.value, NoCpuPath)                       # the class is for the no-CPU case alone
    with pytest.raises(DvsError, match=r"^caller: fp32 only, got torch.float64 \(cast it\)$"):
        gpu_arg("caller", fake(1, 2, 4, 4, dtype=torch.float64), fp32_note=" (cast it)")
    with pytest.raises(DvsError, match=r"^caller: \[N,2,h,w\] expected, got \(2, 4, 4\)$"):
        gpu_arg("caller", fake(2, 4, 4), "[N,2,h,w] expected", ok=is_flow)     # the rank is judged before `ok` reads the shape
    with pytest.raises(DvsError, match=r"^caller: \[N,2,h,w\] expected, got \(1, 3, 4, 4\)$"):
        gpu_arg("caller", fake(1, 3, 4, 4), "[N,2,h,w] expected", ok=is_flow)
    with pytest.raises(DvsError, match=r"expected, got \(1, 1, 2, 5, 7\)$"):
        gpu_arg("caller", fake(1, 1, 2, 5, 7), "[2,h,w] or [N,2,h,w] expected", rank=(3, 4))
