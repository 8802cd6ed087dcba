"""The rigid mode of the RAFT frame stream on the GPU (raft_video.RigidFlowStream, csrc/rigidflow.hip inside the stream): every pair
also carries the rigid flow of the previous frame's depth and the camera motion, and the moving-object labels of flow_up against it.

130x141 frames (padded 136x144), iters = 2, the seeded weights and images of raft_ref / raft_basic_ref: the models, frames and
helpers are those of tests/test_raftstream_gpu.py.  Depth and pose are synthetic (rigidflow_ref.scene: depths in 0.1 .. 10, a pinhole
K, small poses), a different one for every pair.  What the stream computes is compared bit for bit with rigid_flow called by hand on
the stream's own flow_up and valid.  Measured on the MI355X: see DESIGN.md section 24."""
import numpy as np
import pytest
import torch

import rigidflow_ref as R
from test_raftstream_gpu import H0, ITERS, W0, bits, make_model, u8_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import raft_video
    return raft_video


@pytest.fixture
def deterministic():
    """dvs_set_deterministic(1) for one test: the mode in which a forward repeats exactly (tests/test_raftstream_gpu.py says why
    the bit-for-bit comparisons between two streams are made in it)."""
    from deep_visual_slam_amd import _lib
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


def geometry(dev, B, pairs=3):
    """[dict(depth [B,1,H0,W0], T [B,4,4], K [4,4], inv_K [4,4])] on the device, one per pair, all different."""
    out = []
    for i in range(pairs):
        s = R.scene(H0, W0, N=B, seed=40 + i)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        out.append(dict(depth=t(s.depth), T=t(s.T), K=t(s.K), inv_K=t(s.iK)))
    return out


def raw(t):
    return t if t.dtype == torch.uint8 else bits(t)


FIELDS = ("flow_low", "flow_up", "image", "flow_low_bw", "flow_up_bw", "valid", "valid_bw", "rigid", "motion")


def run_stream(stream, frames, geo):
    """Clones of every field of every pair (None where the stream has none): a graph's outputs are valid until the next push only."""
    out = []
    for i, x in enumerate(frames):
        r = stream.push(x, **(geo[i - 1] if i and geo is not None else {}))
        if i == 0:
            assert r is None
        else:
            out.append([None if getattr(r, name) is None else getattr(r, name).clone() for name in FIELDS])
    return out


def differing(a, g):
    return [name for name, x, y in zip(FIELDS, a, g) if (x is None) != (y is None) or (x is not None and not torch.equal(raw(x), raw(y)))]


# ---- the eager stream -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidirectional", [False, True], ids=["forward", "bidirectional"])
@pytest.mark.parametrize("kind,B", [("small", 1), ("basic", 2)])
def test_eager_rigid_stream_over_four_frames(gpu_device, V, kind, B, bidirectional):
    """rigid and motion of every pair are rigid_flow(depth, T, K, inv_K, flow=r.flow_up, valid=r.valid) called by hand, bit for
    bit; the kernel read the un-padded view of the padded flow."""
    model = make_model(kind, gpu_device)
    frames = [x.to(gpu_device) for x in u8_frames(B)]
    geo = geometry(gpu_device, B)
    stream = V.RigidFlowStream(model, iters=ITERS, graph=False, bidirectional=bidirectional, rigid_alpha=0.02, rigid_beta=0.75)
    assert stream.push(frames[0]) is None
    seen = []
    for cur, g in zip(frames[1:], geo):
        r = stream.push(cur, **g)
        assert tuple(r.rigid.shape) == (B, 2, H0, W0) and r.rigid.dtype == torch.float32
        assert tuple(r.motion.shape) == (B, H0, W0) and r.motion.dtype == torch.uint8
        assert (r.valid is not None) == bidirectional and not r.flow_up.is_contiguous()
        rigid, motion = V.rigid_flow(g["depth"], g["T"], g["K"], g["inv_K"], flow=r.flow_up, valid=r.valid, alpha=0.02, beta=0.75)
        assert torch.equal(bits(r.rigid), bits(rigid)) and torch.equal(r.motion, motion)
        want = R.rigid(g["depth"].cpu().numpy(), g["T"].cpu().numpy(), g["K"].cpu().numpy(), g["inv_K"].cpu().numpy(),
                       r.flow_up.cpu().numpy(), None if r.valid is None else r.valid.cpu().numpy(), 0.02, 0.75)
        assert np.array_equal(r.motion.cpu().numpy(), want.label) and np.array_equal(R.bits(r.rigid.cpu().numpy()), R.bits(want.rigid))
        if bidirectional:
            assert not r.motion[r.valid == 0].any()                             # an occluded pixel is not judged
        seen.append(r.rigid.clone())
    assert not torch.equal(bits(seen[0]), bits(seen[1]))                        # each pair's own depth and pose were used
    # inv_K left out: K is inverted on the device; the depth form [B,H0,W0]
    stream.reset()
    stream.push(frames[0])
    g = geo[0]
    r = stream.push(frames[1], depth=g["depth"][:, 0], T=g["T"], K=g["K"])
    rigid, motion = V.rigid_flow(g["depth"], g["T"], g["K"], torch.linalg.inv(g["K"]), flow=r.flow_up, valid=r.valid, alpha=0.02, beta=0.75)
    assert torch.equal(bits(r.rigid), bits(rigid)) and torch.equal(r.motion, motion)


# ---- graph=True ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small", "basic"])
def test_rigid_graph_stream(gpu_device, V, deterministic, kind):
    """The same four frames, depths and poses through the eager and the graph stream: bit-equal on every pair and every field;
    reset() and the same frames: replay against replay, bit for bit, without a new capture; another depth or T between two
    pushes changes the result and captures nothing."""
    model = make_model(kind, gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    geo = geometry(gpu_device, 1)
    eager = V.RigidFlowStream(model, iters=ITERS, graph=False, bidirectional=True)
    graphed = V.RigidFlowStream(model, iters=ITERS, graph=True, bidirectional=True)
    want, got = run_stream(eager, f, geo), run_stream(graphed, f, geo)
    assert graphed.graph is not None and not graphed.stale()
    assert len(want) == len(got) == 3 and all(x is not None for x in got[0])
    assert [differing(w, g) for w, g in zip(want, got)] == [[], [], []]
    for g, a in zip(got, geo):
        rigid, motion = V.rigid_flow(a["depth"], a["T"], a["K"], a["inv_K"], flow=g[1], valid=g[5])
        assert torch.equal(bits(g[7]), bits(rigid)) and torch.equal(g[8], motion)
    # reset() and the same frames: replay against replay, without a new capture
    captured = graphed.graph
    graphed.reset()
    again = run_stream(graphed, f, geo)
    assert graphed.graph is captured
    assert len(again) == 3 and [differing(a, g) for a, g in zip(again, got)] == [[], [], []]
    # the same frame pair with another depth, then another T: the flow stands, rigid and motion follow, nothing is captured
    graphed.reset()
    graphed.push(f[0])
    base = graphed.push(f[1], **geo[0])
    base = (base.flow_up.clone(), base.rigid.clone(), base.motion.clone())
    for change in ("depth", "T"):
        other = dict(geo[0])
        other[change] = geo[1][change]
        graphed.reset()
        graphed.push(f[0])
        r = graphed.push(f[1], **other)
        assert graphed.graph is captured
        assert torch.equal(bits(r.flow_up), bits(base[0])) and not torch.equal(bits(r.rigid), bits(base[1])), change
        rigid, motion = V.rigid_flow(other["depth"], other["T"], other["K"], other["inv_K"], flow=r.flow_up, valid=r.valid)
        assert torch.equal(bits(r.rigid), bits(rigid)) and torch.equal(r.motion, motion), change


# ---- rigid=False ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_without_rigid_nothing_changes(gpu_device, V, deterministic, graph):
    """FlowStream, and RigidFlowStream(rigid=False): the new fields are None, push(frame) takes no further argument and returns the
    bits the stream composed by hand returns (what it returned before the mode existed: the same launches)."""
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    plain = V.FlowStream(model, iters=ITERS, graph=graph, bidirectional=True)
    off = V.RigidFlowStream(model, iters=ITERS, graph=graph, bidirectional=True, rigid=False)
    a, b = run_stream(plain, f, None), run_stream(off, f, None)
    assert [differing(x, y) for x, y in zip(a, b)] == [[], [], []]
    assert all(x[7] is None and x[8] is None and x[5] is not None for x in a + b)
    # by hand: ingest, encode, refine_pair, the kept flow, the masks, the picture
    padder = V.InputPadder((H0, W0))
    with torch.no_grad():
        feats = [model.encode_frame(V.frame_ingest(x, padder._pad)) for x in f]
        kept = None
        for i, got in enumerate(a):
            up = model.refine_pair(feats[i], feats[i + 1], iters=ITERS, flow_init=kept, last_only=True)[-1]
            low = model.flow_low[-1]
            kept = V.forward_interpolate(low)
            up = padder.unpad(up)
            valid, valid_bw = V.flow_consistency(up[:1], up[1:])
            hand = [low[:1], up[:1], V.flow_to_image(up[:1]), low[1:], up[1:], valid, valid_bw, None, None]
            assert differing(hand, got) == [], i
    from deep_visual_slam_amd._lib import DvsError
    with pytest.raises(DvsError, match="arguments of a rigid stream"):
        plain.push(f[0], depth=torch.ones(1, 1, H0, W0, device=gpu_device))


# ---- host=True ------------------------------------------------------------------------------------------------------------------------------
def test_motion_host_is_filled_like_valid_host(gpu_device, V):
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    geo = geometry(gpu_device, 1)
    stream = V.RigidFlowStream(model, iters=ITERS, host=True, graph=False, bidirectional=True)
    assert stream.push(f[0]) is None
    r1 = stream.push(f[1], **geo[0])
    motion1 = r1.motion.cpu().numpy()
    r2 = stream.push(f[2], **geo[1])
    assert r1._slot is not r2._slot and r2._slot["motion"].is_pinned() and r2._slot["event"] is not r1._slot["event"]
    assert np.array_equal(r2.motion_host, r2.motion.cpu().numpy()) and np.array_equal(r2.valid_host, r2.valid.cpu().numpy())
    assert np.array_equal(r1.motion_host, motion1)                            # valid until the push after next
    assert r1.motion_host.dtype == np.uint8 and r1.motion_host.shape == (1, H0, W0) and set(np.unique(motion1)) <= {0, 1, 2}
    r3 = stream.push(f[3], **geo[2])
    assert r3._slot is r1._slot and np.array_equal(r3.motion_host, r3.motion.cpu().numpy())
    one = V.FlowStream(model, iters=ITERS, host=True, graph=False)
    one.push(f[0])
    assert one.push(f[1]).motion_host is None


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_missing_and_misshaped_arguments(gpu_device, V, graph):
    """A missing depth, T or K, or one of another shape, dtype or device, is a DvsError that names it, raised before anything
    runs: the stream then takes the same frame with proper arguments as if nothing had happened."""
    from deep_visual_slam_amd._lib import DvsError
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    g = geometry(gpu_device, 1, pairs=1)[0]
    stream = V.RigidFlowStream(model, iters=ITERS, graph=graph)
    assert stream.push(f[0]) is None                                          # the first frame completes no pair and needs none
    for name in ("depth", "T", "K"):
        with pytest.raises(DvsError, match="FlowStream: a rigid stream needs %s " % name):
            stream.push(f[1], **{k: v for k, v in g.items() if k != name})
    with pytest.raises(DvsError, match="needs depth"):
        stream.push(f[1])
    bad = [("depth", g["depth"][:, :, :-1], r"FlowStream: depth: .* got \(1, 1, 129, 141\)"),
           ("depth", g["depth"].double(), "FlowStream: depth: fp32 only"),
           ("depth", g["depth"].cpu(), "FlowStream: depth: GPU tensors only"),
           ("T", g["T"][0], r"FlowStream: T: \[1,4,4\] expected, got \(4, 4\)"),
           ("K", g["K"][:3, :3], r"FlowStream: K: \[1,4,4\] or \[4,4\] expected, got \(3, 3\)"),
           ("inv_K", g["inv_K"][None].repeat(2, 1, 1), r"FlowStream: inv_K: \[1,4,4\] or \[4,4\] expected")]
    for name, value, msg in bad:
        with pytest.raises(DvsError, match=msg):
            stream.push(f[1], **{**g, name: value})
    r = stream.push(f[1], **g)
    fresh = V.RigidFlowStream(model, iters=ITERS, graph=False)
    fresh.push(f[0])
    w = fresh.push(f[1], **g)
    assert r.valid is None and tuple(r.motion.shape) == (1, H0, W0)
    rigid, motion = V.rigid_flow(g["depth"], g["T"], g["K"], g["inv_K"], flow=r.flow_up)
    assert torch.equal(bits(r.rigid), bits(rigid)) and torch.equal(r.motion, motion)
    assert torch.equal(bits(r.rigid), bits(w.rigid))                          # rigid does not depend on the flow
