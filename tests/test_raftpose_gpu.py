"""The pose mode of the RAFT frame stream on the GPU (raft_video.PoseFlowStream, csrc/posefit.hip inside the stream): every pair also
carries the camera motion fitted to its own flow_up, and rigid and motion are taken under that motion.

130x141 frames (padded 136x144), iters = 2, the seeded weights and images of tests/test_raftstream_gpu.py; depth and intrinsics are
synthetic (posefit_ref.scene), a different depth for every pair.  The flow of seeded weights on random images fits no camera: what
the stream computes is compared BIT FOR BIT with fit_pose and rigid_flow composed by hand on the stream's own flow_up and valid.
Measured on the MI355X: DESIGN.md section 26."""
import numpy as np
import pytest
import torch

import posefit_ref as P
from test_raftrigid_gpu import deterministic, geometry  # noqa: F401  (a fixture, and RigidFlowStream's arguments)
from test_raftstream_gpu import H0, ITERS, W0, bits, make_model, u8_frames

pytestmark = pytest.mark.gpu

# The two flows of the seeded, untrained weights agree on no pixel under the default thresholds, and a stream
# whose mask is empty never fits.  With these a pixel is valid wherever its target stays in the image -- a mask that is neither
# empty nor full (0.75 of the pixels), and another one in each direction -- so that the bidirectional streams below fit for real,
# through a mask in round 1 and through the static label in round 2.
LOOSE = dict(fb_alpha=1.0, fb_beta=1e6)


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import raft_video
    return raft_video


def scenes(dev, B, pairs=3):
    """[dict(depth [B,1,H0,W0], K [4,4], inv_K [4,4])] on the device, one per pair."""
    out = []
    for i in range(pairs):
        s = P.scene(H0, W0, N=B, seed=60 + i)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        out.append(dict(depth=t(s.depth), K=t(s.K), inv_K=t(s.iK)))
    return out


def raw(t):
    return t if t.dtype == torch.uint8 else bits(t) if t.dtype == torch.float32 else t


FIELDS = ("flow_low", "flow_up", "image", "flow_low_bw", "flow_up_bw", "valid", "valid_bw", "rigid", "motion", "T", "pose_status")


def run_stream(stream, frames, geo, guess=None):
    out = []
    for i, x in enumerate(frames):
        kw = dict(geo[i - 1]) if i and geo is not None else {}
        if i and guess is not None:
            kw["T"] = guess
        r = stream.push(x, **kw)
        if i == 0:
            assert r is None
        else:
            out.append([None if getattr(r, name) is None else getattr(r, name).clone() for name in FIELDS])
    return out


def differing(a, g):
    return [name for name, x, y in zip(FIELDS, a, g) if (x is None) != (y is None) or (x is not None and not torch.equal(raw(x), raw(y)))]


def by_hand(V, g, flow_up, valid, T0=None, rounds=2, iters=4, huber=1.0, alpha=0.01, beta=0.5):
    """(T, status, rigid, motion): what the stream is documented to compute."""
    T, mask = T0, valid
    for r in range(rounds):
        if r:
            _, label = V.rigid_flow(g["depth"], T, g["K"], g["inv_K"], flow=flow_up, valid=valid, alpha=alpha, beta=beta)
            mask = (label == 1).view(torch.uint8)
        T, status = V.fit_pose(g["depth"], flow_up, g["K"], g["inv_K"], T0=T, valid=mask, iters=iters, huber=huber)
    rigid, motion = V.rigid_flow(g["depth"], T, g["K"], g["inv_K"], flow=flow_up, valid=valid, alpha=alpha, beta=beta)
    return T, status, rigid, motion


# ---- the eager stream -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidirectional", [False, True], ids=["forward", "bidirectional"])
@pytest.mark.parametrize("kind,B", [("small", 1), ("basic", 2)])
def test_eager_pose_stream_over_four_frames(gpu_device, V, kind, B, bidirectional):
    model = make_model(kind, gpu_device)
    frames = [x.to(gpu_device) for x in u8_frames(B)]
    geo = scenes(gpu_device, B)
    stream = V.PoseFlowStream(model, iters=ITERS, graph=False, bidirectional=bidirectional, rigid_alpha=0.02, rigid_beta=0.75,
                              pose_iters=3, pose_huber=2.0, **LOOSE)
    assert stream.push(frames[0]) is None
    seen = []
    for cur, g in zip(frames[1:], geo):
        r = stream.push(cur, **g)
        assert tuple(r.T.shape) == (B, 4, 4) and r.T.dtype == torch.float32
        assert tuple(r.pose_status.shape) == (B,) and r.pose_status.dtype == torch.int32
        assert tuple(r.rigid.shape) == (B, 2, H0, W0) and tuple(r.motion.shape) == (B, H0, W0)
        assert (r.valid is not None) == bidirectional and not r.flow_up.is_contiguous()
        T, status, rigid, motion = by_hand(V, g, r.flow_up, r.valid, iters=3, huber=2.0, alpha=0.02, beta=0.75)
        assert torch.equal(bits(r.T), bits(T)) and torch.equal(r.pose_status, status)
        assert torch.equal(bits(r.rigid), bits(rigid)) and torch.equal(r.motion, motion)
        assert bool(torch.isfinite(r.T).all())
        if bidirectional:                                   # the mask is a mask: some pixels out, most in, and it is the forward one
            share = float(r.valid.float().mean())
            print("%s B=%d: %.4f of the pixels valid" % (kind, B, share))
            assert 0.0 < share < 1.0 and not torch.equal(r.valid, r.valid_bw)
            # the other direction's mask gives another pose.  (No mask at all gives the SAME pose here: under LOOSE a pixel is valid
            # exactly where its target stays in the image, which the kernel requires of a judged pixel anyway.)
            wrong = by_hand(V, g, r.flow_up, r.valid_bw, iters=3, huber=2.0, alpha=0.02, beta=0.75)[0]
            assert not torch.equal(bits(wrong), bits(T))
        seen.append((r.T.clone(), r.pose_status.clone()))
    print("%s B=%d bidirectional=%s: status %s" % (kind, B, bidirectional, [s.tolist() for _, s in seen]))
    assert not any(bool(s.any()) for _, s in seen)                                # every pair was fitted: status 0
    assert not torch.equal(bits(seen[0][0]), bits(seen[1][0]))                    # each pair's own depth was used
    # inv_K left out, the depth form [B,H0,W0], a guess, one round
    once = V.PoseFlowStream(model, iters=ITERS, graph=False, bidirectional=bidirectional, pose_rounds=1, **LOOSE)
    once.push(frames[0])
    g = geo[0]
    guess = torch.from_numpy(P.start(B, 9)).to(gpu_device)
    r = once.push(frames[1], depth=g["depth"][:, 0], K=g["K"], T=guess)
    hand = dict(g, inv_K=torch.linalg.inv(g["K"]))
    T, status, rigid, motion = by_hand(V, hand, r.flow_up, r.valid, T0=guess, rounds=1)
    assert torch.equal(bits(r.T), bits(T)) and torch.equal(r.pose_status, status) and torch.equal(bits(r.rigid), bits(rigid))
    other = by_hand(V, hand, r.flow_up, r.valid, rounds=1)[0]
    assert not torch.equal(bits(other), bits(T))                                  # the guess was used
    two = by_hand(V, hand, r.flow_up, r.valid, T0=guess, rounds=2)[0]
    assert not status.any() and not torch.equal(bits(two), bits(T))               # and one round is one round


# ---- graph=True ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidirectional", [False, True], ids=["forward", "bidirectional"])
@pytest.mark.parametrize("kind", ["small", "basic"])
def test_pose_graph_stream(gpu_device, V, deterministic, kind, bidirectional):  # noqa: F811
    """The same four frames through the eager and the graph stream: bit-equal on every pair and every field; reset() and the
    same frames: replay against replay without a new capture; a guess is copied into the static buffer before the replay, and the
    identity again when none is passed."""
    model = make_model(kind, gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    geo = scenes(gpu_device, 1)
    eager = V.PoseFlowStream(model, iters=ITERS, graph=False, bidirectional=bidirectional, **LOOSE)
    graphed = V.PoseFlowStream(model, iters=ITERS, graph=True, bidirectional=bidirectional, **LOOSE)
    want, got = run_stream(eager, f, geo), run_stream(graphed, f, geo)
    assert graphed.graph is not None and not graphed.stale()
    assert len(want) == len(got) == 3 and all((x is None) == (name in FIELDS[3:7] and not bidirectional) for name, x in zip(FIELDS, got[0]))
    print("%s: status %s" % (kind, [g[10].tolist() for g in got]))
    assert not any(bool(g[10].any()) for g in got)                                # fitted, not skipped
    assert [differing(w, g) for w, g in zip(want, got)] == [[], [], []]
    for g, a in zip(got, geo):
        T, status, rigid, motion = by_hand(V, a, g[1], g[5])
        assert torch.equal(bits(g[9]), bits(T)) and torch.equal(g[10], status) and torch.equal(bits(g[7]), bits(rigid)) and torch.equal(g[8], motion)
    captured = graphed.graph
    graphed.reset()
    again = run_stream(graphed, f, geo)
    assert graphed.graph is captured
    assert len(again) == 3 and [differing(a, g) for a, g in zip(again, got)] == [[], [], []]
    # a guess, then none again: the static T0 follows, nothing is captured
    guess = torch.from_numpy(P.start(1, 9)).to(gpu_device)
    graphed.reset()
    eager.reset()
    with_guess, want_guess = run_stream(graphed, f, geo, guess), run_stream(eager, f, geo, guess)
    assert graphed.graph is captured and [differing(a, g) for a, g in zip(with_guess, want_guess)] == [[], [], []]
    assert "T" in differing(with_guess[0], got[0])
    graphed.reset()
    assert [differing(a, g) for a, g in zip(run_stream(graphed, f, geo), got)] == [[], [], []]


# ---- host=True, and the streams underneath ----------------------------------------------------------------------------------------------
def test_T_host_rides_the_ring(gpu_device, V):
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    geo = scenes(gpu_device, 1)
    stream = V.PoseFlowStream(model, iters=ITERS, host=True, graph=False, bidirectional=True, **LOOSE)
    assert stream.push(f[0]) is None
    r1 = stream.push(f[1], **geo[0])
    T1 = r1.T.cpu().numpy()
    r2 = stream.push(f[2], **geo[1])
    assert not r1.pose_status.any() and not r2.pose_status.any() and not np.array_equal(T1, r2.T.cpu().numpy())    # two fits, two poses
    assert r1._slot is not r2._slot and r2._slot["T"].is_pinned()
    assert np.array_equal(r2.T_host, r2.T.cpu().numpy()) and np.array_equal(r1.T_host, T1)          # valid until the push after next
    assert r2.T_host.dtype == np.float32 and r2.T_host.shape == (1, 4, 4)
    assert np.array_equal(r2.motion_host, r2.motion.cpu().numpy()) and np.array_equal(r2.valid_host, r2.valid.cpu().numpy())
    assert np.array_equal(r2.flow_low_host, r2.flow_low.cpu().numpy()) and np.array_equal(r2.image_host, r2.image.cpu().numpy())
    # the streams underneath: no T in their slots, the new fields None
    rigid = V.RigidFlowStream(model, iters=ITERS, host=True, graph=False, bidirectional=True)
    rigid.push(f[0])
    r = rigid.push(f[1], **geometry(gpu_device, 1, pairs=1)[0])
    assert sorted(r._slot) == ["event", "flow_low", "image", "motion", "valid"] and r.T_host is None
    assert r.T is None and r.pose_status is None


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_rigid_stream_is_unchanged(gpu_device, V, deterministic, graph):  # noqa: F811
    """RigidFlowStream beside the new subclass: every field is what rigid_flow gives by hand for the T it was handed, and a
    PoseFlowStream with rigid=False is a plain FlowStream."""
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    geo = geometry(gpu_device, 1)
    rigid = V.RigidFlowStream(model, iters=ITERS, graph=graph, bidirectional=True)
    plain = V.FlowStream(model, iters=ITERS, graph=graph, bidirectional=True)
    off = V.PoseFlowStream(model, iters=ITERS, graph=graph, bidirectional=True, rigid=False)
    a, b, c = run_stream(rigid, f, geo), run_stream(plain, f, None), run_stream(off, f, None)
    for x, y, z, g in zip(a, b, c, geo):
        assert differing(x[:7] + [None] * 4, y) == [] and differing(y, z) == []
        assert x[9] is None and x[10] is None and all(t is None for t in y[7:])
        hand = V.rigid_flow(g["depth"], g["T"], g["K"], g["inv_K"], flow=x[1], valid=x[5])
        assert torch.equal(bits(x[7]), bits(hand[0])) and torch.equal(x[8], hand[1])


def test_missing_arguments(gpu_device, V):
    from deep_visual_slam_amd._lib import DvsError
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    g = scenes(gpu_device, 1, pairs=1)[0]
    stream = V.PoseFlowStream(model, iters=ITERS, graph=False)
    assert stream.push(f[0]) is None
    for name in ("depth", "K"):
        with pytest.raises(DvsError, match="FlowStream: a rigid stream needs %s " % name):
            stream.push(f[1], **{k: v for k, v in g.items() if k != name})
    with pytest.raises(DvsError, match=r"FlowStream: T: \[1,4,4\] expected, got \(4, 4\)"):
        stream.push(f[1], T=torch.eye(4, device=gpu_device), **g)
    r = stream.push(f[1], **g)
    T, status, rigid, motion = by_hand(V, g, r.flow_up, None)
    assert torch.equal(bits(r.T), bits(T)) and torch.equal(r.motion, motion)
