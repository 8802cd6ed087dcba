"""Bidirectional RAFT on the GPU (raft.refine_pair, raft_video.FlowStream(bidirectional=True)): both directions of a pair as one loop
at batch 2N, and the forward-backward consistency masks of csrc/flowcons.hip inside the stream.

130x141 frames (padded 136x144), iters = 2, the seeded weights and images of raft_ref / raft_basic_ref: the models, frames, helpers
and the bound OUT_TOL * max|flow| are those of tests/test_raftstream_gpu.py (a convolution route may differ between batch N and
2N, so refine_pair need not be bit-equal to two refine calls; what the stream keeps, masks and replays is compared bit for bit).
Measured on the MI355X: see DESIGN.md section 23."""
import pytest
import torch

import test_raftstream_gpu as S
from test_raftstream_gpu import H0, ITERS, TOL, W0, bits, make_model, u8_frames, within

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import raft_video
    return raft_video


def encode(V, model, frame, dev, mode="sintel"):
    padder = V.InputPadder((H0, W0), mode)
    return model.encode_frame(V.frame_ingest(frame.to(dev), padder._pad))


def pair_by_hand(V, model, kind, fa, fb, flow_init):
    """(flow_low [2N], padded flow_up [2N]) of refine_pair in the mode the stream runs."""
    if kind == "basic":
        return model.refine_pair(fa, fb, iters=ITERS, flow_init=flow_init, test_mode=True)
    up = model.refine_pair(fa, fb, iters=ITERS, flow_init=flow_init, last_only=True)[-1]
    return model.flow_low[-1], up


# ---- refine_pair ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("init", [False, True], ids=["cold", "flow_init"])
@pytest.mark.parametrize("alternate", [False, True], ids=["CorrBlock", "AlternateCorrBlock"])
@pytest.mark.parametrize("kind", ["small", "basic"])
def test_refine_pair_is_two_refines(gpu_device, V, kind, alternate, init, N):
    """Rows [0:N] against refine(f1, f2) and rows [N:2N] against refine(f2, f1), every iteration, and test_mode / last_only."""
    model = make_model(kind, gpu_device, alternate)
    a, b = u8_frames(N)[:2]
    flow_init = None
    if init:
        flow_init = (2.0 * torch.randn(2 * N, 2, 17, 18, generator=torch.Generator().manual_seed(6))).to(gpu_device)
    half = lambda i: None if flow_init is None else flow_init[i * N:(i + 1) * N]
    tag = "%s %s" % (kind, "alt" if alternate else "corr")
    with torch.no_grad():
        fa, fb = encode(V, model, a, gpu_device), encode(V, model, b, gpu_device)
        got = model.refine_pair(fa, fb, iters=ITERS, flow_init=flow_init)
        low = [f.clone() for f in model.flow_low]
        want_fw = model.refine(fa, fb, iters=ITERS, flow_init=half(0))
        low_fw = [f.clone() for f in model.flow_low]
        want_bw = model.refine(fb, fa, iters=ITERS, flow_init=half(1))
        low_bw = model.flow_low
        assert len(got) == len(low) == ITERS
        for i in range(ITERS):
            assert tuple(got[i].shape) == (2 * N, 2, 136, 144) and tuple(low[i].shape) == (2 * N, 2, 17, 18)
            within("%s forward iteration %d" % (tag, i), got[i][:N], want_fw[i], TOL[kind])
            within("%s backward iteration %d" % (tag, i), got[i][N:], want_bw[i], TOL[kind])
            within("%s forward flow_low %d" % (tag, i), low[i][:N], low_fw[i], TOL[kind])
            within("%s backward flow_low %d" % (tag, i), low[i][N:], low_bw[i], TOL[kind])
        assert float((want_fw[-1] - want_bw[-1]).abs().max()) > 100 * TOL[kind] * float(want_fw[-1].abs().max())   # two different flows
        if kind == "basic":
            low_g, up_g = model.refine_pair(fa, fb, iters=ITERS, flow_init=flow_init, test_mode=True)
            low_w, up_w = model.refine(fb, fa, iters=ITERS, flow_init=half(1), test_mode=True)
            within("basic test_mode backward flow_up", up_g[N:], up_w, TOL[kind])
            within("basic test_mode backward flow_low", low_g[N:], low_w, TOL[kind])
            within("basic test_mode forward flow_up", up_g[:N], want_fw[-1], TOL[kind])
        else:
            last = model.refine_pair(fa, fb, iters=ITERS, flow_init=flow_init, last_only=True)
            assert len(last) == 1
            within("small last_only forward", last[0][:N], want_fw[-1], TOL[kind])
            within("small last_only backward", last[0][N:], want_bw[-1], TOL[kind])


def test_refine_pair_refuses_a_flow_init_of_batch_n(gpu_device, V):
    from deep_visual_slam_amd._lib import DvsError
    model = make_model("small", gpu_device)
    a, b = u8_frames(1)[:2]
    with torch.no_grad():
        fa, fb = encode(V, model, a, gpu_device), encode(V, model, b, gpu_device)
        with pytest.raises(DvsError, match=r"refine_pair: flow_init must be a fp32 \[2,2,17,18\]"):
            model.refine_pair(fa, fb, iters=ITERS, flow_init=torch.zeros(1, 2, 17, 18, device=gpu_device))


# ---- the eager stream -------------------------------------------------------------------------------------------------------------------
def check_frame(V, r, B):
    assert tuple(r.flow_low.shape) == tuple(r.flow_low_bw.shape) == (B, 2, 17, 18)
    assert tuple(r.flow_up.shape) == tuple(r.flow_up_bw.shape) == (B, 2, H0, W0)
    assert r.valid.dtype == r.valid_bw.dtype == torch.uint8 and tuple(r.valid.shape) == tuple(r.valid_bw.shape) == (B, H0, W0)
    valid, valid_bw = V.flow_consistency(r.flow_up, r.flow_up_bw)
    assert torch.equal(r.valid, valid) and torch.equal(r.valid_bw, valid_bw)
    assert torch.equal(r.image, V.flow_to_image(r.flow_up))                    # the picture is the forward pair's
    assert torch.isfinite(r.flow_up).all() and torch.isfinite(r.flow_up_bw).all()


@pytest.mark.parametrize("kind,B,mode", [("small", 1, "sintel"), ("basic", 2, "kitti")])
def test_bidirectional_stream_over_four_frames(gpu_device, V, kind, B, mode):
    """Each pair against the hand-composed refine_pair(previous, current, flow_init = the stream's OWN kept flow before that push);
    the kept flow (all 2B rows) and the masks bit for bit; one fnet and one cnet call of batch B per pushed frame."""
    model = make_model(kind, gpu_device)
    frames = u8_frames(B)
    stream = V.FlowStream(model, iters=ITERS, pad_mode=mode, graph=False, bidirectional=True)
    calls = S.Calls(model)
    try:
        assert stream.push(frames[0].to(gpu_device)) is None and stream.flow_init is None
        assert calls.take() == [("cnet", B), ("fnet", B)]
        results, kept_before = [], []
        for cur in frames[1:]:
            kept_before.append(None if stream.flow_init is None else stream.flow_init.clone())
            r = stream.push(cur.to(gpu_device))
            assert calls.take() == [("cnet", B), ("fnet", B)]                 # the backward pair costs no encoder pass
            check_frame(V, r, B)
            assert tuple(stream.flow_init.shape) == (2 * B, 2, 17, 18)
            assert torch.equal(bits(stream.flow_init), bits(V.forward_interpolate(torch.cat((r.flow_low, r.flow_low_bw), 0))))
            results.append(r)
    finally:
        calls.remove()
    assert kept_before[0] is None and kept_before[1] is not None
    padder = V.InputPadder((H0, W0), mode)
    with torch.no_grad():
        feats = [encode(V, model, f, gpu_device, mode) for f in frames]
        for i, r in enumerate(results):
            low, up = pair_by_hand(V, model, kind, feats[i], feats[i + 1], kept_before[i])
            up = padder.unpad(up)
            bound = within("%s pair %d flow_up" % (kind, i), r.flow_up, up[:B], TOL[kind])
            within("%s pair %d flow_up_bw" % (kind, i), r.flow_up_bw, up[B:], TOL[kind])
            within("%s pair %d flow_low" % (kind, i), r.flow_low, low[:B], TOL[kind])
            within("%s pair %d flow_low_bw" % (kind, i), r.flow_low_bw, low[B:], TOL[kind])
            assert r.flow_up.stride() == up[:B].stride() and r.flow_up_bw.stride() == up[B:].stride()
            if i == 1:
                _, cold = pair_by_hand(V, model, kind, feats[1], feats[2], None)
                diff = float((r.flow_up_bw - padder.unpad(cold)[B:]).abs().max())
                print("%s pair 1 backward vs a cold start: %.3e (bound %.3e)" % (kind, diff, bound))
                assert diff > bound                                            # the kept backward flow was used


def test_one_directional_stream_has_the_new_fields_as_none(gpu_device, V):
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    stream = V.FlowStream(model, iters=ITERS, graph=False, bidirectional=False)
    assert stream.push(f[0]) is None
    r = stream.push(f[1])
    assert isinstance(r, V.FlowFrame) and tuple(r.flow_up.shape) == (1, 2, H0, W0) and tuple(stream.flow_init.shape) == (1, 2, 17, 18)
    assert (r.flow_low_bw, r.flow_up_bw, r.valid, r.valid_bw) == (None, None, None, None)
    both = V.FlowStream(model, iters=ITERS, graph=False, bidirectional=True, warm_start=False, image=False)
    both.push(f[0])
    r2 = both.push(f[1])
    assert both.flow_init is None and r2.image is None and r2.valid is not None
    within("the forward pair of a bidirectional stream", r2.flow_up, r.flow_up, TOL["small"])
    # other thresholds reach the kernel
    loose = V.FlowStream(model, iters=ITERS, graph=False, bidirectional=True, fb_alpha=1.0, fb_beta=1e6)
    loose.push(f[0])
    r3 = loose.push(f[1])
    assert torch.equal(r3.valid, V.flow_consistency(r3.flow_up, r3.flow_up_bw, 1.0, 1e6)[0])
    assert int(r3.valid.sum()) >= int(r2.valid.sum())


# ---- graph=True ---------------------------------------------------------------------------------------------------------------------------
FIELDS = ("flow_low", "flow_up", "image", "flow_low_bw", "flow_up_bw", "valid", "valid_bw")


def run_stream(stream, frames):
    """Clones of every field of every pair: a graph's outputs are valid until the next push only."""
    out = []
    for x in frames:
        r = stream.push(x)
        if r is not None:
            out.append([getattr(r, name).clone() for name in FIELDS])
    return out


def differing(a, g):
    raw = lambda t: t if t.dtype == torch.uint8 else bits(t)
    return [name for name, x, y in zip(FIELDS, a, g) if not torch.equal(raw(x), raw(y))]


@pytest.fixture
def deterministic():
    """dvs_set_deterministic(1) for one test: the mode in which a forward repeats exactly (tests/test_raftstream_gpu.py says why
    the chained and the bit-for-bit comparisons are made in it)."""
    from deep_visual_slam_amd import _lib
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


@pytest.mark.parametrize("kind", ["small", "basic"])
def test_bidirectional_graph_stream(gpu_device, V, deterministic, kind):
    """The same four frames through the eager and the graph stream: bit-equal on every pair; reset() and the same frames: replay
    against replay, bit for bit, without a new capture; a weight changed in place: stale(), and a new capture."""
    model = make_model(kind, gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    eager = V.FlowStream(model, iters=ITERS, graph=False, bidirectional=True)
    graphed = V.FlowStream(model, iters=ITERS, graph=True, bidirectional=True)
    assert graphed.push(f[0]) is None and eager.push(f[0]) is None
    assert graphed.graph is not None and not graphed.stale()
    assert tuple(graphed.flow_init.shape) == (2, 2, 17, 18) and not graphed.flow_init.any()      # a zeroed buffer is the cold start
    want, got = run_stream(eager, f[1:]), run_stream(graphed, f[1:])
    assert len(want) == len(got) == 3 and not graphed.stale()
    assert [differing(w, g) for w, g in zip(want, got)] == [[], [], []]
    assert torch.equal(bits(graphed.flow_init), bits(eager.flow_init))
    for g in got:
        valid, valid_bw = V.flow_consistency(g[1], g[4])
        assert torch.equal(g[5], valid) and torch.equal(g[6], valid_bw)
    # reset() and the same frames: replay against replay, without a new capture
    captured = graphed.graph
    graphed.reset()
    assert not graphed.flow_init.any()
    assert graphed.push(f[0]) is None
    again = run_stream(graphed, f[1:])
    assert graphed.graph is captured
    assert len(again) == 3 and [differing(a, g) for a, g in zip(again, got)] == [[], [], []]
    # a weight changed in place
    eager.reset(), graphed.reset()
    for x in f[:2]:
        eager.push(x), graphed.push(x)
    weight = next(model.update_block.parameters())
    saved = weight.detach().clone()
    try:
        with torch.no_grad():
            weight.mul_(1.25)
        assert graphed.stale()
        w, g = eager.push(f[2]), graphed.push(f[2])
        assert not graphed.stale() and graphed.graph is not captured
        for name in ("flow_up", "flow_up_bw"):
            within("%s after the weight change %s" % (kind, name), getattr(g, name), getattr(w, name), TOL[kind])
        moved = float((g.flow_up_bw - got[1][4]).abs().max())
        print("%s: the new weights move the backward flow by %.3e" % (kind, moved))
        assert moved > TOL[kind] * float(w.flow_up_bw.abs().max())
    finally:
        with torch.no_grad():
            weight.copy_(saved)


# ---- host=True ------------------------------------------------------------------------------------------------------------------------------
def test_valid_host_is_filled_like_image_host(gpu_device, V):
    import numpy as np
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    stream = V.FlowStream(model, iters=ITERS, host=True, graph=False, bidirectional=True)
    assert stream.push(f[0]) is None
    r1 = stream.push(f[1])
    valid1 = r1.valid.cpu().numpy()
    r2 = stream.push(f[2])
    assert r1._slot is not r2._slot and r2._slot["valid"].is_pinned()
    assert np.array_equal(r2.valid_host, r2.valid.cpu().numpy()) and np.array_equal(r2.image_host, r2.image.cpu().numpy())
    assert np.array_equal(r2.flow_low_host, r2.flow_low.cpu().numpy())
    assert np.array_equal(r1.valid_host, valid1)                              # valid until the push after next
    assert r1.valid_host.dtype == np.uint8 and r1.valid_host.shape == (1, H0, W0)
    r3 = stream.push(f[3])
    assert r3._slot is r1._slot and np.array_equal(r3.valid_host, r3.valid.cpu().numpy())
    one = V.FlowStream(model, iters=ITERS, host=True, graph=False)
    one.push(f[0])
    assert one.push(f[1]).valid_host is None
