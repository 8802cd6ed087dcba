"""The RAFT frame stream on the GPU (csrc/ingest.hip, raft.encode_frame / refine, raft_video.FlowStream).

dvs_frame_ingest: EXACTLY tests/golden/raftstream_ingest.npz (what the reference's .float() / 255.0, InputPadder.pad and
2 * x - 1.0 returned on the CPU) and the NumPy restatement of tests/raftstream_ref.py, compared as int32 bit patterns, the zero
fourth channel included.  Every operation of the chain is correctly rounded on both sides, so there is no tolerance.

encode_frame / refine and the stream: against the hand-composed pair forward, within OUT_TOL * max|flow| -- the tolerance of
tests/test_raft_gpu.py and tests/test_raft_basic_gpu.py, which tests/test_flowstage_gpu.py already reuses for the same kind of
comparison (a convolution route may differ between batch N and 2N, so the per-frame form need not be bit-equal).
Measured on the MI355X: see DESIGN.md section 22.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import layouts
import raft_basic_ref as RB
import raft_ref as RS
import raftstream_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
FIXTURE = "raftstream_ingest.npz"
H0, W0 = 130, 141          # pads to 136 x 144
ITERS = 2
TOL = {"small": RS.OUT_TOL, "basic": RB.OUT_TOL}


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


@pytest.fixture(scope="module")
def V():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import raft_video
    return raft_video


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- dvs_frame_ingest ---------------------------------------------------------------------------------------------------------------
def run_ingest(V, frames, pad, bgr=False):
    """frame_ingest's result as the dense [N,Hp,Wp,4] the kernel wrote, on the host."""
    out = V.frame_ingest(frames, pad, bgr)
    N, H, W, _ = frames.shape if frames.dim() == 4 else (1,) + tuple(frames.shape)
    assert tuple(out.shape) == (N, 4, pad[2] + H + pad[3], pad[0] + W + pad[1]) and out.dtype == torch.float32 and out.is_cuda
    nhwc = out.permute(0, 2, 3, 1)
    assert nhwc.is_contiguous() and out.data_ptr() % 16 == 0
    return nhwc.cpu().numpy()


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    return int((R.bits(got) != R.bits(want)).sum())


@pytest.mark.parametrize("H,W", R.SIZES, ids=["%dx%d" % s for s in R.SIZES])
def test_ingest_equals_the_reference_exactly(gpu_device, rec, V, H, W):
    """Both pad modes against the fixture (N = 1) and, with the explicit pads, RGB and BGR, N = 1 and 3, against the restatement."""
    frames3 = R.make_frame(H, W, N=3)
    assert np.array_equal(frames3[:1], rec[R.frame_key(H, W)])
    dev3 = torch.from_numpy(frames3).to(gpu_device)
    wrong = 0
    for mode in R.MODES:
        pad = tuple(int(v) for v in rec[R.out_key(H, W, mode) + "/pad"])
        got = run_ingest(V, dev3[:1], pad)
        wrong += same_bits(R.nchw(got), rec[R.out_key(H, W, mode)])
        wrong += int(R.bits(got[..., 3]).any())
    pads = [R.pads(H, W, m) for m in R.MODES] + list(R.EXPLICIT_PADS)
    for pad in pads:
        for bgr in (False, True):
            for N in (1, 3):
                wrong += same_bits(run_ingest(V, dev3[:N], pad, bgr), R.ingest(frames3[:N], pad, bgr))
    single = run_ingest(V, dev3[0], R.EXPLICIT_PADS[1])                   # the [H,W,3] form
    wrong += same_bits(single, R.ingest(frames3[:1], R.EXPLICIT_PADS[1]))
    print("%dx%d: %d elements differ over %d launches" % (H, W, wrong, 2 + 4 * len(pads) + 1))
    assert wrong == 0


def test_ingest_every_byte_value(gpu_device, rec, V):
    frames = rec["frame/all256"]
    got = run_ingest(V, torch.from_numpy(frames).to(gpu_device), (0, 0, 0, 0))
    assert same_bits(R.nchw(got), rec["ingest/all256"]) == 0 and not R.bits(got[..., 3]).any()
    assert len(np.unique(got[..., :3])) == 256


VIEW_SIZES = [(7, 131), (2, 64), (7, 4), (1, 1)]
IN_PLACE = ("planar", "offset", "batch_slice", "chan_slice")             # pixels stay three adjacent bytes: read through strides


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", VIEW_SIZES, ids=["%dx%d" % s for s in VIEW_SIZES])
def test_ingest_reads_views_in_place_or_copies_them(gpu_device, V, H, W, N):
    """Every uint8 view of tests/layouts.py that applies to [N,H,W,3], and a crop of a wider frame: read in place where the
    pixels are three adjacent bytes, copied once otherwise, never read as dense (the views' surroundings hold a sentinel)."""
    frames = R.make_frame(H, W, N)
    dense = torch.from_numpy(frames).to(gpu_device)
    pad = (3, 4, 0, 7)
    want = R.ingest(frames, pad)
    seen = []
    for kind, v in layouts.views(dense):
        assert torch.equal(v, dense)
        kept = V._packed(v)[0]
        if kind in IN_PLACE:
            assert kept is v, kind
        elif kind in ("crop", "transposed") and W > 1:                    # pixels 7 bytes apart / channels not adjacent: one copy
            assert kept is not v and kept.is_contiguous(), kind
        assert same_bits(run_ingest(V, v, pad), want) == 0, kind
        seen.append(kind)
    assert set(("planar", "offset", "batch_slice", "crop")) <= set(seen)
    # the crop a caller means: a window of a wider frame, rows 3 * W + 4 bytes apart, starting 2 bytes into a row
    rows = layouts.make(dense.reshape(N, H, 3 * W), "crop")
    window = rows.unflatten(-1, (W, 3))
    assert torch.equal(window, dense) and V._packed(window)[0] is window
    if H > 1:
        assert window.stride(1) == 3 * W + 4
    assert same_bits(run_ingest(V, window, pad), want) == 0
    assert same_bits(run_ingest(V, window, pad, True), R.ingest(frames, pad, True)) == 0


def test_ingest_repeats_and_ignores_batch_neighbours(gpu_device, V):
    frames = R.make_frame(7, 64, N=3)
    dev = torch.from_numpy(frames).to(gpu_device)
    pad = R.pads(7, 64, "sintel")
    a, b = run_ingest(V, dev, pad), run_ingest(V, dev, pad)
    assert same_bits(a, b) == 0
    other = dev.clone()
    other[0], other[2] = 255 - other[0], 17
    c = run_ingest(V, other, pad)
    assert same_bits(a[1], c[1]) == 0 and same_bits(a[0], c[0]) > 0
    assert same_bits(run_ingest(V, dev[1], pad)[0], a[1]) == 0


# ---- models and frames ----------------------------------------------------------------------------------------------------------------
_MODELS = {}


def make_model(kind, dev, alternate=False):
    """One model per kind with the seeded weights of raft_ref / raft_basic_ref; the correlation block is a switch of the model."""
    from deep_visual_slam_amd import raft
    if kind not in _MODELS:
        if kind == "small":
            model = raft.SmallRAFT(SimpleNamespace(alternate_corr=False))
            model.load_state_dict(RS.make_weights(RS.G6["weight_seed"]), strict=True)
        else:
            model = raft.RAFT(SimpleNamespace(small=False, alternate_corr=False))
            model.load_state_dict(RB.make_weights(RB.G6["weight_seed"]), strict=True)
        _MODELS[kind] = model.to(dev)
    model = _MODELS[kind].eval()
    model.alternate_corr = bool(alternate)
    return model


_FRAMES = {}


def u8_frames(B):
    """Four uint8 frames [B,H0,W0,3] on the host, made once: the seeded images of raft_ref, quantised."""
    if B not in _FRAMES:
        a, b = RS.make_images(B, H0, W0, 81)
        c, d = RS.make_images(B, H0, W0, 82)
        q = lambda x: (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        _FRAMES[B] = [q(a), q(b), q(0.5 * (b + c)), q(d)]
    return _FRAMES[B]


def as_float(u8, dev):
    """The reference's load_image on the CPU: [B,3,H,W] = u8.float() / 255, then to the device."""
    return (u8.permute(0, 3, 1, 2).float() / 255.0).contiguous().to(dev)


def by_hand(V, model, kind, prev, cur, flow_init, dev, mode="sintel"):
    """(flow_low, padded flow_up, padder) of model(pad(prev), pad(cur), flow_init) in the mode FlowPredictor runs."""
    padder = V.InputPadder((H0, W0), mode)
    with torch.no_grad():
        p0, p1 = padder.pad(as_float(prev, dev), as_float(cur, dev))
        if kind == "basic":
            low, up = model(p0, p1, iters=ITERS, flow_init=flow_init, test_mode=True)
        else:
            up = model(p0, p1, iters=ITERS, flow_init=flow_init, last_only=True)[-1]
            low = model.flow_low[-1]
    return low, up, padder


def within(tag, got, want, tol):
    bound = tol * float(want.abs().max())
    err = float((got - want).abs().max())
    print("%s: error %.3e, bound %.3e (max|flow| %.3e)" % (tag, err, bound, float(want.abs().max())))
    assert torch.isfinite(got).all() and err <= bound, tag
    return bound


# ---- encode_frame / refine ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("init", [False, True], ids=["cold", "flow_init"])
@pytest.mark.parametrize("alternate", [False, True], ids=["CorrBlock", "AlternateCorrBlock"])
@pytest.mark.parametrize("kind", ["small", "basic"])
def test_refine_of_two_encoded_frames_is_the_pair_forward(gpu_device, V, kind, alternate, init, N):
    model = make_model(kind, gpu_device, alternate)
    a, b = u8_frames(N)[:2]
    padder = V.InputPadder((H0, W0))
    flow_init = None
    if init:
        flow_init = (2.0 * torch.randn(N, 2, 17, 18, generator=torch.Generator().manual_seed(5))).to(gpu_device)
    with torch.no_grad():
        fa = model.encode_frame(V.frame_ingest(a.to(gpu_device), padder._pad))
        fb = model.encode_frame(V.frame_ingest(b.to(gpu_device), padder._pad))
        assert tuple(fa.fmap.shape) == (N, 128 if kind == "small" else 256, 17, 18)
        assert tuple(fa.net.shape) == (N, model.hidden_dim, 17, 18) and tuple(fa.inp.shape) == (N, model.context_dim, 17, 18)
        p0, p1 = padder.pad(as_float(a, gpu_device), as_float(b, gpu_device))
        want = model(p0, p1, iters=ITERS, flow_init=flow_init)
        got = model.refine(fa, fb, iters=ITERS, flow_init=flow_init)
        assert len(got) == len(want) == ITERS
        for i, (g, w) in enumerate(zip(got, want)):
            assert tuple(g.shape) == (N, 2, 136, 144)
            within("%s %s iteration %d" % (kind, "alt" if alternate else "corr", i), g, w, TOL[kind])
        if kind == "basic":
            low_w, up_w = model(p0, p1, iters=ITERS, flow_init=flow_init, test_mode=True)
            low_g, up_g = model.refine(fa, fb, iters=ITERS, flow_init=flow_init, test_mode=True)
            within("basic test_mode flow_up", up_g, up_w, TOL[kind])
            within("basic test_mode flow_low", low_g, low_w, TOL[kind])
        else:
            last_w = model(p0, p1, iters=ITERS, flow_init=flow_init, last_only=True)
            last_g = model.refine(fa, fb, iters=ITERS, flow_init=flow_init, last_only=True)
            assert len(last_g) == len(last_w) == 1
            within("small last_only", last_g[0], last_w[0], TOL[kind])


# ---- FlowStream -------------------------------------------------------------------------------------------------------------------------
class Calls:
    """Forward hooks on model.fnet and model.cnet: (name, batch of the first argument) per call."""

    def __init__(self, model):
        self.seen = []
        self.handles = [m.register_forward_hook(self._hook(name)) for name, m in (("fnet", model.fnet), ("cnet", model.cnet))]

    def _hook(self, name):
        def hook(module, args, output):
            x = args[0]
            self.seen.append((name, sum(t.shape[0] for t in x) if isinstance(x, (list, tuple)) else x.shape[0]))
        return hook

    def take(self):
        seen, self.seen = self.seen, []
        return sorted(seen)

    def remove(self):
        for h in self.handles:
            h.remove()


def check_frame(V, r, B, bgr=False):
    assert tuple(r.flow_low.shape) == (B, 2, 17, 18) and tuple(r.flow_up.shape) == (B, 2, H0, W0)
    assert r.image.dtype == torch.uint8 and tuple(r.image.shape) == (B, H0, W0, 3)
    assert torch.equal(r.image, V.flow_to_image(r.flow_up, convert_to_bgr=bgr))
    assert torch.isfinite(r.flow_up).all() and not r.flow_up.requires_grad


@pytest.mark.parametrize("kind,B,mode", [("small", 1, "sintel"), ("basic", 2, "kitti")])
def test_stream_over_four_frames(gpu_device, V, kind, B, mode):
    """Each returned pair against the hand-composed model(pad(prev), pad(cur), flow_init = the stream's OWN kept flow before that
    push); what is kept and coloured bit for bit; one fnet and one cnet call per pushed frame, with batch B."""
    model = make_model(kind, gpu_device)
    frames = u8_frames(B)
    stream = V.FlowStream(model, iters=ITERS, pad_mode=mode, graph=False)
    calls = Calls(model)
    try:
        assert stream.push(frames[0].to(gpu_device)) is None and stream.flow_init is None
        assert calls.take() == [("cnet", B), ("fnet", B)]
        results, kept_before = [], []
        for cur in frames[1:]:
            kept_before.append(None if stream.flow_init is None else stream.flow_init.clone())
            r = stream.push(cur.to(gpu_device))
            assert calls.take() == [("cnet", B), ("fnet", B)]             # the pair path encodes 2 B images in fnet per call
            check_frame(V, r, B)
            assert torch.equal(bits(stream.flow_init), bits(V.forward_interpolate(r.flow_low)))
            results.append(r)
    finally:
        calls.remove()
    assert kept_before[0] is None and kept_before[1] is not None
    for i, r in enumerate(results):
        low, up, padder = by_hand(V, model, kind, frames[i], frames[i + 1], kept_before[i], gpu_device, mode)
        bound = within("%s pair %d flow_up" % (kind, i), r.flow_up, padder.unpad(up), TOL[kind])
        within("%s pair %d flow_low" % (kind, i), r.flow_low, low, TOL[kind])
        assert r.flow_up.stride() == padder.unpad(up).stride()
        if i == 1:
            _, cold, _ = by_hand(V, model, kind, frames[1], frames[2], None, gpu_device, mode)
            diff = float((r.flow_up - padder.unpad(cold)).abs().max())
            print("%s pair 1 vs a cold start: %.3e (bound %.3e)" % (kind, diff, bound))
            assert diff > bound                                            # the kept flow was used


def test_stream_reset_options_and_errors(gpu_device, V):
    from deep_visual_slam_amd._lib import DvsError
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    stream = V.FlowStream(model, iters=ITERS, graph=False)
    assert stream.push(f[0]) is None
    r1 = stream.push(f[1])
    # a shape or device change inside a sequence raises; reset() starts a new one: its first push returns None, its first pair is cold
    with pytest.raises(DvsError, match="call reset"):
        stream.push(f[2][:, :, :136].contiguous())
    stream.reset()
    assert stream.flow_init is None
    assert stream.push(f[0][:, :, :136].contiguous()) is None
    assert tuple(stream.push(f[1][:, :, :136].contiguous()).flow_up.shape) == (1, 2, H0, 136)
    stream.reset()
    assert stream.push(f[0][0]) is None                                   # the [H,W,3] form
    again = stream.push(f[1][0])
    same = lambda tag, r: within(tag, r.flow_up, r1.flow_up, TOL["small"])    # two runs: the split-K convolutions add with atomics
    same("after reset()", again)
    # without warm start nothing is kept; without image nothing is coloured
    plain = V.FlowStream(model, iters=ITERS, warm_start=False, image=False, graph=False)
    assert plain.push(f[0]) is None
    r = plain.push(f[1])
    assert plain.flow_init is None and r.image is None
    same("warm_start=False, image=False", r)
    # convert_to_bgr reverses the picture's channels; bgr=True says the FRAMES are BGR: the reversed frames give the same flow
    pic = V.FlowStream(model, iters=ITERS, convert_to_bgr=True, graph=False)
    pic.push(f[0])
    check_frame(V, pic.push(f[1]), 1, bgr=True)
    rev = V.FlowStream(model, iters=ITERS, bgr=True, graph=False)
    assert rev.push(f[0].flip(-1)) is None                                # flip(-1) is a copy: dense BGR frames
    same("bgr=True on reversed frames", rev.push(f[1].flip(-1)))
    # kitti padding: all of the height's padding at the bottom
    kitti = V.FlowStream(model, iters=ITERS, pad_mode="kitti", graph=False)
    kitti.push(f[0])
    rk = kitti.push(f[1])
    _, up, padder = by_hand(V, model, "small", u8_frames(1)[0], u8_frames(1)[1], None, gpu_device, "kitti")
    assert padder._pad == [1, 2, 0, 6]
    within("kitti", rk.flow_up, padder.unpad(up), TOL["small"])
    # a host frame is copied to the model's device
    hosted = V.FlowStream(model, iters=ITERS, graph=False)
    assert stream.frame_copied is None                                    # device frames: no copy to wait for
    hosted.push(u8_frames(1)[0].pin_memory())
    hosted.frame_copied.synchronize()                                     # from here on the caller may reuse its pinned buffer
    same("host frames", hosted.push(u8_frames(1)[1]))
    # a padded size the model refuses keeps the model's own error; a model in train() mode is refused
    with pytest.raises(DvsError, match="at least 128x128"):
        V.FlowStream(model, iters=ITERS, graph=False).push(f[0][:, :100])
    with pytest.raises(DvsError, match="uint8 only"):
        V.FlowStream(model, iters=ITERS, graph=False).push(f[0].float())
    model.train()
    try:
        with pytest.raises(DvsError, match=r"train\(\) mode"):
            V.FlowStream(model, iters=ITERS, graph=False).push(f[0])
    finally:
        model.eval()


# ---- graph=True ----------------------------------------------------------------------------------------------------------------------
def run_stream(stream, frames):
    """Clones of (flow_low, flow_up, image) of every pair: a graph's outputs are valid until the next push only."""
    out = []
    for x in frames:
        r = stream.push(x)
        if r is not None:
            out.append((r.flow_low.clone(), r.flow_up.clone(), r.image.clone()))
    return out


@pytest.fixture
def deterministic():
    """dvs_set_deterministic(1) for one test.  By default the forward's split-K convolutions add with float atomics
    (csrc/conv_fwd.hip, conv_wino.hip), so two runs of the SAME launches differ in the last bits, and along a sequence the warm
    start -- a nearest-source choice -- may turn such a difference into another source.  Comparisons that chain two streams over
    several frames, and the bit-for-bit ones, are therefore made in the mode in which a forward repeats exactly; the bound is the same."""
    from deep_visual_slam_amd import _lib
    before = _lib.deterministic()
    _lib.set_deterministic(True)
    try:
        yield
    finally:
        _lib.set_deterministic(before)


@pytest.mark.parametrize("kind", ["small", "basic"])
def test_graph_stream_against_the_pair_forward(gpu_device, V, kind):
    """The default mode: every replayed pair against the hand-composed model(pad(prev), pad(cur), flow_init = the graph stream's
    OWN kept flow before that push), as test_stream_over_four_frames judges the eager stream; nothing is chained."""
    model = make_model(kind, gpu_device)
    frames = u8_frames(1)
    graphed = V.FlowStream(model, iters=ITERS, graph=True)
    assert graphed.push(frames[0].to(gpu_device)) is None and graphed.graph is not None and not graphed.stale()
    assert not graphed.flow_init.any()                                     # the cold start is a zeroed buffer
    for i, cur in enumerate(frames[1:]):
        kept = graphed.flow_init.clone()
        r = graphed.push(cur.to(gpu_device))
        check_frame(V, r, 1)
        assert torch.equal(bits(graphed.flow_init), bits(V.forward_interpolate(r.flow_low)))
        low, up, padder = by_hand(V, model, kind, frames[i], cur, kept, gpu_device)
        within("%s graph pair %d flow_up" % (kind, i), r.flow_up, padder.unpad(up), TOL[kind])
        within("%s graph pair %d flow_low" % (kind, i), r.flow_low, low, TOL[kind])
        assert r.flow_up.stride() == padder.unpad(up).stride()


@pytest.mark.parametrize("kind", ["small", "basic"])
def test_graph_stream(gpu_device, V, deterministic, kind):
    """The same four frames through the eager and the graph stream; reset(); a weight changed in place."""
    model = make_model(kind, gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    eager, graphed = V.FlowStream(model, iters=ITERS, graph=False), V.FlowStream(model, iters=ITERS, graph=True)
    assert graphed.push(f[0]) is None and eager.push(f[0]) is None
    want, got = run_stream(eager, f[1:]), run_stream(graphed, f[1:])
    assert len(want) == len(got) == 3 and not graphed.stale()
    differing = lambda a, g: [name for name, x, y in zip(("flow_low", "flow_up", "image"), a, g)
                              if not torch.equal(x.view(torch.uint8) if x.dtype == torch.uint8 else bits(x),
                                                 y.view(torch.uint8) if y.dtype == torch.uint8 else bits(y))]
    same = lambda a, g: not differing(a, g)
    for i, (w, g) in enumerate(zip(want, got)):
        within("%s graph vs eager pair %d flow_up" % (kind, i), g[1], w[1], TOL[kind])
        within("%s graph vs eager pair %d flow_low" % (kind, i), g[0], w[0], TOL[kind])
        assert torch.equal(g[2], V.flow_to_image(g[1]))
    print("%s: graph replay bit-equal to the eager stream: %s" % (kind, all(same(w, g) for w, g in zip(want, got))))
    assert torch.equal(bits(graphed.flow_init), bits(V.forward_interpolate(got[-1][0])))
    # reset() and the same frames: replay against replay, bit for bit, without a new capture
    captured = graphed.graph
    graphed.reset()
    assert not graphed.flow_init.any()
    assert graphed.push(f[0]) is None
    again = run_stream(graphed, f[1:])
    assert graphed.graph is captured
    assert len(again) == 3 and [differing(a, g) for a, g in zip(again, got)] == [[], [], []]
    # a weight changed in place: stale(), and the next push matches the eager stream on the new weights
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
        within("%s after the weight change flow_up" % kind, g.flow_up, w.flow_up, TOL[kind])
        moved = float((g.flow_up - got[1][1]).abs().max())
        print("%s: the new weights move the flow by %.3e" % (kind, moved))
        assert moved > TOL[kind] * float(w.flow_up.abs().max())
    finally:
        with torch.no_grad():
            weight.copy_(saved)


# ---- host=True -----------------------------------------------------------------------------------------------------------------------
def test_host_copies_alternate_between_two_pinned_buffers(gpu_device, V):
    model = make_model("small", gpu_device)
    f = [x.to(gpu_device) for x in u8_frames(1)]
    stream = V.FlowStream(model, iters=ITERS, host=True, graph=False)
    assert stream.push(f[0]) is None
    r1 = stream.push(f[1])
    image1, low1 = r1.image.cpu().numpy(), r1.flow_low.cpu().numpy()
    r2 = stream.push(f[2])
    assert r1._slot is not r2._slot and r1._slot["image"].is_pinned() and r2._slot["flow_low"].is_pinned()
    assert np.array_equal(r2.image_host, r2.image.cpu().numpy()) and np.array_equal(r2.flow_low_host, r2.flow_low.cpu().numpy())
    assert np.array_equal(r1.image_host, image1) and np.array_equal(r1.flow_low_host, low1)      # valid until the push after next
    assert r1.image_host.dtype == np.uint8 and r1.image_host.shape == (1, H0, W0, 3)
    assert not np.array_equal(r1.image_host, r2.image_host)
    r3 = stream.push(f[3])
    assert r3._slot is r1._slot and np.array_equal(r3.image_host, r3.image.cpu().numpy())
