"""The video stage on the GPU (csrc/flowstage.hip, raft_video.py) against tests/golden/flowstage.npz, which holds what the
reference's own forward_interpolate and flow_to_image returned (tests/golden/make_golden_flowstage.py).

forward_interp: EXACTLY the fixture.  Every case's smallest relative margin between the best and the second-best squared distance
is recorded (>= 2e-5 here, the generator refuses < 1e-9), so no rounding and no tie rule can explain a difference.

flow_to_image: atan2f is the one operation of the ladder that is correctly rounded on neither side.  NumPy's fp32 arctan2 stays
below 4 ulp and the device's is taken as <= 2 ulp, so |d fk| <= 27 * 6 * ulp(pi) / pi + 2 ulp(54) ~ 2e-5; the restatement
re-evaluates every byte with fk -+ 3e-5 and rad * (1 -+ 4 * 2^-23).  A byte on which all nine variants agree must match exactly,
the others (at most 0.5 % of a case, the generator refuses more) may differ by 1.  radmax is bit-equal to the restatement's.
Measured on the MI355X: see DESIGN.md section 21.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import flowstage_ref as R
import raft_basic_ref as RB
import raft_ref as RS
from conftest import load_golden

pytestmark = pytest.mark.gpu
FIXTURE = "flowstage.npz"


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


# ---- forward_interp ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("h,w", R.FI_SHAPES, ids=["%dx%d" % s for s in R.FI_SHAPES])
def test_forward_interp_equals_the_reference_exactly(gpu_device, rec, V, h, w, N):
    k = R.fi_key(h, w)
    flow = torch.from_numpy(rec[k + "/flow"][:N]).to(gpu_device)
    got = V.forward_interpolate(flow)
    assert got.shape == flow.shape and got.dtype == torch.float32 and got.is_cuda
    want = torch.from_numpy(rec[k + "/out"][:N])
    wrong = int((bits(got) != bits(want)).sum())
    print("%s N=%d: %d of %d elements differ; valid sources %s, smallest margin %.2e"
          % (k, N, wrong, want.numel(), rec[k + "/valid"][:N].tolist(), float(rec[k + "/margin"][:N].min())))
    assert wrong == 0
    if N == 3:
        assert not got[2].any()                                          # no valid source: zeros


def test_forward_interp_single_image_form(gpu_device, rec, V):
    k = R.fi_key(5, 7)
    got = V.forward_interpolate(torch.from_numpy(rec[k + "/flow"][0]).to(gpu_device))
    assert tuple(got.shape) == (2, 5, 7) and torch.equal(got.cpu(), torch.from_numpy(rec[k + "/out"][0]))


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (16, 17), (25, 41)])
def test_forward_interp_zero_flow_returns_zeros(gpu_device, V, h, w):
    """Every source stays on its own pixel; those of row 0 and column 0 are invalid (0 < x1 is strict), the rest are nearest to
    themselves; whatever a pixel takes is a zero flow."""
    got = V.forward_interpolate(torch.zeros(3, 2, h, w, device=gpu_device))
    assert (bits(got) == 0).all()


def test_forward_interp_lowest_index_wins_a_tie(gpu_device, V):
    """The package's own rule where the reference defines none: two sources land on the same point; the lower index is taken."""
    flow = torch.full((1, 2, 3, 70), -1e4)
    flow[0, :, 1, 5] = torch.tensor([20.25, 0.5])       # source 75 -> (25.25, 1.5)
    flow[0, :, 2, 69] = torch.tensor([-43.75, -0.5])    # source 209 -> (25.25, 1.5): the same point, a different flow
    got = V.forward_interpolate(flow.to(gpu_device)).cpu()
    assert torch.equal(got[0, 0], torch.full((3, 70), 20.25)) and torch.equal(got[0, 1], torch.full((3, 70), 0.5))
    flow[0, :, 0, 3] = torch.tensor([22.25, 1.5])       # source 3 -> the same point again, in another wave's share and lower still
    got = V.forward_interpolate(flow.to(gpu_device)).cpu()
    assert torch.equal(got[0, 0], torch.full((3, 70), 22.25)) and torch.equal(got[0, 1], torch.full((3, 70), 1.5))


def test_forward_interp_batch_neighbours_and_repeats(gpu_device, rec, V):
    """An image's result does not depend on its batch neighbours, and two runs give the same bits."""
    for h, w in ((16, 17), (25, 41), (55, 128)):
        flows = torch.from_numpy(rec[R.fi_key(h, w) + "/flow"]).to(gpu_device)
        a = V.forward_interpolate(flows)
        b = V.forward_interpolate(flows)
        assert torch.equal(bits(a), bits(b))
        rev = V.forward_interpolate(flows.flip(0).contiguous()).flip(0)
        assert torch.equal(bits(a), bits(rev))
        for n in range(3):
            assert torch.equal(bits(a[n]), bits(V.forward_interpolate(flows[n])))


def test_forward_interp_refuses_more_than_65536_points(gpu_device, V):
    from deep_visual_slam_amd._lib import DvsError
    with pytest.raises(DvsError, match="exceeds 65536"):
        V.forward_interpolate(torch.zeros(2, 257, 256, device=gpu_device))
    assert tuple(V.forward_interpolate(torch.zeros(2, 256, 256, device=gpu_device)).shape) == (2, 256, 256)


# ---- flow_to_image ----------------------------------------------------------------------------------------------------------
_REFS = {}


def colour_ref(key, flows, clip, bgr):
    """(images, exempt masks) of the restatement for a batch [N,2,H,W]: computed once per case, shared, never modified."""
    if key not in _REFS:
        res = [R.flow_to_image(f, clip, bgr, with_exempt=True) for f in flows]
        _REFS[key] = (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]))
    return _REFS[key]


def check_bytes(tag, got, flows, clip, bgr, fixture):
    """The byte rule of the module docstring, for a batch; prints the figures before it asserts."""
    img, exempt = colour_ref(tag, flows, clip, bgr)
    assert np.array_equal(img, fixture), tag                             # the restatement IS the reference on this case
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == img.shape, (tag, got.dtype, got.shape)
    diff = np.abs(got.astype(np.int32) - img.astype(np.int32))
    print("%s: %d of %d bytes differ (largest difference %d), %d of them on bytes where all variants agree; exempt share %.4f %%"
          % (tag, int((diff > 0).sum()), diff.size, int(diff.max()), int((diff > 0)[~exempt].sum()), 100 * exempt.mean()))
    assert exempt.mean() <= R.MAX_EXEMPT, tag
    assert not diff[~exempt].any(), tag
    assert diff.max() <= 1, tag


def strided_view(flows, dev, top=2, left=1, bottom=3, right=2):
    """`flows` [N,2,H,W] as the window of a larger contiguous tensor filled with NaN: what InputPadder.unpad hands over."""
    N, _, H, W = flows.shape
    big = torch.full((N, 2, H + top + bottom, W + left + right), float("nan"), device=dev)
    view = big[:, :, top:top + H, left:left + W]
    view.copy_(flows)
    assert not view.is_contiguous() or (H == 1 and W == 1 and N == 1)
    return view


def radmax_of(flow, clip=None):
    """dvs_flow_radmax on a dense [N,2,H,W] tensor."""
    from deep_visual_slam_amd import _lib
    N, _, H, W = flow.shape
    out = torch.full((N,), float("nan"), device=flow.device)
    _lib.check(_lib.lib().dvs_flow_radmax(flow.data_ptr(), H * W, W, N, H, W, -1.0 if clip is None else clip, out.data_ptr(),
                                         _lib.stream()), "dvs_flow_radmax")
    return out


@pytest.mark.parametrize("H,W", R.FV_SIZES, ids=["%dx%d" % s for s in R.FV_SIZES])
def test_flow_to_image_noise(gpu_device, rec, V, H, W):
    """N = 3 with three different maxima, N = 1, the [2,H,W] form, and the same flows as a strided view."""
    k = R.fv_key(H, W)
    flows, fixture = rec[k + "/flow"], rec[k + "/image"]
    dense = torch.from_numpy(flows).to(gpu_device)
    got = V.flow_to_image(dense)
    check_bytes(k, got, flows, None, False, fixture)
    want_max = torch.from_numpy(np.array([R.flow_radius(f)[2] for f in flows]))
    assert torch.equal(bits(radmax_of(dense)), bits(want_max))
    assert len({float(m) for m in want_max}) == 3
    assert torch.equal(V.flow_to_image(dense[:1]), got[:1]) and torch.equal(V.flow_to_image(dense[1]), got[1])
    view = strided_view(dense, gpu_device)
    assert torch.equal(V.flow_to_image(view), got) and torch.equal(V.flow_to_image(view[2]), got[2])


@pytest.mark.parametrize("name", R.FV_BIG_NAMES)
def test_flow_to_image_131x77(gpu_device, rec, V, name):
    flow = rec["fv/big/" + name]
    dense = torch.from_numpy(flow).to(gpu_device)
    got = V.flow_to_image(dense)
    check_bytes("fv/big/" + name, got[None], flow[None], None, False, rec["fv/big/%s_image" % name][None])
    assert torch.equal(bits(radmax_of(dense[None])), bits(torch.from_numpy(np.array([R.flow_radius(flow)[2]]))))
    assert torch.equal(V.flow_to_image(strided_view(dense[None], gpu_device))[0], got)


@pytest.mark.parametrize("name", R.FV_SPECIAL_NAMES)
def test_flow_to_image_special_cases(gpu_device, rec, V, name):
    """Zero flow (every byte 255), a single non-zero pixel, clip_flow = 4 (clipped to 0 .. 4, as the reference does), BGR."""
    flow, clip, bgr = R.fv_special(name)
    assert np.array_equal(flow, rec["fv/%s/flow" % name])
    dense = torch.from_numpy(flow).to(gpu_device)
    got = V.flow_to_image(dense, clip_flow=clip, convert_to_bgr=bgr)
    check_bytes("fv/" + name, got[None], flow[None], clip, bgr, rec["fv/%s/image" % name][None])
    assert torch.equal(bits(radmax_of(dense[None], clip)), bits(torch.from_numpy(np.array([R.flow_radius(flow, clip)[2]]))))
    if name == "zero":
        assert (got == 255).all()
    if name == "bgr":
        assert torch.equal(got.flip(-1), V.flow_to_image(dense))
    assert torch.equal(V.flow_to_image(strided_view(dense[None], gpu_device), clip_flow=clip, convert_to_bgr=bgr)[0], got)


def test_flow_to_image_batch_neighbours_and_repeats(gpu_device, rec, V):
    flows = torch.from_numpy(rec[R.fv_key(7, 131) + "/flow"]).to(gpu_device)
    a, b = V.flow_to_image(flows), V.flow_to_image(flows)
    assert torch.equal(a, b) and torch.equal(V.flow_to_image(flows.flip(0).contiguous()).flip(0), a)


# ---- FlowPredictor ----------------------------------------------------------------------------------------------------------
H0, W0 = 130, 141          # pads to 136 x 144


def make_model(kind, dev):
    from deep_visual_slam_amd import raft
    if kind == "small":
        model = raft.SmallRAFT(SimpleNamespace(alternate_corr=False))
        model.load_state_dict(RS.make_weights(RS.G6["weight_seed"]), strict=True)
    else:
        model = raft.RAFT(SimpleNamespace(small=False, alternate_corr=False))
        model.load_state_dict(RB.make_weights(RB.G6["weight_seed"]), strict=True)
    return model.to(dev).eval()


def frames(dev, B=1):
    a, b = RS.make_images(B, H0, W0, 81)
    c, _ = RS.make_images(B, H0, W0, 82)
    return a.to(dev), b.to(dev), (0.5 * (b + c)).to(dev)


def check_record(V, r, B):
    assert tuple(r.flow_low.shape) == (B, 2, 17, 18) and tuple(r.flow_up.shape) == (B, 2, H0, W0)
    assert r.image.dtype == torch.uint8 and tuple(r.image.shape) == (B, H0, W0, 3)
    assert torch.equal(r.image, V.flow_to_image(r.flow_up))
    assert torch.isfinite(r.flow_up).all() and not r.flow_up.requires_grad


def test_predictor_with_small_raft(gpu_device, V):
    """Two consecutive pairs at 130x141, iters=2: what is kept, what is returned, and the second call against the hand-composed
    model(pad(..), flow_init=..) within the RAFT tests' OUT_TOL * max|flow| (the tolerance of tests/test_raft_gpu.py, reused)."""
    from deep_visual_slam_amd._lib import DvsError
    model = make_model("small", gpu_device)
    f0, f1, f2 = frames(gpu_device)
    pred = V.FlowPredictor(model, iters=2)
    padder = V.InputPadder(f0.shape)
    r1 = pred(f0, f1)
    check_record(V, r1, 1)
    assert torch.equal(bits(pred.flow_init), bits(V.forward_interpolate(r1.flow_low)))
    kept = pred.flow_init.clone()
    with torch.no_grad():
        p0, p1 = padder.pad(f0, f1)
        by_hand = model(p0, p1, iters=2, last_only=True)[-1]
    assert tuple(by_hand.shape) == (1, 2, 136, 144)
    assert r1.flow_up.stride() == padder.unpad(by_hand).stride() == (2 * 136 * 144, 136 * 144, 144, 1)      # the un-padded window
    tol = RS.OUT_TOL * float(by_hand.abs().max())
    err = float((r1.flow_up - padder.unpad(by_hand)).abs().max())
    print("first call vs by hand: %.3e (tolerance %.3e)" % (err, tol))
    assert err <= tol
    r2 = pred(f1, f2)
    check_record(V, r2, 1)
    assert torch.equal(bits(pred.flow_init), bits(V.forward_interpolate(r2.flow_low)))
    with torch.no_grad():
        p1, p2 = padder.pad(f1, f2)
        warm = model(p1, p2, iters=2, flow_init=kept, last_only=True)[-1]
        cold = model(p1, p2, iters=2, last_only=True)[-1]
    tol = RS.OUT_TOL * float(warm.abs().max())
    err = float((r2.flow_up - padder.unpad(warm)).abs().max())
    print("second call vs by hand with flow_init: %.3e (tolerance %.3e); vs a cold start: %.3e"
          % (err, tol, float((r2.flow_up - padder.unpad(cold)).abs().max())))
    assert err <= tol
    assert float((r2.flow_up - padder.unpad(cold)).abs().max()) > tol                   # the kept flow was used
    # a shape change inside a sequence raises; reset() starts a new one and drops the kept flow
    g0, g1 = f0[:, :, :, :136].contiguous(), f1[:, :, :, :136].contiguous()
    with pytest.raises(DvsError, match="call reset"):
        pred(g0, g1)
    pred.reset()
    assert pred.flow_init is None
    r3 = pred(g0, g1)
    assert tuple(r3.flow_up.shape) == (1, 2, H0, 136)
    pred.reset()
    r4 = pred(f1, f2)
    assert float((r4.flow_up - padder.unpad(cold)).abs().max()) <= tol
    # without warm start nothing is kept; without image nothing is coloured; BGR reverses the channels
    plain = V.FlowPredictor(model, iters=2, warm_start=False, image=False)
    r5 = plain(f1, f2)
    assert plain.flow_init is None and r5.image is None
    bgr = V.FlowPredictor(model, iters=2, convert_to_bgr=True)(f1, f2)
    assert torch.equal(bgr.image, V.flow_to_image(bgr.flow_up, convert_to_bgr=True))
    # a padded size the model refuses keeps the model's own error; a model in train() mode is refused
    with pytest.raises(DvsError, match="at least 128x128"):
        V.FlowPredictor(model, iters=2)(f0[:, :, :100], f1[:, :, :100])
    model.train()
    with pytest.raises(DvsError, match=r"train\(\) mode"):
        V.FlowPredictor(model, iters=2)(f0, f1)


def test_predictor_with_raft(gpu_device, V):
    """The full-size model once, B = 2, kitti padding: test_mode's (flow_low, flow_up), the warm start, the colouring."""
    model = make_model("basic", gpu_device)
    f0, f1, f2 = frames(gpu_device, B=2)
    pred = V.FlowPredictor(model, iters=2, pad_mode="kitti")
    padder = V.InputPadder(f0.shape, "kitti")
    r1 = pred(f0, f1)
    check_record(V, r1, 2)
    kept = pred.flow_init.clone()
    assert torch.equal(bits(kept), bits(V.forward_interpolate(r1.flow_low)))
    r2 = pred(f1, f2)
    check_record(V, r2, 2)
    with torch.no_grad():
        p1, p2 = padder.pad(f1, f2)
        low, warm = model(p1, p2, iters=2, flow_init=kept, test_mode=True)
    tol = RB.OUT_TOL * float(warm.abs().max())
    err = float((r2.flow_up - padder.unpad(warm)).abs().max())
    print("RAFT second call vs by hand with flow_init: %.3e (tolerance %.3e)" % (err, tol))
    assert err <= tol and float((r2.flow_low - low).abs().max()) <= RB.OUT_TOL * float(low.abs().max())
    assert r2.flow_up.stride() == padder.unpad(warm).stride()
