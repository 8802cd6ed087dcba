"""CPU-side checks of the video stage (csrc/flowstage.hip, raft_video.py): the NumPy restatements of tests/flowstage_ref.py equal
what the reference's own functions returned (tests/golden/flowstage.npz), InputPadder pads as the reference does, the three new
entry points refuse bad arguments on the host before any launch, the ABI is still 12, and raft_video's input errors."""
import numpy as np
import pytest
import torch

import flowstage_ref as R
from conftest import load_golden

FIXTURE = "flowstage.npz"


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


# ---- restatements against the reference's recorded results --------------------------------------------------------------------
@pytest.mark.parametrize("h,w", R.FI_SHAPES, ids=["%dx%d" % s for s in R.FI_SHAPES])
def test_forward_interpolate_restatement_equals_the_reference(rec, h, w):
    k = R.fi_key(h, w)
    flows = rec[k + "/flow"]
    assert np.array_equal(flows, R.fi_inputs(h, w))
    for n, name in enumerate(R.FI_IMAGES):
        out, margin, nvalid = R.forward_interpolate(flows[n])
        assert out.dtype == np.float32 and np.array_equal(out, rec[k + "/out"][n]), name
        assert nvalid == int(rec[k + "/valid"][n]) and float(margin.min()) == float(rec[k + "/margin"][n])
        assert float(margin.min()) >= 1e-9
    assert int(rec[k + "/valid"][2]) == 0 and not rec[k + "/out"][2].any()
    assert int(rec[k + "/valid"][1]) == min(6, int(rec[k + "/valid"][0]))


def fv_cases(rec):
    """(name, flow [2,H,W], clip_flow, bgr, reference image) of every colouring case of the fixture."""
    for H, W in R.FV_SIZES:
        k = R.fv_key(H, W)
        for n in range(3):
            yield "%s[%d]" % (k, n), rec[k + "/flow"][n], None, False, rec[k + "/image"][n]
    for name in R.FV_BIG_NAMES:
        yield "big/" + name, rec["fv/big/" + name], None, False, rec["fv/big/%s_image" % name]
    for name in R.FV_SPECIAL_NAMES:
        _, clip, bgr = R.fv_special(name)
        yield name, rec["fv/%s/flow" % name], clip, bgr, rec["fv/%s/image" % name]


def test_flow_to_image_restatement_equals_the_reference(rec):
    count = 0
    for name, flow, clip, bgr, image in fv_cases(rec):
        got = R.flow_to_image(flow, clip, bgr)
        assert got.dtype == np.uint8 and got.shape == flow.shape[1:] + (3,) and np.array_equal(got, image), name
        count += 1
    assert count == 3 * len(R.FV_SIZES) + len(R.FV_BIG_NAMES) + len(R.FV_SPECIAL_NAMES)
    assert (rec["fv/zero/image"] == 255).all()
    assert float(rec["fv/exempt"].max()) <= R.MAX_EXEMPT


def test_fixture_inputs_are_the_seeded_ones(rec):
    for H, W in R.FV_SIZES:
        assert np.array_equal(rec[R.fv_key(H, W) + "/flow"], R.fv_noise(H, W))
    for name in R.FV_SPECIAL_NAMES:
        assert np.array_equal(rec["fv/%s/flow" % name], R.fv_special(name)[0])
    assert np.array_equal(rec["fv/big/large"], R.fv_big("large"))


def test_colorwheel_from_segment_lengths():
    w = R.make_colorwheel()
    assert w.shape == (55, 3) and w.min() == 0 and w.max() == 255 and np.array_equal(w, np.floor(w))
    assert w[0].tolist() == [255, 0, 0] and w[15].tolist() == [255, 255, 0] and w[21].tolist() == [0, 255, 0]
    assert w[25].tolist() == [0, 255, 255] and w[36].tolist() == [0, 0, 255] and w[49].tolist() == [255, 0, 255]
    assert w[54].tolist() == [255, 0, 43]


# ---- InputPadder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sintel", "kitti"])
@pytest.mark.parametrize("H,W,Hp,Wp", [(130, 141, 136, 144), (436, 1024, 440, 1024)])
def test_input_padder_pads_and_unpads(rec, H, W, Hp, Wp, mode):
    from deep_visual_slam_amd import raft_video
    k = "pad/%dx%d/%s" % (H, W, mode)
    want = [int(v) for v in rec[k + "/pad"]]
    padder = raft_video.InputPadder((1, 3, H, W), mode)
    assert list(padder._pad) == want == list(R.InputPadder((1, 3, H, W), mode)._pad)
    x = torch.arange(H * W, dtype=torch.float32).reshape(1, 1, H, W)
    y = torch.flip(x, dims=(-1,))
    px, py = padder.pad(x, y)
    assert tuple(px.shape) == tuple(py.shape) == (1, 1, Hp, Wp)
    ux = padder.unpad(px)
    assert torch.equal(ux, x) and torch.equal(padder.unpad(py), y)
    assert ux.data_ptr() == px.data_ptr() + 4 * (want[2] * Wp + want[0])                 # a view, not a copy
    (mine,) = R.InputPadder((1, 3, H, W), mode).pad(x.numpy())
    assert np.array_equal(px.numpy(), mine)
    if k + "/padded" in rec:
        assert np.array_equal(px.numpy().astype(np.int16), rec[k + "/padded"])
        assert np.array_equal(ux.numpy().astype(np.int16), rec[k + "/unpadded"])


# ---- argument checks of the new entries, on a machine without a GPU -----------------------------------------------------------
P = 4096          # a non-NULL, 16-byte aligned "device pointer": nothing dereferences it before the checks fail


def _interp(l, flow=P, out=2 * P, N=1, h=5, w=7):
    return l.dvs_forward_interp(flow, out, N, h, w, None)


def _radmax(l, flow=P, plane=35, row=7, N=1, H=5, W=7, clip=-1.0, radmax=2 * P):
    return l.dvs_flow_radmax(flow, plane, row, N, H, W, clip, radmax, None)


def _image(l, flow=P, plane=35, row=7, radmax=2 * P, out=3 * P, N=1, H=5, W=7, clip=-1.0, bgr=0):
    return l.dvs_flow_to_image(flow, plane, row, radmax, out, N, H, W, clip, bgr, None)


BAD_CALLS = [
    ("interp: NULL flow", _interp, dict(flow=None)),
    ("interp: NULL out", _interp, dict(out=None)),
    ("interp: misaligned", _interp, dict(flow=P + 2)),
    ("interp: in place", _interp, dict(out=P)),
    ("interp: P = 0 (h)", _interp, dict(h=0)),
    ("interp: P = 0 (w)", _interp, dict(w=0)),
    ("interp: P = 65537", _interp, dict(h=1, w=65537)),
    ("interp: P = 2^32 + 1 as ints", _interp, dict(h=65537, w=65537)),
    ("interp: N = 0", _interp, dict(N=0)),
    ("interp: N = -1", _interp, dict(N=-1)),
    ("radmax: NULL flow", _radmax, dict(flow=None)),
    ("radmax: NULL radmax", _radmax, dict(radmax=None)),
    ("radmax: row stride < W", _radmax, dict(row=6)),
    ("radmax: plane stride < the image", _radmax, dict(plane=34)),
    ("radmax: N = 0", _radmax, dict(N=0)),
    ("radmax: H = 0", _radmax, dict(H=0, plane=7)),
    ("radmax: W = 0", _radmax, dict(W=0)),
    ("radmax: 2^31 pixels", _radmax, dict(N=2, H=32768, W=32768, row=32768, plane=1 << 30)),
    ("radmax: NaN clip", _radmax, dict(clip=float("nan"))),
    ("image: NULL flow", _image, dict(flow=None)),
    ("image: NULL radmax", _image, dict(radmax=None)),
    ("image: NULL out", _image, dict(out=None)),
    ("image: misaligned out", _image, dict(out=3 * P + 4)),
    ("image: row stride < W", _image, dict(row=6)),
    ("image: plane stride < the image", _image, dict(plane=34)),
    ("image: N = 0", _image, dict(N=0)),
    ("image: N = -3", _image, dict(N=-3)),
    ("image: bgr = 2", _image, dict(bgr=2)),
]
ENTRY = {_interp: b"dvs_forward_interp", _radmax: b"dvs_flow_radmax", _image: b"dvs_flow_to_image"}


@pytest.mark.parametrize("name,call,kw", BAD_CALLS, ids=[b[0] for b in BAD_CALLS])
def test_new_entries_refuse_bad_arguments(built, name, call, kw):
    l = built.lib()
    assert call(l, **kw) == -1                       # DVS_ERR_INVALID: no launch was tried (this machine has no GPU to refuse one)
    assert ENTRY[call] in l.dvs_last_error()


def test_messages_say_what_is_wrong(built):
    l = built.lib()
    assert _interp(l, h=1, w=65537) < 0 and b"65537 exceeds 65536" in l.dvs_last_error()
    assert _radmax(l, row=6) < 0 and b"row stride 6 is below W=7" in l.dvs_last_error()
    assert _image(l, plane=34) < 0 and b"plane stride 34" in l.dvs_last_error()


def test_abi_is_still_12(built):
    assert built.ABI_VERSION == 12 and built.lib().dvs_abi_version() == 12
    for name in ("dvs_forward_interp", "dvs_flow_radmax", "dvs_flow_to_image"):
        assert name in built.exported_symbols() and hasattr(built.lib(), name)


# ---- raft_video's input errors ----------------------------------------------------------------------------------------------
def test_raft_video_input_errors(built):
    from deep_visual_slam_amd import raft, raft_video
    E = built.DvsError
    for fn in (raft_video.forward_interpolate, raft_video.flow_to_image):
        with pytest.raises(E, match="GPU tensors only .* no CPU path"):
            fn(torch.zeros(2, 5, 7))
        with pytest.raises(E, match="GPU tensors only"):
            fn(np.zeros((2, 5, 7), np.float32))
    meta = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="meta")
    with pytest.raises(E, match="GPU tensors only"):
        raft_video.forward_interpolate(meta(2, 5, 7))
    with pytest.raises(E, match="model must be a raft.RAFT or a raft.SmallRAFT"):
        raft_video.FlowPredictor(torch.nn.Identity())
    model = raft.SmallRAFT()
    with pytest.raises(E, match="iters=0"):
        raft_video.FlowPredictor(model, iters=0)
    pred = raft_video.FlowPredictor(model.eval(), iters=2)
    with pytest.raises(E, match="image1: GPU tensors only .* no CPU path"):
        pred(torch.zeros(1, 3, 130, 141), torch.zeros(1, 3, 130, 141))
    model.train()
    with pytest.raises(E, match=r"train\(\) mode"):
        pred(torch.zeros(1, 3, 130, 141), torch.zeros(1, 3, 130, 141))


class _FakeCuda:
    """Stands in for a GPU tensor as far as raft_video's checks look before they touch the device."""

    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.dtype, self.is_cuda, self.device = torch.Size(shape), dtype, True, "cuda:0"

    def dim(self):
        return len(self.shape)


def test_raft_video_dtype_and_rank_errors(built, monkeypatch):
    from deep_visual_slam_amd import raft_video
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _FakeCuda)))
    E = built.DvsError
    for fn in (raft_video.forward_interpolate, raft_video.flow_to_image):
        with pytest.raises(E, match="fp32 only, got torch.float16"):
            fn(_FakeCuda((2, 5, 7), torch.float16))
        with pytest.raises(E, match="fp32 only, got torch.float64"):
            fn(_FakeCuda((1, 2, 5, 7), torch.float64))
        for shape in ((5, 7), (3, 5, 7), (1, 3, 5, 7), (1, 1, 2, 5, 7), (2, 0, 7)):
            with pytest.raises(E, match="expected, got"):
                fn(_FakeCuda(shape))
