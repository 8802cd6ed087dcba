"""CPU-side checks of the RAFT frame stream (csrc/ingest.hip, raft_video.FlowStream): the NumPy restatement of
tests/raftstream_ref.py equals what the reference's own chain returned (tests/golden/raftstream_ingest.npz) bit for bit, the
header declares dvs_frame_ingest and the binding lists it, the ABI is still 12, and every argument error of dvs_frame_ingest,
frame_ingest and FlowStream that can be raised without a device is raised."""
import os
import re

import numpy as np
import pytest
import torch

import raftstream_ref as R
from conftest import ROOT, load_golden

FIXTURE = "raftstream_ingest.npz"


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


# ---- the restatement against the reference's recorded results -------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("H,W", R.SIZES, ids=["%dx%d" % s for s in R.SIZES])
def test_restatement_equals_the_reference_bit_for_bit(rec, H, W, mode):
    frames = rec[R.frame_key(H, W)]
    assert frames.dtype == np.uint8 and np.array_equal(frames, R.make_frame(H, W))
    pad = tuple(int(v) for v in rec[R.out_key(H, W, mode) + "/pad"])
    assert pad == R.pads(H, W, mode)
    want = rec[R.out_key(H, W, mode)]
    got = R.ingest(frames, pad)
    assert got.dtype == np.float32 and got.shape == (1, pad[2] + H + pad[3], pad[0] + W + pad[1], 4)
    assert want.dtype == np.float32 and (want.shape[2] % 8, want.shape[3] % 8) == (0, 0)
    assert np.array_equal(R.bits(R.nchw(got)), R.bits(want))
    assert not R.bits(got[..., 3]).any()                                  # +0.0, not -0.0


def test_restatement_on_every_byte_value(rec):
    frames = rec["frame/all256"]
    assert np.array_equal(frames, R.all_bytes_frame()) and len(np.unique(frames)) == 256
    want = rec["ingest/all256"]
    assert np.array_equal(R.bits(R.nchw(R.ingest(frames, (0, 0, 0, 0)))), R.bits(want))
    assert len(np.unique(want)) == 256 and want.min() == -1.0 and want.max() == 1.0
    # BGR is the channel reversal of the same values
    assert np.array_equal(R.ingest(frames, (0, 0, 0, 0), bgr=True)[..., :3], R.ingest(frames, (0, 0, 0, 0))[..., 2::-1])


def test_restatement_is_the_torch_expression_on_the_cpu():
    """The yardstick itself: .float() / 255.0, F.pad(replicate), 2 * x - 1.0, evaluated by torch on the CPU."""
    frames = R.make_frame(7, 131, N=2)
    pad = (3, 4, 0, 7)
    x = torch.from_numpy(frames).permute(0, 3, 1, 2).float() / 255.0
    want = (2 * torch.nn.functional.pad(x, pad, mode="replicate") - 1.0).numpy()
    assert np.array_equal(R.bits(R.nchw(R.ingest(frames, pad))), R.bits(want))


# ---- header, binding, ABI ----------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry(built):
    src = open(os.path.join(ROOT, "include", "dvslam.h")).read()
    m = re.search(r"\bint\s+dvs_frame_ingest\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    assert m and m.group(1).count(",") + 1 == 13
    assert "dvs_frame_ingest" in built.exported_symbols() and len(built._SIGNATURES["dvs_frame_ingest"][1]) == 13
    assert hasattr(built.lib(), "dvs_frame_ingest")
    assert "2.0f * q - 1.0f" in src and "clamp(y - top, 0, H - 1)" in src            # the arithmetic is stated


def test_abi_is_still_12(built):
    assert built.ABI_VERSION == 12 and built.lib().dvs_abi_version() == 12


# ---- argument checks of the entry, on a machine without a GPU ---------------------------------------------------------------------
P = 4096          # a non-NULL, 16-byte aligned "device pointer": nothing dereferences it before the checks fail


def _ingest(l, src=P, image=5 * 21, row=21, dst=2 * P, N=1, H=5, W=7, left=0, right=1, top=1, bottom=2, bgr=0):
    return l.dvs_frame_ingest(src, image, row, dst, N, H, W, left, right, top, bottom, bgr, None)


BAD_CALLS = [
    ("NULL src", dict(src=None)),
    ("NULL dst", dict(dst=None)),
    ("misaligned dst", dict(dst=2 * P + 4)),
    ("N = 0", dict(N=0)),
    ("N = -1", dict(N=-1)),
    ("N = 65536", dict(N=65536)),
    ("H = 0", dict(H=0)),
    ("W = 0", dict(W=0)),
    ("left = 8", dict(left=8)),
    ("right = -1", dict(right=-1)),
    ("top = 8", dict(top=8)),
    ("bottom = -2", dict(bottom=-2)),
    ("bgr = 2", dict(bgr=2)),
    ("row stride < 3 W", dict(row=20)),
    ("image stride < the frame", dict(image=5 * 21 - 1)),
    ("too many lanes", dict(H=1 << 20, W=1 << 20, row=3 << 20, image=3 << 40)),
    ("stride out of range", dict(row=1 << 41, image=1 << 45)),
]


@pytest.mark.parametrize("name,kw", BAD_CALLS, ids=[b[0] for b in BAD_CALLS])
def test_entry_refuses_bad_arguments(built, name, kw):
    l = built.lib()
    assert _ingest(l, **kw) == -1                    # DVS_ERR_INVALID: no launch was tried (this machine has no GPU to refuse one)
    assert b"dvs_frame_ingest" in l.dvs_last_error()


def test_messages_say_what_is_wrong(built):
    l = built.lib()
    assert _ingest(l, row=20) < 0 and b"row stride 20 is below 3 * W = 21" in l.dvs_last_error()
    assert _ingest(l, image=104) < 0 and b"image stride 104 is below" in l.dvs_last_error()
    assert _ingest(l, left=8) < 0 and b"left=8" in l.dvs_last_error() and b"0 .. 7" in l.dvs_last_error()


# ---- the Python layer's input errors ------------------------------------------------------------------------------------------------
def test_frame_ingest_input_errors(built):
    from deep_visual_slam_amd import raft_video
    E = built.DvsError
    with pytest.raises(E, match="GPU tensors only .* no CPU path"):
        raft_video.frame_ingest(torch.zeros(5, 7, 3, dtype=torch.uint8))
    with pytest.raises(E, match="uint8 only, got torch.float32"):
        raft_video.frame_ingest(torch.zeros(5, 7, 3))
    with pytest.raises(E, match="a uint8 tensor .* expected, got ndarray"):
        raft_video.frame_ingest(np.zeros((5, 7, 3), np.uint8))
    for shape in ((7, 3), (5, 7, 4), (3, 5, 7), (1, 1, 5, 7, 3), (0, 7, 3)):
        with pytest.raises(E, match="expected, got"):
            raft_video.frame_ingest(torch.zeros(shape, dtype=torch.uint8))
    meta = torch.empty((5, 7, 3), dtype=torch.uint8, device="meta")
    with pytest.raises(E, match="GPU tensors only"):
        raft_video.frame_ingest(meta)


def test_flow_stream_input_errors(built):
    from deep_visual_slam_amd import raft, raft_video
    E = built.DvsError
    with pytest.raises(E, match="model must be a raft.RAFT or a raft.SmallRAFT"):
        raft_video.FlowStream(torch.nn.Identity())
    model = raft.SmallRAFT()
    with pytest.raises(E, match="iters=0"):
        raft_video.FlowStream(model, iters=0)
    stream = raft_video.FlowStream(model.eval(), iters=2)
    frame = torch.zeros(130, 141, 3, dtype=torch.uint8)
    with pytest.raises(E, match="uint8 only, got torch.float32"):
        stream.push(frame.float())
    with pytest.raises(E, match=r"\[H,W,3\] or \[N,H,W,3\] expected, got \(3, 130, 141\)"):
        stream.push(frame.permute(2, 0, 1))
    with pytest.raises(E, match="a uint8 tensor"):
        stream.push(frame.numpy())
    with pytest.raises(E, match="the model is on cpu; GPU only"):           # a host frame is fine, a host model is not
        stream.push(frame)
    model.train()
    with pytest.raises(E, match=r"train\(\) mode"):
        stream.push(frame)
    with pytest.raises(E, match="host=True only"):
        raft_video.FlowFrame(None, None, None).image_host
    stream.reset()                                                          # harmless before the first push
    # the issue's signature, and the default that the measured table of DESIGN.md section 22 decided
    import inspect
    params = inspect.signature(raft_video.FlowStream.__init__).parameters
    assert list(params)[1:11] == ['model', 'iters', 'warm_start', 'pad_mode', 'image', 'convert_to_bgr', 'bgr', 'graph', 'host', 'warmup']
    assert params['graph'].default is True and params['host'].default is False and params['iters'].default == 12
    assert raft_video.FlowStream(model, graph=False).use_graph is False


def test_encode_frame_and_refine_input_errors(built):
    from deep_visual_slam_amd import raft
    E = built.DvsError
    model = raft.SmallRAFT().eval()
    with pytest.raises(E, match=r"SmallRAFT.encode_frame: image4: GPU tensors only"):
        model.encode_frame(torch.zeros(1, 4, 136, 144))
    with pytest.raises(E, match=r"SmallRAFT.refine: feat1.fmap: GPU tensors only"):
        model.refine(object(), object())
