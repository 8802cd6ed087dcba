"""Guard-band runs (tests/guard.py) of dvs_frame_ingest (csrc/ingest.hip) at ragged shapes: the output sits between NaN bands and
the source between canary bands, all compared as raw bytes, and the values are checked bit for bit against tests/raftstream_ref.py
(a read outside the source would show as a wrong value at the clamped border, a write outside the output as a changed band).
The vector form (three dwords per lane) runs where the source pointer, the strides, W and `left` are multiples of 4; one byte
of storage offset puts the same frame through the scalar form."""
import numpy as np
import pytest
import torch

import guard
import raftstream_ref as R

pytestmark = pytest.mark.gpu
WIDTHS = (3, 4, 5, 64, 131)
CASES = [(H, W) for H in (1, 7) for W in WIDTHS]
PADS = ((0, 0, 0, 0), (3, 4, 0, 7), (4, 4, 0, 0))           # left = 4: the vector form's window clamped at the left border


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


@pytest.mark.parametrize("form", ["vector", "scalar"])
@pytest.mark.parametrize("pad", PADS, ids=["pad%d%d%d%d" % p for p in PADS])
@pytest.mark.parametrize("H,W", CASES, ids=["%dx%d" % c for c in CASES])
def test_frame_ingest_stays_inside_its_buffers(gpu_device, L, H, W, pad, form):
    N = 2
    frames = R.make_frame(H, W, N)
    shift = 0 if form == "vector" else 1
    g = guard.Bands(gpu_device)
    flat = torch.full((shift + frames.size,), 201, dtype=torch.uint8)
    flat[shift:] = torch.from_numpy(frames).reshape(-1)
    placed = g.place(flat, pattern=guard.CANARY)
    src = placed[shift:]
    left, right, top, bottom = pad
    out = g.empty((N, top + H + bottom, left + W + right, 4), pattern=guard.POISON)
    is_vector = shift == 0 and W % 4 == 0 and left % 4 == 0                 # the entry's own rule: 3 * W and 3 * H * W are then multiples of 4
    assert src.data_ptr() % 4 == shift
    L.check(L.lib().dvs_frame_ingest(src.data_ptr(), 3 * H * W, 3 * W, out.data_ptr(), N, H, W, left, right, top, bottom, 0, L.stream()),
            "dvs_frame_ingest")
    g.check()
    got = out.cpu().numpy()
    assert np.array_equal(R.bits(got), R.bits(R.ingest(frames, pad))), (form, is_vector)
