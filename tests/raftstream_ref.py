"""NumPy restatement of dvs_frame_ingest (csrc/ingest.hip) and the seeded inputs of tests/golden/raftstream_ingest.npz, which
holds what the reference's own chain returned on the CPU (tests/golden/make_golden_raftstream.py):

    load_image      torch.from_numpy(img).permute(2, 0, 1).float()[None] / 255.0      model/raft/raft.py:22-23
    InputPadder     F.pad(x, pad, mode='replicate')                                  model/raft/core/utils/utils.py:7-21
    RAFT.forward    2 * image - 1.0                                                  model/raft/core/raft.py:70-71, 188-190

Every operation is fp32 and rounded on its own; the division is the correctly rounded quotient and 2 * q is exact, so the result
has one defined bit pattern per byte value and the comparisons of the tests are exact."""
import numpy as np

WIDTHS = (1, 3, 4, 5, 63, 64, 65, 131)
HEIGHTS = (1, 2, 7)
MODES = ("sintel", "kitti")
SIZES = [(H, W) for H in HEIGHTS for W in WIDTHS]
# (left, right, top, bottom), as InputPadder._pad orders them; (4, 4, 0, 0) is the one non-zero left pad that keeps the vector form
EXPLICIT_PADS = ((0, 0, 0, 0), (3, 4, 0, 7), (0, 1, 3, 4), (4, 4, 0, 0))
ALL_BYTES = (16, 16)


def frame_key(H, W):
    return "frame/%dx%d" % (H, W)


def out_key(H, W, mode):
    return "ingest/%dx%d/%s" % (H, W, mode)


def make_frame(H, W, N=1):
    """Seeded uint8 frames [N,H,W,3]; frame n of a size is the same whatever N is."""
    return np.stack([np.random.default_rng(1000003 * H + 1009 * W + n).integers(0, 256, (H, W, 3), dtype=np.uint8) for n in range(N)])


def all_bytes_frame():
    """[1,16,16,3]: every byte value, three times each, no channel constant."""
    H, W = ALL_BYTES
    return ((np.arange(H * W * 3, dtype=np.int64) * 7) % 256).astype(np.uint8).reshape(1, H, W, 3)


def pads(H, W, mode):
    """InputPadder._pad = (left, right, top, bottom)."""
    pad_ht = (((H // 8) + 1) * 8 - H) % 8
    pad_wd = (((W // 8) + 1) * 8 - W) % 8
    if mode == "sintel":
        return (pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2)
    return (pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht)


def ingest(frames, pad, bgr=False):
    """frames uint8 [N,H,W,3] -> fp32 [N,Hp,Wp,4]: 2 * (x / 255) - 1, replicate-padded, fourth channel zero."""
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
    left, right, top, bottom = pad
    x = frames[..., ::-1] if bgr else frames
    q = x.astype(np.float32) / np.float32(255.0)
    v = np.float32(2.0) * q - np.float32(1.0)
    assert v.dtype == np.float32
    v = np.pad(v, ((0, 0), (top, bottom), (left, right), (0, 0)), mode="edge")
    return np.concatenate([v, np.zeros(v.shape[:3] + (1,), np.float32)], axis=-1)


def nchw(out4):
    """The first three channels of an ingest result as the reference's [N,3,Hp,Wp]."""
    return np.ascontiguousarray(out4[..., :3].transpose(0, 3, 1, 2))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)
