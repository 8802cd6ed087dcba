"""NumPy restatements of what csrc/flowstage.hip and raft_video.py replace: forward_interpolate and InputPadder
(model/raft/core/utils/utils.py:7-54) and flow_to_image (model/raft/core/utils/flow_viz.py:20-132), each with the reference's own
dtype ladder spelled out.  tests/golden/make_golden_flowstage.py runs the reference's functions and these on the same inputs; the
CPU tests hold the two equal, byte for byte, so the GPU tests may use either.

This is a plain module (imported like raft_ref), not a conftest.
"""
import numpy as np

F32 = np.float32


# ---- forward_interpolate ----------------------------------------------------------------------------------------------------
def forward_interpolate(flow, chunk=512):
    """(out [2,h,w] fp32, margin [h,w] fp64, valid count) of flow [2,h,w] fp32: utils.py:26-54 as a brute-force search in fp64.

    x1 = x + dx, y1 = y + dy in fp64 (int64 grid + fp32 flow); a source is valid iff 0 < x1 < w and 0 < y1 < h; every grid pixel
    takes the flow of the valid source with the smallest d2 = (x1 - x)^2 + (y1 - y)^2, the lowest row-major index among equals
    (np.argmin's rule, and the kernel's).  No valid source: zeros (the reference has no answer there: NaN from griddata on zero points under SciPy 1.15).
    margin = (second smallest d2 - smallest d2) / second smallest d2 per pixel, 1 with fewer than two valid sources, 0 where the
    two smallest are both 0: where it is tiny the reference's KD-tree and this rule may legitimately pick different sources."""
    flow = np.asarray(flow)
    assert flow.dtype == F32 and flow.ndim == 3 and flow.shape[0] == 2, (flow.dtype, flow.shape)
    dx, dy = flow[0], flow[1]
    h, w = dx.shape
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1 = (x0 + dx).reshape(-1)
    y1 = (y0 + dy).reshape(-1)
    assert x1.dtype == np.float64
    valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    idx = np.nonzero(valid)[0]
    out = np.zeros((2, h * w), F32)
    margin = np.ones(h * w, np.float64)
    if idx.size:
        sx, sy = x1[idx], y1[idx]
        tx, ty = x0.reshape(-1).astype(np.float64), y0.reshape(-1).astype(np.float64)
        for lo in range(0, h * w, chunk):
            ex = sx[None, :] - tx[lo:lo + chunk, None]
            ey = sy[None, :] - ty[lo:lo + chunk, None]
            d2 = ex * ex + ey * ey
            best = np.argmin(d2, axis=1)
            out[0, lo:lo + chunk] = dx.reshape(-1)[idx[best]]
            out[1, lo:lo + chunk] = dy.reshape(-1)[idx[best]]
            if idx.size > 1:
                two = np.partition(d2, 1, axis=1)[:, :2]
                with np.errstate(invalid="ignore", divide="ignore"):
                    margin[lo:lo + chunk] = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
    return out.reshape(2, h, w), margin.reshape(h, w), int(idx.size)


# ---- flow_to_image ----------------------------------------------------------------------------------------------------------
SEGMENTS = (15, 6, 4, 11, 13, 6)          # red-yellow, yellow-green, green-cyan, cyan-blue, blue-magenta, magenta-red
NCOLS = sum(SEGMENTS)


def make_colorwheel():
    """[55,3] fp64, flow_viz.py:20-67: an even segment s holds channel s/2 at 255 and ramps the next one up, an odd one holds
    channel (s+1)/2 at 255 and ramps the one before down; the ramp is floor(255 * i / length)."""
    wheel = np.zeros((NCOLS, 3))
    k = 0
    for s, n in enumerate(SEGMENTS):
        ramp = np.floor(255 * np.arange(n) / n)
        wheel[k:k + n, ((s + 1) // 2) % 3] = 255
        if s % 2:
            wheel[k:k + n, (s - 1) // 2] = 255 - ramp
        else:
            wheel[k:k + n, (s // 2 + 1) % 3] = ramp
        k += n
    return wheel


def flow_radius(flow, clip_flow=None):
    """(u, v, rad_max) in fp32 of flow [2,H,W] fp32: flow_viz.py:123-128."""
    flow = np.asarray(flow)
    assert flow.dtype == F32 and flow.ndim == 3 and flow.shape[0] == 2, (flow.dtype, flow.shape)
    if clip_flow is not None:
        flow = np.clip(flow, F32(0), F32(clip_flow))
    u, v = flow[0], flow[1]
    rad = np.sqrt(u * u + v * v)
    assert rad.dtype == F32
    return u, v, rad.max()


def _colors(fk, rad, convert_to_bgr):
    """flow_viz.py:91-105 from fk (fp64 here: the fp32 value widened, or a perturbed one) and rad (fp32 or fp64)."""
    wheel = make_colorwheel()
    fk = np.clip(fk, 0.0, float(NCOLS - 1))                  # a no-op for the ladder's own fk in 0 .. 54
    k0 = np.floor(fk).astype(np.int32)
    k1 = k0 + 1
    k1[k1 == NCOLS] = 0
    f = fk - k0
    img = np.zeros(fk.shape + (3,), np.uint8)
    for i in range(3):
        col0 = wheel[k0, i] / 255.0
        col1 = wheel[k1, i] / 255.0
        col = (1 - f) * col0 + f * col1
        inside = rad <= 1
        col = np.where(inside, 1 - rad * (1 - col), col * 0.75)
        img[..., 2 - i if convert_to_bgr else i] = np.floor(255 * col)
    return img


def flow_to_image(flow, clip_flow=None, convert_to_bgr=False, with_exempt=False):
    """uint8 [H,W,3] of flow [2,H,W] fp32 (the model's layout): flow_viz.py:109-132 under NumPy >= 2 scalar promotion.  fp32, each
    operation rounded on its own, up to fk; fp64 from floor(fk) on.

    with_exempt=True returns (image, exempt [H,W,3] bool, largest difference between variants): a byte is exempt where
    re-evaluating it with fk -+ 3e-5 and rad * (1 -+ 4 * 2^-23), in all nine combinations, does not give one value.  atan2f is
    the one operation that is correctly rounded on neither side: NumPy's fp32 arctan2 stays below 4 ulp and the device's is
    taken as <= 2 ulp, so |d fk| <= 27 * 6 * ulp(pi) / pi + 2 ulp(54) ~ 2e-5."""
    u, v, rad_max = flow_radius(flow, clip_flow)
    den = rad_max + F32(1e-5)
    assert den.dtype == F32
    u = u / den
    v = v / den
    rad = np.sqrt(u * u + v * v)
    a = np.arctan2(-v, -u) / F32(np.pi)
    fk = (a + F32(1)) / F32(2) * F32(NCOLS - 1)
    assert fk.dtype == F32 and rad.dtype == F32
    img = _colors(fk.astype(np.float64), rad, convert_to_bgr)
    if not with_exempt:
        return img
    lo, hi = img.astype(np.int32), img.astype(np.int32)
    for dfk in (-3e-5, 0.0, 3e-5):
        for drad in (-4.0 * 2.0 ** -23, 0.0, 4.0 * 2.0 ** -23):
            var = _colors(fk.astype(np.float64) + dfk, rad.astype(np.float64) * (1.0 + drad), convert_to_bgr).astype(np.int32)
            lo, hi = np.minimum(lo, var), np.maximum(hi, var)
    return img, hi != lo, int((hi - lo).max())


# ---- InputPadder ------------------------------------------------------------------------------------------------------------
class InputPadder:
    """utils.py:7-24 on NumPy arrays [..., H, W]: edge padding to multiples of 8."""

    def __init__(self, dims, mode="sintel"):
        self.ht, self.wd = dims[-2:]
        pad_ht = (((self.ht // 8) + 1) * 8 - self.ht) % 8
        pad_wd = (((self.wd // 8) + 1) * 8 - self.wd) % 8
        if mode == "sintel":
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]
        else:
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]

    def pad(self, *inputs):
        left, right, top, bottom = self._pad
        return [np.pad(x, [(0, 0)] * (x.ndim - 2) + [(top, bottom), (left, right)], mode="edge") for x in inputs]

    def unpad(self, x):
        ht, wd = x.shape[-2:]
        left, right, top, bottom = self._pad
        return x[..., top:ht - bottom, left:wd - right]


# ---- the cases of the fixture (tests/golden/flowstage.npz) ------------------------------------------------------------------
# forward_interp: the kernel owns 64 grid pixels per workgroup, a wave takes 64 sources of each staged tile of 1024
FI_SHAPES = [(1, 1), (2, 3), (5, 7), (7, 9), (8, 8), (5, 13), (1, 257), (257, 1), (16, 17), (31, 33), (32, 32), (25, 41), (1, 1025),
             (55, 128)]
FI_IMAGES = ("most", "six", "none")       # per shape: most sources valid, six valid, none valid
MAX_EXEMPT = 5e-3                         # flow_to_image: share of a case's bytes that may be exempt from exact comparison
FV_WIDTHS, FV_HEIGHTS = (1, 3, 4, 5, 63, 64, 65, 131), (1, 2, 7)
FV_SIZES = [(H, W) for H in FV_HEIGHTS for W in FV_WIDTHS]
FV_SCALES = (1.0, 3.0, 0.01)              # the three images of a noise case: different maxima, all below 21 (see FV_LARGE)
FV_LARGE = 30.0                           # at FV_BIG only: past rad_max ~ 21 the largest pixel's rad = rad_max / (rad_max + 1e-5) is
                                          # within 4 * 2^-23 of 1, the `rad <= 1` branch of its variants flips and its 3 bytes are
                                          # exempt -- 0.5 % of the bytes only from 200 pixels up
FV_BIG = (131, 77)
FV_SPECIAL = (7, 65)                      # zero flow, a single non-zero pixel, clip_flow, BGR
PAD_SIZES = [(130, 141), (436, 1024)]


def fi_key(h, w):
    return "fi/%dx%d" % (h, w)


def fv_key(H, W):
    return "fv/%dx%d" % (H, W)


def fi_inputs(h, w):
    """[3,2,h,w] fp32: the three images of a forward_interp case (FI_IMAGES), seeded by the shape."""
    rng = np.random.default_rng(1000 * h + w)
    a = rng.standard_normal((2, h, w)) * np.array([max(0.5, 0.15 * w), max(0.5, 0.15 * h)])[:, None, None]
    a = a.astype(F32)
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    valid = ((x0 + a[0] > 0) & (x0 + a[0] < w) & (y0 + a[1] > 0) & (y0 + a[1] < h)).reshape(-1)
    if not valid.any():                   # a tiny shape whose draw left nothing inside: pixel 0 stays
        a[:, 0, 0] = (0.5, 0.25)
        valid[0] = True
    keep = rng.permutation(np.nonzero(valid)[0])[:6]
    b = np.full((2, h * w), -1e4, F32)
    b[:, keep] = a.reshape(2, -1)[:, keep]
    c = np.full((2, h, w), 1e4, F32)
    return np.stack([a, b.reshape(2, h, w), c])


def fv_noise(H, W):
    """[3,2,H,W] fp32 noise at the three scales."""
    for attempt in range(50):              # a draw with more than 0.5 % exempt bytes is refused as a case: at a few hundred bytes
        rng = np.random.default_rng(77 * H + W + 100003 * attempt)                            # one exempt byte is too many
        flows = np.stack([(rng.standard_normal((2, H, W)) * s).astype(F32) for s in FV_SCALES])
        exempt = sum(int(flow_to_image(f, with_exempt=True)[1].sum()) for f in flows)
        if exempt <= MAX_EXEMPT * 3 * (3 * H * W):
            return flows
    raise RuntimeError("fv_noise(%d, %d): no draw within the exempt cap" % (H, W))


def fv_big(name):
    """[2,131,77] fp32: large (noise at FV_LARGE) or smooth."""
    H, W = FV_BIG
    if name == "smooth":
        return fv_smooth(H, W)
    rng = np.random.default_rng(4242)
    return (rng.standard_normal((2, H, W)) * {"large": FV_LARGE}[name]).astype(F32)


FV_BIG_NAMES = ("large", "smooth")


def fv_smooth(H, W):
    """[2,H,W] fp32: a rotation about the centre plus a slow wave -- every direction, radii from 0 up."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u = -(y - H / 2) * 0.11 + 3.0 * np.sin(x / 17.0)
    v = (x - W / 2) * 0.13 + 2.0 * np.cos(y / 23.0)
    return np.stack([u, v]).astype(F32)


def fv_special(name):
    """(flow [2,H,W], clip_flow, convert_to_bgr) of the named case at FV_SPECIAL."""
    H, W = FV_SPECIAL
    noise = fv_noise(H, W)[1]
    if name == "zero":
        return np.zeros((2, H, W), F32), None, False
    if name == "single":
        f = np.zeros((2, H, W), F32)
        f[:, 3, 40] = (-2.5, 1.25)
        return f, None, False
    if name == "clip":
        return noise, 4.0, False
    if name == "bgr":
        return noise, None, True
    raise KeyError(name)


FV_SPECIAL_NAMES = ("zero", "single", "clip", "bgr")
