"""NumPy restatement of dvs_flow_consistency (csrc/flowcons.hip; include/dvslam.h states the arithmetic) and the seeded inputs of its
tests: the forward-backward check of UnFlow (Meister et al. 2018, eq. 2) with the bilinear gather of the reference's bilinear_sampler
(model/raft/core/utils/utils.py:57-71) in pixel coordinates.

`direction(a, b)` is one direction, operation by operation in fp32; with dtype=np.float64 the same function starts from the
fp32-ROUNDED qx, qy (which is the definition: the sample position is an fp32 number) and does everything after it in fp64.
tests/golden/make_golden_flowcons.py runs the reference's bilinear_sampler on the cases of CASES; tests/test_flowcons_cpu.py holds
the restatement's gather against it.

This is a plain module (imported like flowstage_ref), not a conftest.
"""
from types import SimpleNamespace

import numpy as np

import flowstage_ref

F32 = np.float32
ALPHA, BETA = 0.01, 0.5


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def direction(a, b, alpha=ALPHA, beta=BETA, dtype=F32):
    """One direction: own flow a [N,2,H,W] fp32 on its image's grid, partner flow b [N,2,H,W] fp32.  A namespace of [N,H,W] fields:
    inside (bool), bu, bv (the gathered partner flow; 0 where not inside), tu, tv (the same gather of |b|: what the rounding errors
    of bu, bv scale with), sx, sy, d, m, thr, excess (`dtype`; +inf where not inside or where d - thr is NaN), valid (uint8)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == F32 and b.dtype == F32 and a.shape == b.shape and a.ndim == 4 and a.shape[1] == 2, (a.dtype, a.shape, b.shape)
    N, _, H, W = a.shape
    T = dtype
    alpha, beta = T(F32(alpha)), T(F32(beta))                 # the entry takes fp32 arguments
    au, av = a[:, 0], a[:, 1]
    with np.errstate(all="ignore"):
        qx = np.arange(W, dtype=F32)[None, None, :] + au
        qy = np.arange(H, dtype=F32)[None, :, None] + av
        assert qx.dtype == F32 and qy.dtype == F32
        inside = (qx >= 0) & (qx <= F32(W - 1)) & (qy >= 0) & (qy <= F32(H - 1))
        qx, qy = np.where(inside, qx, F32(0)).astype(T), np.where(inside, qy, F32(0)).astype(T)    # outside: nothing is read
        fx, fy = np.floor(qx), np.floor(qy)
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        wx, wy = qx - fx, qy - fy
        ux, uy = 1 - wx, 1 - wy
        n = np.arange(N)[:, None, None]

        def s(p):
            p = p.astype(T)
            top = p[n, y0, x0] * ux + p[n, y0, x1] * wx
            bot = p[n, y1, x0] * ux + p[n, y1, x1] * wx
            return top * uy + bot * wy

        bu, bv = s(b[:, 0]), s(b[:, 1])
        tu, tv = s(np.abs(b[:, 0])), s(np.abs(b[:, 1]))
        au, av = au.astype(T), av.astype(T)
        sx, sy = au + bu, av + bv
        d = sx * sx + sy * sy
        m = (au * au + av * av) + (bu * bu + bv * bv)
        thr = alpha * m + beta
        e = d - thr
        assert e.dtype == T
        excess = np.where(inside & ~np.isnan(e), e, T(np.inf))
        valid = (inside & (excess <= 0)).astype(np.uint8)
    zero = lambda t: np.where(inside, t, T(0))
    return SimpleNamespace(inside=inside, bu=zero(bu), bv=zero(bv), tu=zero(tu), tv=zero(tv), sx=zero(sx), sy=zero(sy), d=zero(d),
                           m=zero(m), thr=zero(thr), alpha=alpha, excess=excess, valid=valid)


def consistency(a, b, alpha=ALPHA, beta=BETA, dtype=F32):
    """(direction a, direction b) of the flows a (on image 1's grid) and b (on image 2's)."""
    return direction(a, b, alpha, beta, dtype), direction(b, a, alpha, beta, dtype)


# ---- shapes and inputs ---------------------------------------------------------------------------------------------------------------
WIDTHS, HEIGHTS = flowstage_ref.FV_WIDTHS, flowstage_ref.FV_HEIGHTS           # (1, 3, 4, 5, 63, 64, 65, 131) x (1, 2, 7)
SIZES = [(H, W) for H in HEIGHTS for W in WIDTHS]
BIG = (131, 77)
SCALES = (0.01, 0.7, 3.0, 30.0)           # everything valid ... mostly outside
BAND_UNITS = 16.0                         # no pixel of a seeded case has |excess| within this many units of 2^-23 (d + thr)


def units(r32, r64):
    """(err, dist, count) per pixel, in units of 2^-23 (d + thr), over the pixels that are inside and finite in fp64 (0, inf, 0
    elsewhere): err = |excess32 - excess64|, dist = |excess64| (the distance from the threshold) and count = the bound on err
    that the operation count gives, with u = 2^-24 the relative error of one fp32 operation, to first order in u:

        wx, wy           exact (q - floor(q), q an fp32 number in both runs)
        bu               6 roundings on its longest path (1 - wx, the product, the sum, 1 - wy, the product, the sum), each
                         acting on terms whose absolute sum is tu = the same gather of |b.u|:          |dbu| <= 6 u tu
        sx = a.u + bu    |dsx| <= 6 u tu + u |sx|
        sx * sx          2 |sx| |dsx| + u sx^2 = 12 u |sx| tu + 3 u sx^2
        d                12 u (|sx| tu + |sy| tv) + 3 u d + u d
        bu^2 + bv^2      12 u (|bu| tu + |bv| tv) + 2 u (bu^2 + bv^2);   a.u^2 + a.v^2: 2 u of itself
        m                12 u (|bu| tu + |bv| tv) + 3 u m
        thr              alpha dm + u alpha m + u thr <= 5 u thr + 12 u alpha (|bu| tu + |bv| tv)
        excess           dd + dthr + u |excess| <= 6 u (d + thr) + 12 u [|sx| tu + |sy| tv + alpha (|bu| tu + |bv| tv)]

    = (3 + 6 A) units, A = [...] / (d + thr): A <= 1 where nothing cancels (tu = |bu|, |sx| >= |bu|), larger where a small sx is
    the difference of large numbers."""
    ok = r64.inside & np.isfinite(r64.excess)
    unit = 2.0 ** -23 * (r64.d + r64.thr)
    with np.errstate(all="ignore"):
        err = np.where(ok, np.abs(r32.excess.astype(np.float64) - r64.excess) / unit, 0.0)
        dist = np.where(ok, np.abs(r64.excess) / unit, np.inf)
        A = (np.abs(r64.sx) * r64.tu + np.abs(r64.sy) * r64.tv + r64.alpha * (np.abs(r64.bu) * r64.tu + np.abs(r64.bv) * r64.tv))
        count = np.where(ok, 3.0 + 6.0 * A / (r64.d + r64.thr), 0.0)
    return err, dist, count


def in_band(a, b, alpha=ALPHA, beta=BETA):
    """Pixels of either direction whose fp64 excess lies within max(BAND_UNITS, its own count) units of the threshold: only there
    may the fp32 mask differ from the fp64 one."""
    total = 0
    for r32, r64 in zip(consistency(a, b, alpha, beta), consistency(a, b, alpha, beta, np.float64)):
        _, dist, count = units(r32, r64)
        total += int((dist < np.maximum(BAND_UNITS, count)).sum())
    return total


def noise(H, W, scale, N=3):
    """(a, b) [N,2,H,W] fp32: a is noise at `scale`, b = -a + noise at a tenth of it + a few large outliers -- so that at the small
    scales most pixels are valid and some are not.  A draw with a pixel inside the band is redrawn, as fv_noise redraws."""
    for attempt in range(50):
        rng = np.random.default_rng(int(1000 * scale) + 977 * H + W + 100003 * attempt)
        a = (rng.standard_normal((N, 2, H, W)) * scale).astype(F32)
        b = (-a + rng.standard_normal((N, 2, H, W)) * (0.1 * scale)).astype(F32)
        b = np.where(rng.random((N, 1, H, W)) < 0.1, b + F32(2.0), b).astype(F32)
        if in_band(a, b) == 0:
            return a, b
    raise RuntimeError("noise(%d, %d, %g): no draw outside the band" % (H, W, scale))


def smooth(H, W, N=1):
    """The rotation-plus-wave field of flowstage_ref.fv_smooth and its negative: b = -a is the exact inverse only where a is
    constant, so the interior is valid where the field varies slowly and invalid where it does not."""
    a = np.repeat(flowstage_ref.fv_smooth(H, W)[None], N, 0)
    for n in range(N):
        a[n] *= F32(1.0 / (1 + n))
    return a, (-a).astype(F32)


def zero(H, W, N=1):
    z = np.zeros((N, 2, H, W), F32)
    return z, z.copy()


def edge(H, W, outside=False):
    """N = 1: every pixel's flow lands exactly on (W - 1, H - 1) -- or, with outside=True, one fp32 step past it in x (even
    pixels) or in y (odd pixels); b is zero, so |a|^2 decides."""
    y, x = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    u, v = F32(W - 1) - x, F32(H - 1) - y
    if outside:
        odd = ((x + y) % 2).astype(bool)
        over = lambda t: np.nextafter(t, F32(np.inf), dtype=F32) if t > 0 else F32(2.0 ** -24)
        u = np.where(~odd, u + (over(F32(W - 1)) - F32(W - 1)), u).astype(F32)
        v = np.where(odd, v + (over(F32(H - 1)) - F32(H - 1)), v).astype(F32)
    a = np.stack([u, v])[None].astype(F32)
    return a, np.zeros_like(a)


def special(H, W):
    """N = 2 noise at scale 0.7 with NaN and +-inf entries in both flows."""
    a, b = noise(H, W, 0.7, N=2)
    a, b = a.copy(), b.copy()
    rng = np.random.default_rng(5 * H + W)
    for t in (a, b):
        flat = t.reshape(-1)
        idx = rng.permutation(flat.size)[:max(3, flat.size // 8)]
        flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf], F32), idx.size)
    return a, b


def occluder(H=24, W=40, top=8, left=10, size=8, shift=5):
    """A static background and a size x size square that moves by (+shift, 0) from image 1 to image 2; both analytic flows are
    integer valued.  (a, b [1,2,H,W], want_valid, want_valid_bw [1,H,W] uint8): the forward mask is 0 exactly on the shift x size
    background pixels of image 1 that the square newly covers, the backward mask on the shift x size pixels of image 2 it uncovers."""
    a, b = np.zeros((1, 2, H, W), F32), np.zeros((1, 2, H, W), F32)
    a[0, 0, top:top + size, left:left + size] = shift                      # image 1: the square moves right
    b[0, 0, top:top + size, left + shift:left + shift + size] = -shift     # image 2: the square came from the left
    va, vb = np.ones((1, H, W), np.uint8), np.ones((1, H, W), np.uint8)
    va[0, top:top + size, left + size:left + size + shift] = 0             # background of image 1 under the square's new place
    vb[0, top:top + size, left:left + shift] = 0                           # background of image 2 where the square was
    return a, b, va, vb


def cases(H, W):
    """[(name, a, b)] at one shape: the input families of the kernel tests."""
    out = [("noise%g" % s, *noise(H, W, s)) for s in SCALES]
    out += [("smooth", *smooth(H, W, N=3)), ("zero", *zero(H, W, N=3)), ("edge", *edge(H, W)), ("outside", *edge(H, W, True)),
            ("special", *special(H, W))]
    return out


# ---- the fixture (tests/golden/flowcons.npz): the reference's bilinear_sampler on a few of the cases ---------------------------------
GOLDEN_SIZES = [(2, 3), (7, 5), (7, 64), (7, 131), (2, 65)]                  # H, W >= 2: the reference divides by W - 1 and H - 1
GOLDEN_SCALES = (0.7, 3.0)


def golden_key(H, W, scale):
    return "%dx%d/noise%g" % (H, W, scale)
