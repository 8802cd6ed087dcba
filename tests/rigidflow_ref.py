"""NumPy restatement of dvs_rigid_flow (csrc/rigidflow.hip; include/dvslam.h states the arithmetic) and the seeded inputs of its
tests: the reference's BackprojectDepth and Project3D (vo/learner_func.py:106-159) in pixel coordinates, and the residual of a
measured flow against the rigid flow.

`rigid(...)` is the entry, operation by operation in fp32; with dtype=np.float64 the same formulas are evaluated in fp64 from the
fp32 inputs.  tests/golden/make_golden_rigidflow.py runs the reference's own layers on the cases of GOLDEN;
tests/test_rigidflow_cpu.py holds the restatement against them.

The error bounds (u = 2^-24, the relative error of one fp32 operation; first order in u; |.| of a sum means the sum of the
absolute values of its terms, which is what a rounding error of a partial sum scales with, in ANY order of summation):

    r_i = iK[i][0] x + iK[i][1] y + iK[i][2]       a term passes 1 product and at most 2 sums:        |dr_i| <= 3 u R_i
                                                   R_i = |iK[i][0] x| + |iK[i][1] y| + |iK[i][2]|
    X_i = d r_i                                    |dX_i| <= 3 u |d| R_i + u |X_i| <= 4 u A_i          A_i = |d| R_i
    P[i][j] = sum_k K[i][k] T[k][j]                a term passes 1 product and at most 3 sums:        |dP_ij| <= 4 u Q_ij
                                                   Q_ij = sum_k |K[i][k] T[k][j]|
    c_i = sum_j P[i][j] X_j + P[i][3]              the product: |X_j| dP_ij + |P_ij| dX_j + u |P_ij X_j| <= 9 u Q_ij A_j, and at
                                                   most 3 sums; P[i][3]: 4 u Q_i3 and at most 3 sums:
                                                   |dc_i| <= 12 u C_i                                  C_i = sum_j Q_ij A_j + Q_i3
    den = c_z + eps                                |dden| <= 12 u C_z + u |den|
    p = c_x / den                                  through dp/dc_x = 1 / den and dp/dden = -c_x / den^2, and its own rounding:
                                                   |dp| <= E = 12 u (C_x + |p| C_z) / |den| + 2 u |p|

E bounds the distance of EITHER side (the restatement in the header's order, the reference's matmuls in whatever order) from the
exact value of the formulas on the fp32 inputs.  The reference then normalises, t = p / (W - 1) (u |t|), (t - 0.5) (u |t - 0.5|),
* 2 (exact), and the fixture un-normalises in fp64 (exact): the round trip costs at most u (|p| + |p| + (W - 1) / 2), about one
ulp of the coordinate.  Restatement against fixture:

    |p - p_reference| <= 2 E + u (2 |p| + (W - 1) / 2)                                  (fixture_bound; H - 1 for the y coordinate)

fp32 against fp64, per pixel (units): r = p - x adds one rounding, D = E + u |r|; then, as flowcons_ref.units,

    ex = f - r            D + u |ex|
    ex^2                  2 |ex| D + 3 u ex^2
    e2                    2 (|ex| Dx + |ey| Dy) + 4 u e2
    m                     2 (|ru| Dx + |rv| Dy) + 3 u m
    thr = alpha m + beta  2 alpha (|ru| Dx + |rv| Dy) + 5 u thr
    excess = e2 - thr     2 [(|ex| + alpha |ru|) Dx + (|ey| + alpha |rv|) Dy] + 6 u (e2 + thr)

= (3 + G) units of 2^-23 (e2 + thr), G = [(|ex| + alpha |ru|) Dx + (|ey| + alpha |rv|) Dy] / (u (e2 + thr)).

This is a plain module (imported like flowcons_ref), not a conftest.
"""
from types import SimpleNamespace

import numpy as np

import flowstage_ref

F32 = np.float32
U = 2.0 ** -24
ALPHA, BETA, EPS = 0.01, 0.5, 1e-7
QNAN = 0x7FC00000


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def _mats(m, N, T):
    m = np.asarray(m)
    assert m.dtype == F32 and m.shape in ((4, 4), (N, 4, 4)), (m.dtype, m.shape)
    return np.broadcast_to(m, (N, 4, 4)).astype(T)


def rigid(depth, T, K, iK, flow=None, valid=None, alpha=ALPHA, beta=BETA, eps=EPS, dtype=F32):
    """The entry: depth [N,H,W] or [N,1,H,W], T [N,4,4], K and iK [4,4] or [N,4,4], flow [N,2,H,W] or None, all fp32; valid uint8
    [N,H,W] or None.  A namespace of [N,H,W] fields in `dtype`: px, py, cz, den, ru, rv (a non-finite one is the quiet NaN), inside
    (bool), and with a flow ex, ey, e2, m, thr, excess (+inf where not judged), label (uint8)."""
    depth = np.asarray(depth)
    assert depth.dtype == F32 and depth.ndim in (3, 4), (depth.dtype, depth.shape)
    if depth.ndim == 4:
        assert depth.shape[1] == 1
        depth = depth[:, 0]
    N, H, W = depth.shape
    Tt = dtype
    T, K, iK = _mats(T, N, Tt), _mats(K, N, Tt), _mats(iK, N, Tt)
    at = lambda m, i, j: m[:, i, j][:, None, None]
    with np.errstate(all="ignore"):
        P = [[((at(K, i, 0) * at(T, 0, j) + at(K, i, 1) * at(T, 1, j)) + at(K, i, 2) * at(T, 2, j)) + at(K, i, 3) * at(T, 3, j)
              for j in range(4)] for i in range(3)]
        x = np.arange(W, dtype=F32).astype(Tt)[None, None, :]
        y = np.arange(H, dtype=F32).astype(Tt)[None, :, None]
        d = depth.astype(Tt)
        r = [(at(iK, i, 0) * x + at(iK, i, 1) * y) + at(iK, i, 2) for i in range(3)]
        X, Y, Z = d * r[0], d * r[1], d * r[2]
        c = [((P[i][0] * X + P[i][1] * Y) + P[i][2] * Z) + P[i][3] for i in range(3)]
        den = c[2] + Tt(F32(eps))
        px, py = c[0] / den, c[1] / den
        ru, rv = px - x, py - y
        assert ru.dtype == Tt and rv.dtype == Tt and px.shape == (N, H, W)
        nan = np.array([QNAN], np.uint32).view(F32)[0].astype(Tt)
        ru, rv = np.where(np.isfinite(ru), ru, nan), np.where(np.isfinite(rv), rv, nan)
        inside = (c[2] > 0) & (px >= 0) & (px <= Tt(W - 1)) & (py >= 0) & (py <= Tt(H - 1))
        out = SimpleNamespace(px=px, py=py, cz=np.broadcast_to(c[2], px.shape), den=np.broadcast_to(den, px.shape), ru=ru, rv=rv,
                              inside=inside, rigid=np.stack([ru, rv], 1), alpha=Tt(F32(alpha)))
        if flow is None:
            return out
        flow = np.asarray(flow)
        assert flow.dtype == F32 and flow.shape == (N, 2, H, W), (flow.dtype, flow.shape)
        alpha, beta = Tt(F32(alpha)), Tt(F32(beta))
        fu, fv = flow[:, 0].astype(Tt), flow[:, 1].astype(Tt)
        ex, ey = fu - ru, fv - rv
        e2 = ex * ex + ey * ey
        m = (fu * fu + fv * fv) + (ru * ru + rv * rv)
        thr = alpha * m + beta
        e = e2 - thr
        assert e.dtype == Tt
        judged = inside & ~np.isnan(e)
        if valid is not None:
            valid = np.asarray(valid)
            assert valid.dtype == np.uint8 and valid.shape == (N, H, W)
            judged = judged & (valid != 0)
        out.excess = np.where(judged, e, Tt(np.inf))
        out.label = np.where(judged, np.where(e <= 0, 1, 2), 0).astype(np.uint8)
        out.judged, out.ex, out.ey, out.e2, out.m, out.thr = judged, ex, ey, e2, m, thr
    return out


# ---- the bounds of the module docstring -------------------------------------------------------------------------------------------------
def coordinate_error(depth, T, K, iK, eps=EPS):
    """(Ex, Ey, Ez, r64): E of the module docstring for px and for py and the bound 12 u C_z of cz, [N,H,W] fp64, and the fp64 run
    they are taken from."""
    r64 = rigid(depth, T, K, iK, eps=eps, dtype=np.float64)
    N, H, W = r64.px.shape
    T, K, iK = (np.abs(_mats(m, N, np.float64)) for m in (T, K, iK))
    x, y = np.arange(W, dtype=np.float64)[None, None, :], np.arange(H, dtype=np.float64)[None, :, None]
    d = np.abs(np.asarray(depth, np.float64).reshape(N, H, W))
    at = lambda m, i, j: m[:, i, j][:, None, None]
    A = [d * (at(iK, i, 0) * x + at(iK, i, 1) * y + at(iK, i, 2)) for i in range(3)]
    Q = lambda i, j: sum(at(K, i, k) * at(T, k, j) for k in range(4))
    C = [sum(Q(i, j) * A[j] for j in range(3)) + Q(i, 3) for i in range(3)]
    with np.errstate(all="ignore"):
        E = [12 * U * (C[i] + np.abs(p) * C[2]) / np.abs(r64.den) + 2 * U * np.abs(p) for i, p in ((0, r64.px), (1, r64.py))]
    return E[0], E[1], 12 * U * C[2] + 0 * r64.px, r64


def fixture_bound(depth, T, K, iK, eps=EPS):
    """(bound on |px - the reference's px|, the same for py), per pixel."""
    Ex, Ey, _, r64 = coordinate_error(depth, T, K, iK, eps)
    N, H, W = r64.px.shape
    return 2 * Ex + U * (2 * np.abs(r64.px) + (W - 1) / 2), 2 * Ey + U * (2 * np.abs(r64.py) + (H - 1) / 2)


BAND_UNITS = 16.0        # no pixel of a seeded case has |excess| within max(this, its own count) units of 2^-23 (e2 + thr) of 0


def units(s, flow, r32, r64, alpha=ALPHA):
    """(err, dist, count, Dx, Dy) per pixel over the pixels judged in fp64 (0, inf, 0 elsewhere for the first three): err =
    |excess32 - excess64|, dist = |excess64| and count = the bound on err, in units of 2^-23 (e2 + thr); Dx, Dy bound |ru32 - ru64|
    and |rv32 - rv64|."""
    Ex, Ey, _, _ = coordinate_error(s.depth, s.T, s.K, s.iK, s.eps)
    Dx, Dy = Ex + U * np.abs(r64.ru), Ey + U * np.abs(r64.rv)
    ok = r64.judged & np.isfinite(r64.excess)
    unit = 2.0 ** -23 * (r64.e2 + r64.thr)
    with np.errstate(all="ignore"):
        err = np.where(ok, np.abs(r32.excess.astype(np.float64) - r64.excess) / unit, 0.0)
        dist = np.where(ok, np.abs(r64.excess) / unit, np.inf)
        a = float(F32(alpha))
        G = ((np.abs(r64.ex) + a * np.abs(r64.ru)) * Dx + (np.abs(r64.ey) + a * np.abs(r64.rv)) * Dy) / (U * (r64.e2 + r64.thr))
        count = np.where(ok, 3.0 + G, 0.0)
    return err, dist, count, Dx, Dy


def border_margin(s):
    """The smallest (distance of px, py from the closed border and of cz from 0) / (its bound) over all pixels: above 1, `inside`
    is the same in fp32 and in fp64."""
    Ex, Ey, Ez, r64 = coordinate_error(s.depth, s.T, s.K, s.iK, s.eps)
    with np.errstate(all="ignore"):
        mx = np.minimum(np.abs(r64.px), np.abs(r64.px - (s.W - 1))) / Ex
        my = np.minimum(np.abs(r64.py), np.abs(r64.py - (s.H - 1))) / Ey
        mz = np.abs(r64.cz) / Ez
    return float(np.nanmin(np.minimum(np.minimum(mx, my), mz)))


# ---- shapes and inputs --------------------------------------------------------------------------------------------------------------------
WIDTHS, HEIGHTS = flowstage_ref.FV_WIDTHS, flowstage_ref.FV_HEIGHTS           # (1, 3, 4, 5, 63, 64, 65, 131) x (1, 2, 7)
SIZES = [(H, W) for H in HEIGHTS for W in WIDTHS]
BIG = (131, 77)


def pinhole(H, W):
    """(K, inv_K) fp32 [4,4]: the reference's normalised KITTI intrinsics scaled to the size, and their fp64 inverse rounded."""
    K = np.array([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64).astype(F32)
    return K, np.linalg.inv(K.astype(np.float64)).astype(F32)


def pose(axisangle, translation):
    """T fp32 [4,4] = translation after rotation (Rodrigues in fp64): transformation_from_parameters without invert."""
    a = np.asarray(axisangle, np.float64)
    th = np.linalg.norm(a)
    k = a / th if th > 0 else a
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T[:3, 3] = translation
    return T.astype(F32)


def scene(H, W, N=3, seed=0, aa=0.05, t=0.2, eps=EPS):
    """Depths in 0.1 .. 10, a pinhole K, small poses: a namespace depth [N,1,H,W], T [N,4,4], K, iK [4,4], eps.  Redrawn until no
    pixel's px, py or cz lies within its own error bound of where `inside` changes (border_margin)."""
    K, iK = pinhole(H, W)
    for attempt in range(50):
        rng = np.random.default_rng(7919 * H + 31 * W + 1000003 * seed + 15485867 * attempt)
        depth = rng.uniform(0.1, 10.0, (N, 1, H, W)).astype(F32)
        T = np.stack([pose(rng.uniform(-aa, aa, 3), rng.uniform(-t, t, 3)) for _ in range(N)])
        s = SimpleNamespace(depth=depth, T=T, K=K, iK=iK, eps=eps, H=H, W=W, N=N)
        if border_margin(s) > 1.0:
            return s
    raise RuntimeError("scene(%d, %d): no draw away from the border" % (H, W))


def measured(s, seed=0, sigma=0.3, alpha=ALPHA, beta=BETA, band=True):
    """A measured flow [N,2,H,W] fp32 for the scene: its rigid flow (0 where that is not finite) plus noise, a tenth of the pixels
    moved by (3, -2).  Redrawn until no judged pixel lies within max(BAND_UNITS, its own count) units of the threshold (band=False: the first draw,
    for inputs that are compared with the fp32 restatement only)."""
    base = np.nan_to_num(rigid(s.depth, s.T, s.K, s.iK, eps=s.eps, dtype=np.float64).rigid, nan=0.0, posinf=0.0, neginf=0.0)
    base = np.clip(base, -1e4, 1e4)
    for attempt in range(50):
        rng = np.random.default_rng(104729 * seed + 7919 * s.H + 31 * s.W + 1000003 * attempt + 17)
        flow = base + rng.standard_normal(base.shape) * sigma
        flow = np.where(rng.random((s.N, 1, s.H, s.W)) < 0.1, flow + np.array([3.0, -2.0])[None, :, None, None], flow).astype(F32)
        if not band or in_band(s, flow, alpha, beta) == 0:
            return flow
    raise RuntimeError("measured(%d, %d): no draw outside the band" % (s.H, s.W))


def in_band(s, flow, alpha=ALPHA, beta=BETA):
    r32 = rigid(s.depth, s.T, s.K, s.iK, flow, None, alpha, beta, s.eps)
    r64 = rigid(s.depth, s.T, s.K, s.iK, flow, None, alpha, beta, s.eps, np.float64)
    _, dist, count, _, _ = units(s, flow, r32, r64, alpha)
    return int((dist < np.maximum(BAND_UNITS, count)).sum())


def mask(H, W, N, seed=0):
    """A validity mask uint8 [N,H,W], about a fifth of it 0."""
    rng = np.random.default_rng(613 * H + W + 99991 * seed)
    return (rng.random((N, H, W)) >= 0.2).astype(np.uint8)


def sprinkle(t, values, seed):
    """A copy of t with an eighth of its elements (at least 3) replaced by `values` in turn."""
    t = t.copy()
    flat = t.reshape(-1)
    idx = np.random.default_rng(seed).permutation(flat.size)[:max(3, flat.size // 8)]
    flat[idx] = np.resize(np.array(values, F32), idx.size)
    return t


def edge(H, W):
    """N = 3: inv_K's first two columns are zero and K = I, so that every pixel's ray is (0, 0, 1) and px = tx / d, py = ty / d
    with tx = W - 1, ty = H - 1 and eps = 0.  Image 0: d = 1, every pixel lands exactly on (W - 1, H - 1) (inside: the border is
    closed); image 1: d = 1 - 2^-24, the correctly rounded quotient is one fp32 step past W - 1 and H - 1 (not inside, unless
    W = H = 1); image 2: d = 1 + 2^-23, just inside."""
    K = np.eye(4, dtype=F32)
    iK = np.zeros((4, 4), F32)
    iK[2, 2] = iK[3, 3] = 1
    T = np.eye(4, dtype=F32)
    T[0, 3], T[1, 3] = W - 1, H - 1
    depth = np.ones((3, 1, H, W), F32)
    depth[1], depth[2] = F32(1 - 2.0 ** -24), F32(1 + 2.0 ** -23)
    return SimpleNamespace(depth=depth, T=np.stack([T] * 3), K=K, iK=iK, eps=0.0, H=H, W=W, N=3)


def behind(H, W):
    """The camera moves 3 forward-to-backward through the depths 0.1 .. 10 (and a little sideways): part of every image has cz <= 0."""
    s = scene(H, W, seed=5)
    for n in range(s.N):
        s.T[n] = pose((0.0, 0.02 * n, 0.0), (0.05, 0.0, -3.0))
    return s


def cases(H, W):
    """[(name, scene, flow or None, valid or None, alpha, beta)] at one shape: the input families of the kernel tests.  N = 3."""
    out = []
    s = scene(H, W)
    flow, valid = measured(s), mask(H, W, s.N)
    out += [("rigid only", s, None, None, ALPHA, BETA), ("flow", s, flow, None, ALPHA, BETA), ("flow and valid", s, flow, valid, ALPHA, BETA),
            ("valid without flow", s, None, valid, ALPHA, BETA)]
    bad = scene(H, W, seed=1)
    bad.depth = sprinkle(bad.depth, [0.0, -1.5, np.nan, np.inf], 3 * H + W)
    out.append(("depths of 0, negative, NaN, inf", bad, measured(scene(H, W, seed=1)), valid, ALPHA, BETA))
    b = behind(H, W)
    out.append(("behind the camera", b, measured(b, sigma=0.5), None, ALPHA, BETA))
    e = edge(H, W)
    rng = np.random.default_rng(H + 7 * W)
    out.append(("edge", e, (rng.standard_normal((3, 2, H, W)) * 0.5).astype(F32) + np.array([W - 1, H - 1], F32)[None, :, None, None]
                - np.stack(np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32)), 0)[None], None, ALPHA, BETA))
    out.append(("NaN and inf flow", s, sprinkle(flow, [np.nan, np.inf, -np.inf], 5 * H + W), valid, ALPHA, BETA))
    other = scene(H, W, seed=2, eps=1e-3)
    out.append(("other alpha, beta, eps", other, measured(other, alpha=0.05, beta=0.25), None, 0.05, 0.25))
    zero = scene(H, W, seed=3, eps=0.0)
    out.append(("eps = 0", zero, measured(zero, alpha=0.0, beta=0.0), valid, 0.0, 0.0))
    return out


def run(case, dtype=F32):
    name, s, flow, valid, alpha, beta = case
    return rigid(s.depth, s.T, s.K, s.iK, flow, valid if flow is not None else None, alpha, beta, s.eps, dtype)


# ---- the scene: constant depth, a translation along x, and a square that moves on its own ----------------------------------------------
def translating_scene(H=24, W=40, top=8, left=10, size=8, shift=5):
    """Depth 4 everywhere, fx = fy = 32, the principal point at (16, 12), identity rotation, tx = 0.5, eps = 0: every quantity is a
    dyadic number, the rigid flow is fx * tx / d = (4, 0) EXACTLY.  The measured flow is the rigid flow except on a size x size
    square displaced by a further (+shift, 0).  (scene, flow, want_rigid [1,2,H,W], want_label [1,H,W])."""
    K = np.array([[32, 0, 16, 0], [0, 32, 12, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F32)
    iK = np.linalg.inv(K.astype(np.float64)).astype(F32)
    T = np.eye(4, dtype=F32)[None].copy()
    T[0, 0, 3] = 0.5
    s = SimpleNamespace(depth=np.full((1, 1, H, W), 4.0, F32), T=T, K=K, iK=iK, eps=0.0, H=H, W=W, N=1)
    want = np.zeros((1, 2, H, W), F32)
    want[:, 0] = 32 * 0.5 / 4.0
    flow = want.copy()
    flow[0, 0, top:top + size, left:left + size] += shift
    label = np.ones((1, H, W), np.uint8)
    label[0, top:top + size, left:left + size] = 2
    label[0, :, W - 4:] = 0                                    # x + 4 > W - 1: the point leaves the image, the pixel is not judged
    return s, flow, want, label


# ---- the fixture (tests/golden/rigidflow.npz): the reference's BackprojectDepth and Project3D on ten small scenes -------------------------
GOLDEN = [(2, 3), (7, 5), (7, 64), (7, 131), (2, 65), (3, 4), (7, 63), (5, 131), (2, 64), (7, 65)]       # H, W >= 2: it divides by W - 1
MIN_CZ = 0.05


def golden_key(H, W):
    return "%dx%d" % (H, W)


def golden_inputs(H, W):
    """(depth [1,1,H,W], axisangle [1,1,3], translation [1,1,3], K, inv_K [1,4,4]) fp32: depths in 0.1 .. 10, axis-angle up to 0.05,
    translation up to 0.2 (along z up to 0.04, so that cz stays above MIN_CZ at the nearest depths)."""
    rng = np.random.default_rng(15485863 + 7919 * H + 31 * W)
    depth = rng.uniform(0.1, 10.0, (1, 1, H, W)).astype(F32)
    aa = rng.uniform(-0.05, 0.05, (1, 1, 3)).astype(F32)
    tr = (rng.uniform(-0.2, 0.2, (1, 1, 3)) * np.array([1.0, 1.0, 0.2])).astype(F32)
    K, iK = pinhole(H, W)
    return depth, aa, tr, K[None], iK[None]
