"""Training-mode BatchNorm2d (+ residual, + ReLU, + the stem's max pool) GIVEN THE STATISTICS TABLE, restated.

Plain torch on the CPU, one function for every precision: `dtype=torch.float64` is the reference, `dtype=torch.float32` is the
calibration run -- the error that fp32 arithmetic of this formulation makes on the same inputs.  Nothing here uses autograd; the
backward is written out and the discontinuous decisions (ReLU mask, winning pool tap) are INPUTS of it.

The per-channel sums `stats` = [slots][G][2][C] (sum, sum of squares; fp32, as the convolution epilogue leaves them) are an exact
input and are never recomputed from y: the kernels form  var = max(s1/count - mean^2, 0)  from them, and at a large mean^2/var the
rounding of s1 to fp32 moves the variance by more than any tolerance, so a reference that recomputed it would disagree with a
correct kernel.  What this formulation loses is carried by the tolerance instead:

    kappa_c = 1 + (s1_c/count + mean_c^2) / (var_c + eps)         conditioning of invstd with respect to the two sums
    |got - ref64| <= K * 2^-24 * kappa_c * scale_c                 for every channel c          (check_channels)

with scale_c the channel's maximum of the output's own expression, every term replaced by its absolute value (fp64).

Tensors are NCHW ([B, C, H, W]); group g of G is the g-th slice of B/G images with row g of every [G][.][C] table.
"""
import math

import torch

EPS, MOMENTUM = 1e-5, 0.1
U = 2.0 ** -24

# --------------------------------------------------------------------------------------------------------------- calibration
# `python tests/bn_ref.py` runs the fp32 restatement against the fp64 one over every shape / mode below (the stem shapes too) and
# two summation orders of the channel sums ("seq": one accumulator; "pair64": sequential blocks of 64, then a pairwise tree) and
# prints the largest  err / (2^-24 * kappa * scale)  per family.  K = 4 x that ratio, never below 16; the factor 4 is for the
# kernels' different but equally legitimate roundings (FMA contraction, rsqrtf, v_rcp, the order of the atomics).
#
# Taken over ALL channels the ratio is not "in the tens": the bound is a first-order model, and three kinds of channel leave it.
#   * 2^-24 * kappa near 1 (mean 1e3 / std 1 at count = 4, where the sample variance happens to be 0.05; count == 1 at |y| = 1e3):
#     the fp32 variance is clamped to 0 while the fp64 one is not, invstd is off by its whole ratio to 1/sqrt(eps) (x 70), and
#     dy carries invstd cubed.
#   * count == 1: z = y * scale + shift is  beta  plus the cancellation of two terms of size |gamma y| / sqrt(eps), while the
#     scale of z is |beta| alone and kappa = 1 + 2 y^2 / eps is small for a small y.
#   * the constant channel: xhat = (y - mean) * invstd is pure rounding of the mean (1e-8 in fp64, 1e-7 in fp32), times 316.
# One K over everything would be 4.3e3 forward and 3.2e6 backward, and no mutant of tests/test_bn_ref_cpu.py could be told from
# rounding.  So each family records TWO values: K of the regular channels (count > 1 and kappa <= KAPPA_REG), which is the one
# that has teeth, and K of all channels -- the single K the procedure yields when read literally -- which bounds the rest.  No
# channel is judged by more than the literal K.
KAPPA_REG = 1e4
# measured ratios: (regular channels, all channels) for fwd / bwd, one value for the running statistics and the plain sums
#   fwd regular 4.00 (fin.mean, 24 slot copies)      all 1067 (z, count == 1, class 1)                     -> K 16 / 4269
#   bwd regular 3.18 (dgamma, C = 1024, M = 15)       all 7.94e5 (dy, class 4 at count = 4, clamped in fp32)  -> K 16 / 3.175e6
#   run 4.13 (running_mean, 24 slot copies) -> 16.5   sum 9.64 (sequential sum of 270 values of class 3) -> 38.6
# worst ratio per class (0 .. 7), fp32 restatement on the CPU:
#   fwd regular  4.0   3.35  3.55  2.8   -     -      -     -        (classes 4-7 have kappa > 1e4 throughout)
#   fwd all      208   1067  54    2.8   190   23.2   10.7  6.9      (classes 0-2: count == 1 only)
#   bwd regular  2.0   3.2   1.8   1.7   -     -      -     -
#   bwd all      2.0   3.2   1.8   1.7   7.9e5 6.7e3  149   2.2
#   run          2.6   3.7   3.7   2.0   4.1   2.2    1.9   2.2
# the kernels on an MI355X (tests/test_bn_edges_gpu.py prints them): regular 4.0 fwd / 2.8 bwd / 3.2 run / 4.2 sums; all
# channels 239 fwd (z, class 1 at count == 1) and 9.1e3 bwd (dy, class 4)
MEASURED = {"fwd": (3.998, 1067.0), "bwd": (3.183, 7.936e5), "run": 4.125, "sum": 9.64}
K = {"fwd": (16.0, 4269.0), "bwd": (16.0, 3.175e6), "run": 16.5, "sum": 38.6}

# (B, C, H, W, groups, slots, seeds): seeds = the class orders the case runs with (C = 4 holds only four classes at a time)
SHAPES = [
    (2, 16, 5, 7, 1, 1, (0,)),
    (2, 4, 5, 7, 1, 1, (0, 4)),
    (3, 8, 3, 5, 1, 2, (1,)),
    (3, 64, 9, 10, 1, 16, (2,)),
    (2, 64, 9, 10, 2, 17, (3,)),
    (4, 128, 3, 5, 2, 24, (4,)),
    (1, 1024, 3, 5, 1, 1, (5,)),
    (2, 1024, 2, 2, 2, 4, (6,)),
    (1, 16, 1, 1, 1, 1, (7,)),
    (2, 512, 1, 1, 2, 1, (8,)),
]
MODES = ("plain", "relu", "residual", "res_bn")
# (B, C, H, W, groups, seed)
STEM_SHAPES = [(1, 64, 15, 21, 1, 0), (2, 16, 9, 10, 2, 1), (3, 64, 3, 5, 1, 2), (2, 64, 2, 2, 2, 3), (1, 4, 7, 9, 1, 0)]
WELL = (0, 1, 2, 3)                                  # classes whose statistics are well conditioned


# ------------------------------------------------------------------------------------------------------------------- inputs
def channel_classes(C, seed=0, shift=0):
    """Class of every channel: (c + c // 8 + seed + shift) % 8 -- c % 8 in the first block of eight at seed 0; every later block is
    rotated by one, and the seed rotates all of them, so that every class meets every vector lane c % 4."""
    c = torch.arange(C)
    return (c + c // 8 + seed + shift) % 8


def make_y(B, C, H, W, seed, shift=0):
    """fp32 [B, C, H, W]; channel c drawn from its class:
        0  std 1, mean 0            1  std 1e-3 (var = 1e-6 < eps: eps decides)      2  std 1e3           3  mean 30
        4  mean 1e3, std 1          5  mean -3e2                                       6  constant 0.75 (var exactly 0)
        7  2 + 1e-4 * randn (the variance is lost in s1/count - mean^2; the clamp at 0 may hit)"""
    gen = torch.Generator().manual_seed(1000 + 17 * seed + shift)
    r = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
    std = torch.tensor([1.0, 1e-3, 1e3, 1.0, 1.0, 1.0, 0.0, 1e-4], dtype=torch.float64)
    mean = torch.tensor([0.0, 0.0, 0.0, 30.0, 1e3, -3e2, 0.75, 2.0], dtype=torch.float64)
    cls = channel_classes(C, seed, shift)
    return (r * std[cls][None, :, None, None] + mean[cls][None, :, None, None]).float()


def make_affine(C, seed, shift=0):
    """(gamma, beta, running_mean, running_var) fp32.  |gamma| is log-uniform in [1e-2, 1e2] with both signs, 1e2 and -1e-2 are
    present, and the first class-0 channel has gamma = beta = 0 exactly (its z is an exact zero: the ReLU mask's edge)."""
    gen = torch.Generator().manual_seed(2000 + 17 * seed + shift)
    mag = 10.0 ** (torch.rand(C, generator=gen, dtype=torch.float64) * 4 - 2)
    sign = torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0).double()
    gamma = (mag * sign).float()
    beta = (torch.rand(C, generator=gen) * 0.6 - 0.3).float()
    rm, rv = (torch.randn(C, generator=gen) * 0.1).float(), (torch.rand(C, generator=gen) + 0.5).float()
    cls = channel_classes(C, seed, shift)
    zero = int((cls == 0).nonzero()[0]) if bool((cls == 0).any()) else 0
    gamma[zero], beta[zero] = 0.0, 0.0
    gamma[(zero + 1) % C], gamma[(zero + 2) % C] = 1e2, -1e-2
    return gamma, beta, rm, rv


def stats_table(y, groups, slots=1):
    """fp32 [slots][G][2][C]: the fp64 sums of y per sub-batch, rounded; slots > 1: copies with unequal shares whose sum is that."""
    st = torch.stack([torch.stack([p.sum((0, 2, 3)), (p * p).sum((0, 2, 3))]) for p in y.double().chunk(groups, 0)])
    share = torch.linspace(0.5, 1.5, slots, dtype=torch.float64) if slots > 1 else torch.ones(1, dtype=torch.float64)
    return (st[None] * (share / share.sum())[:, None, None, None]).float()


# ------------------------------------------------------------------------------------------------------------------ helpers
def gcn(t, G):
    """[B, C, H, W] -> [G, C, rows of the group]"""
    B, C, H, W = t.shape
    return t.reshape(G, B // G, C, H * W).permute(0, 2, 1, 3).reshape(G, C, -1)


def ungcn(t, G, shape):
    B, C, H, W = shape
    return t.reshape(G, C, B // G, H * W).permute(0, 2, 1, 3).reshape(B, C, H, W)


def csum(t, order="seq"):
    """Sum over the last dimension in a stated order (it matters in fp32 only)."""
    n = t.shape[-1]
    if order == "seq":
        acc = torch.zeros_like(t[..., 0])
        for i in range(n):
            acc = acc + t[..., i]
        return acc
    assert order == "pair64", order
    nb = (n + 63) // 64
    x = torch.zeros(t.shape[:-1] + (nb * 64,), dtype=t.dtype)
    x[..., :n] = t
    x = csum(x.reshape(t.shape[:-1] + (nb, 64)), "seq")
    while x.shape[-1] > 1:
        if x.shape[-1] % 2:
            x = torch.cat([x, torch.zeros_like(x[..., :1])], -1)
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _amax(t):
    return t.abs().amax(-1)


# ------------------------------------------------------------------------------------------------------------------ forward
def finalize(stats, count, gamma, beta, eps=EPS, dtype=torch.float64, mutant=None):
    """The [G][4][C] table (scale, shift, mean, invstd) from the fp32 sums, plus what the checker needs (kappa, the absolute
    expressions).  The slot copies are added in order.  `mutant` (here and below) plants one named error: it exists for
    tests/test_bn_ref_cpu.py, which proves that the checker rejects each of them."""
    st = stats.reshape((-1,) + tuple(stats.shape[-3:])) if stats.dim() >= 3 else stats.reshape(1, 1, 2, -1)
    st = st.to(dtype)
    if mutant == "slots16":
        st = st[:16]
    cnt = torch.tensor(float(count) + (1.0 if mutant == "count+1" else 0.0), dtype=dtype)
    acc = st[0]
    for k in range(1, st.shape[0]):
        acc = acc + st[k]
    s0, s1 = acc[:, 0], acc[:, 1]
    g, b = gamma.to(dtype), beta.to(dtype)
    mean = s0 / cnt
    var = (s1 / cnt - mean * mean).clamp_min(0)            # biased, as used for normalisation
    nvar = var * cnt / (cnt - 1) if mutant == "unbiased_norm" else var
    e = {"no_eps": 0.0, "eps1e-6": 1e-6}.get(mutant, eps)
    invstd = 1 / torch.sqrt(nvar + torch.tensor(e, dtype=dtype))
    scale = g * invstd
    shift = b - mean * g * invstd
    t = dict(scale=scale, shift=shift, mean=mean, invstd=invstd, var=var, gamma=g, beta=b, count=float(count), G=st.shape[1])
    t["table"] = torch.stack([scale, shift, mean, invstd], 1)
    t["m2"] = s1 / cnt + mean * mean                       # |s1/count| + |mean^2|: the absolute expression of var
    t["kappa"] = 1 + t["m2"] / (var + eps)
    return t


def table_bounds(t):
    """(kappa, scale) of the four table rows, stacked as the table is: [G][4][C]."""
    one = torch.ones_like(t["kappa"])
    kap = torch.stack([t["kappa"], t["kappa"], one, t["kappa"]], 1)
    sc = torch.stack([t["gamma"].abs() * t["invstd"], t["beta"].abs() + (t["mean"] * t["gamma"]).abs() * t["invstd"],
                      t["mean"].abs(), t["invstd"]], 1)
    return kap, sc


def running(t, momentum, running_mean, running_var, mutant=None):
    """Running statistics after G successive momentum updates (unbiased variance; left unscaled at count == 1), with the absolute
    expressions of both as their scales."""
    dtype, cnt, G = t["mean"].dtype, t["count"], t["G"]
    rm, rv = running_mean.to(dtype), running_var.to(dtype)
    srm, srv = rm.abs(), rv.abs()
    f = cnt / (cnt - 1) if cnt > 1 else 1.0
    for g in range(1 if mutant == "momentum_once" else G):
        unb = t["var"][g] if mutant == "biased_running" else t["var"][g] * f
        rm = (1 - momentum) * rm + momentum * t["mean"][g]
        rv = (1 - momentum) * rv + momentum * unb
        srm = (1 - momentum) * srm + momentum * t["mean"][g].abs()
        srv = (1 - momentum) * srv + momentum * t["m2"][g] * f
    return dict(running_mean=rm, running_var=rv, scale_mean=srm, scale_var=srv)


def forward(y, stats, count, gamma, beta, eps, momentum, running_mean, running_var, relu, residual=None, res_table=None,
            dtype=torch.float64, mutant=None):
    """z = act(y * scale + shift [+ residual | + residual * rscale + rshift]) with scale / shift from `stats`; `res_table` = the
    residual's own finalize() result.  Returns z, the table (`tab`), the running statistics, G (what num_batches_tracked grows by)
    and the per-channel (kappa, scale) of z, both [G][C]."""
    t = finalize(stats, count, gamma, beta, eps, dtype, mutant)
    G = t["G"]
    yy = gcn(y.to(dtype), G)
    tz = t
    if mutant == "group0_table" and G > 1:
        tz = dict(t, scale=t["scale"][:1].expand(G, -1), shift=t["shift"][:1].expand(G, -1))
    z = yy * tz["scale"][..., None] + tz["shift"][..., None]
    kap = t["kappa"]
    sc = t["gamma"].abs()[None, :, None] * t["invstd"][..., None] * (yy - t["mean"][..., None]).abs() + t["beta"].abs()[None, :, None]
    if residual is not None:
        r = gcn(residual.to(dtype), G)
        if res_table is not None and mutant != "res_identity":
            z = z + (r * res_table["scale"][..., None] + res_table["shift"][..., None])
        else:
            z = z + r
        if res_table is not None:
            kap = torch.maximum(kap, res_table["kappa"])
            sc = sc + (res_table["gamma"].abs()[None, :, None] * res_table["invstd"][..., None]
                       * (r - res_table["mean"][..., None]).abs() + res_table["beta"].abs()[None, :, None])
        else:
            sc = sc + r.abs()
    pre = z
    if relu:
        z = z.clamp_min(0)
    out = dict(z=ungcn(z, G, y.shape), pre=ungcn(pre, G, y.shape), tab=t, G=G, kappa=kap.double(), scale=_amax(sc).double())
    if running_mean is not None:
        out.update(running(t, momentum, running_mean, running_var, mutant))
    return out


# ----------------------------------------------------------------------------------------------------------------- backward
def _bwd_core(du, y, t, order, mutant=None):
    """du, y: [G][C][M].  dy = gamma * invstd * (du - sum du / M - xhat * sum(du * xhat) / M), the two sums per group."""
    M = du.shape[-1]
    mean, invstd, g = t["mean"][..., None], t["invstd"][..., None], t["gamma"][None, :, None]
    xhat = (y - mean) * invstd
    sdu, sdx = csum(du, order), csum(du * xhat, order)
    term = xhat * sdx[..., None] / M
    if mutant == "no_xhat_term":
        term = torch.zeros_like(term)
    dy = g * invstd * (du - sdu[..., None] / M - term)
    a_du, a_dx = du.abs().sum(-1), (du * xhat).abs().sum(-1)
    return dict(dy=dy, dbeta=csum(sdu.transpose(0, 1), "seq"), dgamma=csum(sdx.transpose(0, 1), "seq"),
                scale_dy=_amax(g.abs() * invstd * (du.abs() + a_du[..., None] / M + xhat.abs() * a_dx[..., None] / M)).double(),
                scale_dbeta=a_du.sum(0).double(), scale_dgamma=a_dx.sum(0).double(), kappa=t["kappa"].double(),
                kappa_sum=t["kappa"].amax(0).double())


def backward(dz, mask, y, t, residual=None, res_table=None, dtype=torch.float64, order="seq", mutant=None):
    """Gradients of forward() for the cotangent dz; `mask` = the ReLU mask (bool [B, C, H, W]) or None without a ReLU.
    Returns dy, dgamma, dbeta, dres (residual given) and r_dy, r_dgamma, r_dbeta (the residual has its own table), each with
    its per-channel scale; `du` = dz * mask."""
    G = t["G"]
    du = dz.to(dtype) if mask is None else dz.to(dtype) * mask.to(dtype)
    out = {"du": du}
    main = _bwd_core(gcn(du, G), gcn(y.to(dtype), G), t, order, mutant)
    out.update(main)
    out["dy"] = ungcn(main["dy"], G, y.shape)
    if mutant == "swap_affine":
        out["dgamma"], out["dbeta"] = out["dbeta"], out["dgamma"]
    if residual is not None:
        out["dres"] = du
        out["scale_dres"] = _amax(gcn(du, G)).double()
        if res_table is not None:
            sub = _bwd_core(gcn(du, G), gcn(residual.to(dtype), G), res_table, order, mutant)
            out.update({"r_" + k: v for k, v in sub.items()})
            out["r_dy"] = ungcn(sub["dy"], G, y.shape)
    return out


# ---------------------------------------------------------------------------------------------------------------- stem tail
def _taps(H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    oy, ox = torch.arange(Ho)[:, None], torch.arange(Wo)[None, :]
    for tap in range(9):
        iy, ix = 2 * oy - 1 + tap // 3, 2 * ox - 1 + tap % 3
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        yield tap, iy.clamp(0, H - 1).expand(Ho, Wo), ix.clamp(0, W - 1).expand(Ho, Wo), ok.expand(Ho, Wo)


def window_values(z):
    """[9][B, C, Ho, Wo]: the values of the 3x3 stride-2 pad-1 windows in scan order, -inf outside the image."""
    out = []
    for tap, iy, ix, ok in _taps(z.shape[2], z.shape[3]):
        v = z[:, :, iy, ix]
        out.append(torch.where(ok[None, None], v, torch.full_like(v, -math.inf)))
    return torch.stack(out)


def max_pool(z):
    """(pooled [B, C, Ho, Wo], index uint8 [B, Ho, Wo, C]) of the 3x3 stride-2 pad-1 max pool: FIRST maximum in scan order."""
    w = window_values(z)
    best, idx = w[0].clone(), torch.zeros(w[0].shape, dtype=torch.uint8)
    for tap in range(1, 9):
        better = w[tap] > best
        best = torch.where(better, w[tap], best)
        idx = torch.where(better, torch.full_like(idx, tap), idx)
    return best, idx.permute(0, 2, 3, 1).contiguous()


def pool_gather(dpool, idx, shape, dtype):
    """The pool's input gradient [B, C, H, W]: every pooled pixel hands its cotangent to the tap its index byte names."""
    dz = torch.zeros(shape, dtype=dtype)
    ix8 = idx.permute(0, 3, 1, 2).long()
    dp = dpool.to(dtype)
    for tap, iy, ix, ok in _taps(shape[2], shape[3]):
        b, c, oy, ox = ((ix8 == tap) & ok[None, None]).nonzero(as_tuple=True)
        dz.index_put_((b, c, iy[oy, ox], ix[oy, ox]), dp[b, c, oy, ox], accumulate=True)
    return dz


def stem_forward(y, stats, count, gamma, beta, eps, momentum, running_mean, running_var, dtype=torch.float64, mutant=None):
    """relu(bn(y)) and its 3x3 stride-2 pad-1 max pool (first maximum in scan order)."""
    out = forward(y, stats, count, gamma, beta, eps, momentum, running_mean, running_var, True, dtype=dtype, mutant=mutant)
    out["pooled"], out["idx"] = max_pool(out["z"])
    return out


def stem_backward(dpool, idx, dz_extra, mask, y, t, dtype=torch.float64, order="seq", mutant=None):
    """Backward of the stem tail: the pool gradient gathered through the given index bytes, plus an optional second cotangent on
    z, then backward()."""
    dz = pool_gather(dpool, idx, y.shape, dtype)
    if dz_extra is not None:
        dz = dz + dz_extra.to(dtype)
    return backward(dz, mask, y, t, dtype=dtype, order=order, mutant=mutant)


# ------------------------------------------------------------------------------------------------------------------ checker
def _gc(t, like):
    """A result next to its [G'][C] bound, as [G', C, n]: [C] -> [1, C, 1]; [G, C] -> [G, C, 1]; [B, C, H, W] -> gcn."""
    if t.dim() == 4:
        return gcn(t, like.shape[0])
    return t[None, :, None] if t.dim() == 1 else t[..., None]


def channel_ratios(got, ref64, kappa, scale):
    """[G'][C]: the channel's max |got - ref64| over 2^-24 * kappa * scale (0 where the error vanishes, inf where only the
    bound does or the result is not finite)."""
    scale = torch.as_tensor(scale, dtype=torch.float64)
    kappa = torch.as_tensor(kappa, dtype=torch.float64)
    if scale.dim() == 1:
        scale = scale.reshape(1, -1)
    kappa = kappa.reshape(1, -1) if kappa.dim() == 1 else kappa
    g, r = _gc(got.detach().cpu().double(), scale), _gc(ref64.double(), scale)
    assert g.shape == r.shape, (g.shape, r.shape)
    err = (g - r).abs().amax(-1)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (U * kappa * scale))
    return torch.where(torch.isfinite(g).all(-1), ratio, torch.full_like(ratio, math.inf))


def worst_per_class(ratio, classes):
    return {int(k): float(ratio[:, classes == k].max()) for k in classes.unique()}


def check_channels(name, got, ref64, kappa, scale, K, classes=None):
    """Every channel c: max |got - ref64| <= K * 2^-24 * kappa_c * scale_c and every value finite (K: a number, or one per channel).
    Prints the worst ratio per class; returns the worst ratio / K."""
    ratio = channel_ratios(got, ref64, kappa, scale)
    if classes is not None:
        print("%-16s err / (2^-24 kappa scale), worst per class: %s" % (
            name, "  ".join("%d: %.3g" % kv for kv in sorted(worst_per_class(ratio, classes).items()))))
    Kt = torch.as_tensor(K, dtype=torch.float64).expand_as(ratio)
    over = ratio / Kt
    if bool((over > 1).any()):
        g, c = divmod(int(over.argmax()), over.shape[1])
        raise AssertionError("%s: %d channel(s) over their bound; worst: group %d channel %d%s at ratio %.4g against K = %g" % (
            name, int((over > 1).sum()), g, c, "" if classes is None else " (class %d)" % int(classes[c]), float(ratio[g, c]),
            float(Kt[g, c])))
    return float(over.max())


# -------------------------------------------------------------------------------------------------------------------- cases
def make_case(B, C, H, W, groups, slots, seed, mode):
    """Everything one bn_act case reads.  mode: plain | relu | residual | res_bn (the last three end in a ReLU).  In res_bn the
    residual has its own class assignment (shifted by three channels), affine parameters and statistics."""
    c = dict(shape=(B, C, H, W), G=groups, slots=slots, seed=seed, mode=mode, relu=mode != "plain", count=(B // groups) * H * W,
             classes=channel_classes(C, seed), rclasses=None, y=make_y(B, C, H, W, seed), residual=None, res=None)
    c["stats"] = stats_table(c["y"], groups, slots)
    c["gamma"], c["beta"], c["rm"], c["rv"] = make_affine(C, seed)
    c["dz"] = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(3000 + seed))
    if mode in ("residual", "res_bn"):
        c["residual"] = make_y(B, C, H, W, seed, shift=3)
        c["rclasses"] = channel_classes(C, seed, 3)
    if mode == "res_bn":
        g, b, rm, rv = make_affine(C, seed, shift=3)
        c["res"] = dict(stats=stats_table(c["residual"], groups, 1)[0], gamma=g, beta=b, rm=rm, rv=rv)
    return c


def run_forward(c, dtype=torch.float64, mutant=None):
    """forward() of a case; with res_bn also r_tab (the residual's table) and the residual's running statistics."""
    rt = None
    if c["res"] is not None:
        r = c["res"]
        rt = finalize(r["stats"], c["count"], r["gamma"], r["beta"], EPS, dtype, mutant)
    out = forward(c["y"], c["stats"], c["count"], c["gamma"], c["beta"], EPS, MOMENTUM, c["rm"], c["rv"], c["relu"], c["residual"], rt,
                  dtype=dtype, mutant=mutant)
    if rt is not None:
        out["r_tab"] = rt
        out.update({"r_" + k: v for k, v in running(rt, MOMENTUM, c["res"]["rm"], c["res"]["rv"], mutant).items()})
    return out


def run_backward(c, fwd, mask, dtype=torch.float64, order="seq", mutant=None):
    return backward(c["dz"], mask, c["y"], fwd["tab"], c["residual"], fwd.get("r_tab"), dtype=dtype, order=order, mutant=mutant)


def fwd_tensors(out):
    """The comparable tensors of a restatement's forward output (a kernel run is asked for the same)."""
    got = dict(z=out["z"], table=out["tab"]["table"], running_mean=out["running_mean"], running_var=out["running_var"])
    if "r_tab" in out:
        got.update(r_table=out["r_tab"]["table"], r_running_mean=out["r_running_mean"], r_running_var=out["r_running_var"])
    return got


def forward_items(got, ref):
    """(name, got, ref64, kappa, scale, family, the kappa that decides the channel's tier) of every forward quantity in `got`:
    z, table, running_mean, running_var [, r_table, r_running_mean, r_running_var]."""
    items = [("z", got["z"], ref["z"], ref["kappa"], ref["scale"], "fwd", ref["kappa"])] if "z" in got else []
    for pre in ("", "r_"):
        if pre + "table" not in got:
            continue
        t = ref[pre + "tab"]
        kap, sc = table_bounds(t)
        for row, nm in enumerate(("scale", "shift", "mean", "invstd")):
            items.append((pre + "fin." + nm, got[pre + "table"][:, row], t["table"][:, row], kap[:, row], sc[:, row], "fwd", t["kappa"]))
        if pre + "running_mean" in got:
            items.append((pre + "running_mean", got[pre + "running_mean"], ref[pre + "running_mean"], 1.0, ref[pre + "scale_mean"],
                          "run", None))
            items.append((pre + "running_var", got[pre + "running_var"], ref[pre + "running_var"], 1.0, ref[pre + "scale_var"],
                          "run", None))
    return items


def backward_items(got, ref):
    """The same for dy, dgamma, dbeta [, dres, r_dy, r_dgamma, r_dbeta]."""
    items = []
    for pre in ("", "r_"):
        if pre + "dy" not in got:
            continue
        ks = ref[pre + "kappa_sum"]
        items.append((pre + "dy", got[pre + "dy"], ref[pre + "dy"], ref[pre + "kappa"], ref[pre + "scale_dy"], "bwd", ref[pre + "kappa"]))
        items.append((pre + "dgamma", got[pre + "dgamma"], ref[pre + "dgamma"], ks, ref[pre + "scale_dgamma"], "bwd", ks))
        items.append((pre + "dbeta", got[pre + "dbeta"], ref[pre + "dbeta"], 1.0, ref[pre + "scale_dbeta"], "bwd", ks))
    if "dres" in got:
        items.append(("dres", got["dres"], ref["dres"], 1.0, ref["scale_dres"], "bwd", ref["kappa"]))
    return items


def regular(tier_kappa, count):
    """[G'][C] bool: the channels of the regular tier."""
    tk = torch.as_tensor(tier_kappa, dtype=torch.float64)
    tk = tk.reshape(1, -1) if tk.dim() == 1 else tk
    return (tk <= KAPPA_REG) & (count > 1)


def tier_K(fam, tier_kappa, count):
    """The K of every channel: the regular tier's where count > 1 and kappa <= KAPPA_REG, the family's all-channel K elsewhere."""
    k = K[fam]
    if not isinstance(k, tuple):
        return torch.tensor(float(k), dtype=torch.float64)
    return torch.where(regular(tier_kappa, count), torch.tensor(float(k[0]), dtype=torch.float64),
                       torch.tensor(float(k[1]), dtype=torch.float64))


def check_items(items, count, classes, rclasses=None, prefix=""):
    """check_channels over a list of items, each channel with the recorded K of its family and tier; the worst ratio / K."""
    worst = 0.0
    for name, g, r, kap, sc, fam, tk in items:
        cls = rclasses if (name.startswith("r_") and rclasses is not None) else classes
        worst = max(worst, check_channels(prefix + name, g, r, kap, sc, tier_K(fam, tk, count), cls))
    return worst


def undecided(ref, count):
    """(share, decided): the share of the elements of channels with kappa <= 1e3 whose |z64| -- before the ReLU clamps it, so
    that a safely negative element counts as decided -- is below the forward bound: the ones whose ReLU mask the bound leaves
    open; and the [B, C, H, W] mask of the elements of ALL channels above it."""
    G = ref["G"]
    bound = (tier_K("fwd", ref["kappa"], count) * U * ref["kappa"] * ref["scale"])[..., None]
    under = gcn(ref["pre"], G).double().abs() < bound
    sel = (ref["kappa"] <= 1e3)[..., None].expand_as(under)
    share = float(under[sel].double().mean()) if bool(sel.any()) else 0.0
    return share, ungcn(~under, G, ref["z"].shape)


def sum_ratios(y, G, order):
    """fp32 channel sums of y and y^2 in `order` against the fp64 sums: (ratio over 2^-24 sum|y|, ratio over 2^-24 sum y^2)."""
    yy = gcn(y, G)
    y64 = yy.double()
    return (channel_ratios(csum(yy, order), y64.sum(-1), 1.0, y64.abs().sum(-1)),
            channel_ratios(csum(yy * yy, order), (y64 * y64).sum(-1), 1.0, (y64 * y64).sum(-1)))


def stem_case(B, C, H, W, G, seed):
    c = make_case(B, C, H, W, G, 1, seed, "relu")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    c["dpool"] = torch.randn(B, C, Ho, Wo, generator=torch.Generator().manual_seed(4000 + seed))
    c["args"] = (c["y"], c["stats"], c["count"], c["gamma"], c["beta"], EPS, MOMENTUM, c["rm"], c["rv"])
    return c


def measure(verbose=True):
    """Largest err / (2^-24 kappa scale) of the fp32 restatement against the fp64 one, per family and tier, over SHAPES x MODES
    and the stem shapes, both summation orders: {"fwd": [regular, all], "bwd": [regular, all], "run": [all], "sum": [all]}."""
    worst, where = {"fwd": [0.0, 0.0], "bwd": [0.0, 0.0], "run": [0.0], "sum": [0.0]}, {}

    def note(items, tag, count):
        for name, g, r, kap, sc, fam, tk in items:
            ra = channel_ratios(g, r, kap, sc)
            assert bool(torch.isfinite(ra).all()), (tag, name)
            tiers = [torch.ones_like(ra, dtype=torch.bool)]
            if len(worst[fam]) == 2:
                tiers = [regular(tk, count).expand_as(ra), tiers[0]]
            for i, sel in enumerate(tiers):
                v = float(ra[sel].max()) if bool(sel.any()) else 0.0
                if v > worst[fam][i]:
                    worst[fam][i], where[fam, i] = v, (tag, name)

    for B, C, H, W, G, slots, seeds in SHAPES:
        for seed in seeds:
            for mode in MODES:
                c = make_case(B, C, H, W, G, slots, seed, mode)
                ref, f32 = run_forward(c), run_forward(c, torch.float32)
                tag = (B, C, H, W, G, slots, seed, mode)
                note(forward_items(fwd_tensors(f32), ref), tag, c["count"])
                mask = (f32["z"] > 0) if c["relu"] else None
                rb = run_backward(c, ref, mask)
                for order in ("seq", "pair64"):
                    note(backward_items(run_backward(c, f32, mask, torch.float32, order), rb), tag + (order,), c["count"])
            for order in ("seq", "pair64"):
                for r in sum_ratios(make_y(B, C, H, W, seed), G, order):
                    if float(r.max()) > worst["sum"][0]:
                        worst["sum"][0], where["sum", 0] = float(r.max()), ((B, C, H, W, G, seed), order)
    for shape in STEM_SHAPES:
        c = stem_case(*shape)
        ref, f32 = stem_forward(*c["args"]), stem_forward(*c["args"], dtype=torch.float32)
        tag = ("stem",) + tuple(shape)
        note(forward_items(fwd_tensors(f32), ref), tag, c["count"])
        mask = f32["z"] > 0
        rb = stem_backward(c["dpool"], f32["idx"], c["dz"], mask, c["y"], ref["tab"])
        for order in ("seq", "pair64"):
            got = stem_backward(c["dpool"], f32["idx"], c["dz"], mask, c["y"], f32["tab"], torch.float32, order)
            note(backward_items(got, rb), tag + (order,), c["count"])
    if verbose:
        for fam in worst:
            for i, v in enumerate(worst[fam]):
                print("%-4s %-8s worst ratio %.4g at %s -> K = %.4g" % (fam, ("regular", "all")[i] if len(worst[fam]) == 2 else "all", v,
                                                                        where.get((fam, i)), max(16.0, 4 * v)))
    return worst


if __name__ == "__main__":
    measure()
