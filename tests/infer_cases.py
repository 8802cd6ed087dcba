"""Inference conv epilogue cases: conv2d_forward with a folded-BatchNorm bias, the BasicBlock identity and a ReLU in the
epilogue, one case per launch regime of csrc/conv_fwd.hip.

Under eval() + no_grad, nn_ops.conv_bn_act calls conv.conv2d_forward(x, w_f, b_f, ..., act="relu", residual=identity).  What
runs then depends on the tile arithmetic of launch_mode / launch_dma: the LDS-DMA kernel with the epilogue in the kernel
(conv_epilogue_body<..., ACT, RES>), the same kernel split over K (splitk_zero_kernel -> atomics -> splitk_finish_kernel), the
register-staged kernel (Cin % 32 != 0, the bf16 mode), or the generic planar kernel with the input normalisation folded in
(the stem, which leaves stem_fwd as soon as it has a bias or an activation).

  ROWS                     the case table (tests/test_inference_kernels_gpu.py runs it against fp64)
  regime(row, ...)         the launch a row gets, restated from the C++ as plain arithmetic; tests/test_inference_cpu.py
                           asserts that every row lands in the regime its id names
  combos(row)              the epilogue combinations (bias, residual, relu) a row runs
  inputs(row) / reference  seeded CPU operands and the fp64 torch composition act(conv(x, w) + bias + residual)

A plain module (imported like guard and conv_cases), not a conftest.
"""
import collections
import itertools
import re

import torch
import torch.nn.functional as F

BK = 32                 # csrc/conv_common.h: channels of one K stage
SPLITK_TILES = 320      # csrc/conv_fwd.hip launch_dma: sk_tiles, fewer tiles split K ...
SPLITK_FEW = 200        # ... towards 256 workgroups below this many tiles, towards 1024 from it on
TILE128_MIN = 448       # csrc/conv_fwd.hip launch_mode: fewer 128-row tiles take the 64 x 128 configuration

Row = collections.namedtuple("Row", "id B ci co k s H W planar combo all7 bf16 kernel tile tiles ksplit")
# combo = (bias, residual, relu) of the product's call; all7: also every other non-empty combination; bf16: also in the bf16 mode
_P, _E, _D = (1, 1, 1), (1, 0, 1), (1, 0, 0)        # BasicBlock tail, a stage's conv1 / the stem, the downsample branch
ROWS = [
    #   id               B  ci   co   k  s  H    W    planar combo all7  bf16   kernel    tile        tiles ksplit
    Row("l1_split2",     1, 64,  64,  3, 1, 9,   13,  False, _P, True,  True,  "dma",    (128, 64),  1,    2),
    Row("l3_split8",     1, 256, 256, 3, 1, 5,   7,   False, _P, False, True,  "dma",    (64, 128),  2,    8),
    Row("l4_split16_b3", 3, 512, 512, 3, 1, 3,   5,   False, _P, False, False, "dma",    (64, 128),  4,    16),
    Row("split_t1024",   1, 128, 512, 3, 1, 56,  57,  False, _P, False, False, "dma",    (64, 128),  200,  4),
    Row("edge_316",      1, 64,  512, 3, 1, 70,  72,  False, _P, False, False, "dma",    (64, 128),  316,  2),
    Row("edge_320",      1, 64,  512, 3, 1, 71,  72,  False, _P, True,  True,  "dma",    (64, 128),  320,  1),
    Row("tile128",       1, 32,  512, 3, 1, 120, 120, False, _P, False, False, "dma",    (128, 128), 452,  1),
    Row("nc1",           3, 32,  64,  3, 1, 9,   13,  False, _P, False, False, "dma",    (128, 64),  3,    1),
    Row("cout96",        1, 64,  96,  3, 1, 9,   13,  False, _P, False, False, "dma",    (64, 128),  2,    2),
    Row("buf_odd",       3, 20,  36,  3, 1, 11,  17,  False, _P, True,  False, "buf",    (128, 64),  5,    1),
    Row("buf_48",        1, 48,  64,  3, 1, 11,  17,  False, _P, False, True,  "buf",    (128, 64),  2,    1),
    Row("s2_entry",      1, 64,  128, 3, 2, 15,  21,  False, _E, False, True,  "dma",    (64, 128),  2,    2),
    Row("ds_1x1",        1, 64,  128, 1, 2, 15,  21,  False, _D, False, True,  "dma",    (64, 64),   4,    2),
    Row("stem3",         1, 3,   64,  7, 2, 38,  50,  True,  _E, False, False, "planar", (128, 64),  4,    1),
    Row("stem6",         3, 6,   64,  7, 2, 37,  259, True,  _E, False, True,  "planar", (128, 64),  58,   1),
]
BY_ID = {r.id: r for r in ROWS}


def pad(row):
    return row.k // 2


def out_hw(row):
    p = pad(row)
    return (row.H + 2 * p - row.k) // row.s + 1, (row.W + 2 * p - row.k) // row.s + 1


def rows_m(row):
    ho, wo = out_hw(row)
    return row.B * ho * wo


# ---------------------------------------------------------------------------------------------- the launch arithmetic
def _cdiv(a, b):
    return -(-a // b)


def launch(M, ci, co, k, planar=False, precision="fp32", deterministic=False):
    """(kernel, (BM, BN), tiles, ksplit) of a forward launch without a statistics epilogue, M output rows.
    csrc/conv_fwd.hip: launch_mode picks the tile, launch_cfg / dma_eligible the kernel, launch_dma the K split."""
    if co > 64:                                             # launch_mode
        t64, t128 = _cdiv(M, 64) * _cdiv(co, 128), _cdiv(M, 128) * _cdiv(co, 128)
        rounds, full = t128 / 512.0, _cdiv(t128, 512)
        tail_waste = rounds <= 3.2 and (full - rounds) / full > 0.2
        if k == 1 and t64 < 224:                            # gemm_small (the statistics form does not apply here)
            tile = (64, 64)
        else:
            tile = (64, 128) if (t128 < TILE128_MIN or tail_waste) else (128, 128)
    else:
        tile = (128, 64) if co > 32 else (128, 32)
    tiles = _cdiv(M, tile[0]) * _cdiv(co, tile[1])
    if planar:                                              # launch_cfg: IN_PLANAR is always register-staged
        return "planar", tile, tiles, 1
    if precision == "bf16" or ci % BK or k > 3:             # launch_cfg (bf16 tiles) / dma_eligible
        return "buf", tile, tiles, 1
    ksplit, nc = 1, ci // BK                                # launch_dma
    if not deterministic and tiles < SPLITK_TILES and nc >= 2 and co % 4 == 0:
        target = 256 if tiles < SPLITK_FEW else 1024
        want = min(nc, _cdiv(target, tiles))
        per = _cdiv(nc, want)
        ksplit = _cdiv(nc, per)
    return "dma", tile, tiles, ksplit


def regime(row, precision="fp32", deterministic=False):
    return launch(rows_m(row), row.ci, row.co, row.k, row.planar, precision, deterministic)


def id_claims(row):
    """What a row's id says about its launch, as {field: value} (parsed from the id, not from the table)."""
    out = {}
    m = re.search(r"split(\d+)", row.id)
    if m:
        out["ksplit"] = int(m.group(1))
    m = re.match(r"edge_(\d+)", row.id)
    if m:
        out["tiles"] = int(m.group(1))
    if row.id == "tile128":
        out["tile"] = (128, 128)
    if row.id.startswith("buf_"):
        out["kernel"] = "buf"
    if row.id.startswith("stem"):
        out["kernel"] = "planar"
    return out


# ---------------------------------------------------------------------------------------------- epilogues and operands
ALL7 = [c for c in itertools.product((0, 1), repeat=3) if any(c)]


def combos(row):
    """The product's combination first; rows marked all7 run every non-empty subset of {bias, residual, relu}."""
    return [row.combo] + ([c for c in ALL7 if c != row.combo] if row.all7 else [])


def combo_id(c):
    return "".join(n for n, on in zip(("b", "r", "a"), c) if on)


def stem_norm(cin, dyadic):
    """Per-channel (in_scale, in_shift) of the stem's folded input normalisation.  dyadic (the bf16 mode): powers of two and
    multiples of 1/4, so that x * scale is exact and x * scale + shift rounds once whether or not the compiler contracts it to
    an fma -- the bf16 rounding of the operand is then the same in the kernel and in the specification."""
    c = torch.arange(cin, dtype=torch.float32)
    if dyadic:
        return 2.0 ** (c % 3 + 1), -(c % 4) * 0.25 - 0.5
    return (1.0 + 0.1 * c) / 0.225, -0.45 / 0.225 - 0.05 * c


def inputs(row, seed=0, dyadic=False):
    """Seeded CPU operands of a row: x (NCHW; the kernels take NHWC memory, the stem planar), w scaled by sqrt(2 / (Cin k k)),
    bias, a unit-scale residual (it changes the sign of a large share of the outputs) and the stem's normalisation or None."""
    g = torch.Generator().manual_seed(seed + 1000 * ROWS.index(row))
    ho, wo = out_hw(row)
    x = torch.randn(row.B, row.ci, row.H, row.W, generator=g)
    w = torch.randn(row.co, row.ci, row.k, row.k, generator=g) * (2.0 / (row.ci * row.k * row.k)) ** 0.5
    b = torch.randn(row.co, generator=g) * 0.5
    r = torch.randn(row.B, row.co, ho, wo, generator=g)
    return x, w, b, r, (stem_norm(row.ci, dyadic) if row.planar else None)


def conv_reference(row, x, w, norm, spec=None):
    """fp64 conv2d(x, w) of a row (the stem: of the normalised image).  spec: the operand rounding of the bf16 mode, applied to
    w and to the tensor the kernel multiplies (x, for the stem the normalised image in fp32)."""
    if norm is not None:
        sc, sh = (t.double()[None, :, None, None] for t in norm)
        x = x.double() * sc + sh
        if spec is not None:
            x = x.float()                           # the fp32 value of the fold (one rounding: see stem_norm)
    spec = spec or (lambda t: t.double())
    return F.conv2d(spec(x), spec(w), None, row.s, pad(row))


def epilogue(y, b, r, combo):
    """fp64: act(y + bias + residual) -- bias and residual INSIDE the activation; neither is rounded in the bf16 mode."""
    has_b, has_r, relu = combo
    if has_b:
        y = y + b.double()[None, :, None, None]
    if has_r:
        y = y + r.double()
    return F.relu(y) if relu else y


def reference(row, x, w, b, r, norm, combo, spec=None):
    return epilogue(conv_reference(row, x, w, norm, spec), b, r, combo)


# ---------------------------------------------------------------------------------------------- BasicBlock groups (part B)
Block = collections.namedtuple("Block", "id ci co s H W relu residual res_bn")
BLOCKS = [
    Block("plain",    64, 64,  1, 12, 20, True,  False, False),
    Block("residual", 128, 128, 1, 6,  10, True,  True,  False),
    Block("res_bn",   64, 128, 2, 13, 17, True,  True,  True),       # stride 2 + 1x1 downsample: output 7 x 9
    Block("norelu",   64, 64,  1, 17, 23, False, False, False),
]
STEMS = [(1, 3, 38, 50), (3, 6, 37, 259)]
