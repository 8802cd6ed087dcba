"""The on-the-fly correlation block on the GPU (altcorr_* kernels of csrc/corr.hip, raft_corr.AlternateCorrBlock).

It is the function CorrBlock computes (pooling is linear), so the truth and the bound are those of test_corr_gpu.py: the fixture
recorded from the reference's own CorrBlock and tests/corr_ref.py in fp64; bound = 3 x the largest error of corr_ref's fp32 run
against its fp64 run on the same inputs, never below 2 ulp of the largest |value| (corr_ref.check), per level.  What the
reference leaves at exactly zero must be exactly zero.  Where the (h*w)^2 volume does not fit, the windowed restatement
tests/altcorr_ref.py takes corr_ref's place under the same rule.

Outputs and dfmap1 have one owner per element and repeat bit for bit; dfmap2 is summed with float atomics and is only held to
the bound."""
import functools

import pytest
import torch

import altcorr_ref as A
import corr_ref as R
from conftest import load_golden
from corr_ref import check, make_case, reference

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def run_gpu(dev, f1, f2, coords, douts, L, r, cl_in=False, cl_out=False, cls="AlternateCorrBlock"):
    from deep_visual_slam_amd import raft_corr
    place = lambda t: (t.to(dev).contiguous(memory_format=CL) if cl_in else t.to(dev).contiguous()).requires_grad_(True)
    g1, g2 = place(f1.float()), place(f2.float())
    block = getattr(raft_corr, cls)(g1, g2, num_levels=L, radius=r)
    outs = [block(c.float().to(dev), memory_format=CL if cl_out else None) for c in coords]
    for o in outs:
        assert tuple(o.shape) == (f1.shape[0], L * (2 * r + 1) ** 2) + tuple(f1.shape[2:])
        assert o.is_contiguous(memory_format=CL if cl_out else torch.contiguous_format)
    d1, d2 = torch.autograd.grad(outs, [g1, g2], [(d.float().to(dev).contiguous(memory_format=CL) if cl_out else d.float().to(dev))
                                                  for d in douts])
    torch.cuda.synchronize()
    return block, outs, d1, d2


@functools.lru_cache(maxsize=None)
def case(B, Cn, H, W, L, r, n_lookups=1, seed=0):
    """(inputs, {dtype: (outs, dfmap1, dfmap2)}) of corr_ref: computed once, shared, never modified."""
    inputs = make_case(B, Cn, H, W, L, r, n_lookups=n_lookups, seed=seed)
    return inputs, reference(*inputs, L, r)


def check_all(name, got, ref, L, r):
    """Outputs per level and both gradients of one run against corr_ref's fp64 run, bound from its fp32 run."""
    _, outs, d1, d2 = got
    (o64, a64, b64), (o32, a32, b32) = ref[torch.float64], ref[torch.float32]
    for k, o in enumerate(outs):
        for i, sl in enumerate(R.level_slices(L, r)):
            check("%s lookup %d level %d" % (name, k, i), o[:, sl], o64[k][:, sl], o32[k][:, sl])
            zero = o64[k][:, sl] == 0
            if zero.any():
                assert float(o[:, sl].detach().cpu()[zero].abs().max()) == 0.0, "zero padding must be exact (%s level %d)" % (name, i)
    check(name + " dfmap1", d1, a64, a32)
    check(name + " dfmap2", d2, b64, b32)


# ---- the fixture -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fix():
    rec = load_golden("corr_b2_c24_17x23.npz")
    t = lambda k: torch.from_numpy(rec[k])
    B, Cn, H, W, L, r = (int(v) for v in rec["meta/shape"])
    f1, f2, coords, dout = t("in/fmap1"), t("in/fmap2"), [t("in/coords0"), t("in/coords1")], t("in/dout")
    ref = {}
    for dt in (torch.float64, torch.float32):
        outs, g1, g2 = R.grads(f1.to(dt), f2.to(dt), coords, [dout, dout], L, r)
        ref[dt] = dict(outs=outs, g1=g1, g2=g2, levels=R.level_grads(f1.to(dt), f2.to(dt), coords, [dout, dout], L, r))
    return dict(rec=rec, f1=f1, f2=f2, coords=coords, dout=dout, L=L, r=r, ref=ref)


def test_fixture_forward_per_level(gpu_device, fix):
    _, outs, _, _ = run_gpu(gpu_device, fix["f1"], fix["f2"], fix["coords"], [fix["dout"]] * 2, fix["L"], fix["r"])
    r64, r32 = fix["ref"][torch.float64], fix["ref"][torch.float32]
    for k, o in enumerate(outs):
        want = torch.from_numpy(fix["rec"]["ref/out%d" % k])
        for i, sl in enumerate(R.level_slices(fix["L"], fix["r"])):
            # compared with the fixture; the third argument makes the bound 3 x |corr_ref fp32 - corr_ref fp64| of this level
            w = want[:, sl].double()
            check("lookup %d level %d vs the reference" % (k, i), o[:, sl], w, r32["outs"][k][:, sl] - r64["outs"][k][:, sl] + w)
            zero = want[:, sl] == 0
            assert zero.any()
            assert float(o[:, sl].detach().cpu()[zero].abs().max()) == 0.0, "zero padding must be exact (lookup %d level %d)" % (k, i)


def test_fixture_gradients(gpu_device, fix):
    _, _, d1, d2 = run_gpu(gpu_device, fix["f1"], fix["f2"], fix["coords"], [fix["dout"]] * 2, fix["L"], fix["r"])
    r64, r32 = fix["ref"][torch.float64], fix["ref"][torch.float32]
    for name, got, key in (("dfmap1", d1, "g1"), ("dfmap2", d2, "g2")):
        want = torch.from_numpy(fix["rec"]["ref/" + name]).double()
        check(name + " vs the reference", got, want, r32[key] - r64[key] + want)


def test_fixture_gradients_per_level(gpu_device, fix):
    """The cotangent restricted to one level's channels at a time, against corr_ref in fp64."""
    r64, r32 = fix["ref"][torch.float64], fix["ref"][torch.float32]
    for i, sl in enumerate(R.level_slices(fix["L"], fix["r"])):
        m = torch.zeros_like(fix["dout"])
        m[:, sl] = fix["dout"][:, sl]
        _, _, d1, d2 = run_gpu(gpu_device, fix["f1"], fix["f2"], fix["coords"], [m, m], fix["L"], fix["r"])
        check("level %d dfmap1" % i, d1, r64["levels"][i][0], r32["levels"][i][0])
        check("level %d dfmap2" % i, d2, r64["levels"][i][1], r32["levels"][i][1])


# ---- the kernels' edges: the pixel tile of 32, the channel chunk of 64, the radius ---------------------------------------------
EDGES = [
    # name, B, C, H, W, levels, radius, channels_last inputs, channels_last output and cotangent
    ("n63_one_level_r0", 1, 8, 3, 21, 1, 0, False, False),
    ("n63_one_level_r0_cl", 1, 8, 3, 21, 1, 0, True, True),
    ("n64_two_tiles", 2, 4, 8, 8, 2, 2, True, False),
    ("n65_one_past_the_tile", 1, 36, 5, 13, 2, 2, False, True),
    ("17x23_cl", 2, 24, 17, 23, 4, 3, True, True),
    ("17x23_nchw", 2, 24, 17, 23, 4, 3, False, False),
    ("c4", 1, 4, 16, 16, 4, 3, False, False),
    ("c36_below_a_chunk", 2, 36, 17, 15, 3, 2, True, True),
    ("c68_chunk_and_a_tail", 1, 68, 8, 9, 2, 2, False, True),
    ("c128_two_chunks", 1, 128, 16, 17, 4, 3, False, True),
    ("c256_four_chunks_one_level_r4", 1, 256, 16, 16, 1, 4, True, False),
    ("33x31_c36_r4", 3, 36, 33, 31, 4, 4, True, False),
    ("33x31_r4_nchw", 1, 36, 33, 31, 4, 4, False, True),
]


@pytest.mark.parametrize("edge", EDGES, ids=[c[0] for c in EDGES])
def test_edges_against_fp64(gpu_device, edge):
    name, B, Cn, H, W, L, r, cl_in, cl_out = edge
    (f1, f2, coords, douts), ref = case(B, Cn, H, W, L, r)
    check_all(name, run_gpu(gpu_device, f1, f2, coords, douts, L, r, cl_in, cl_out), ref, L, r)


def test_both_forms_agree_on_the_gpu(gpu_device):
    """AlternateCorrBlock against CorrBlock: each is within its bound of fp64, so they differ by at most the sum of the bounds."""
    B, Cn, H, W, L, r = 2, 36, 17, 23, 4, 3
    (f1, f2, coords, douts), ref = case(B, Cn, H, W, L, r, 2, 7)
    alt = run_gpu(gpu_device, f1, f2, coords, douts, L, r)
    allp = run_gpu(gpu_device, f1, f2, coords, douts, L, r, cls="CorrBlock")
    r64, r32 = ref[torch.float64], ref[torch.float32]
    triples = [(alt[2], allp[2], r64[1], r32[1], "dfmap1"), (alt[3], allp[3], r64[2], r32[2], "dfmap2")]
    for k in range(2):
        for i, sl in enumerate(R.level_slices(L, r)):
            triples.append((alt[1][k][:, sl], allp[1][k][:, sl], r64[0][k][:, sl], r32[0][k][:, sl], "lookup %d level %d" % (k, i)))
    for a, b, w64, w32, name in triples:
        diff, bnd = float((a.detach().double() - b.detach().double()).abs().max()), R.bound(w64, w32)
        print("%s: |alternate - all-pairs| %.3e, 2 x bound %.3e" % (name, diff, 2 * bnd))
        assert diff <= 2 * bnd, (name, diff, bnd)


# ---- past the all-pairs form's limit ---------------------------------------------------------------------------------------
def test_a_map_whose_volume_does_not_fit(gpu_device):
    """184 x 256: (h*w)^2 = 2.2e9 >= 2^31.  CorrBlock refuses it; the on-the-fly form runs it.  corr_ref cannot build that volume
    either, so the windowed restatement is the truth here: fp64 for the values, its fp32 run for the bound."""
    from deep_visual_slam_amd import raft_corr
    from deep_visual_slam_amd._lib import DvsError
    B, Cn, H, W, L, r = 1, 8, 184, 256, 4, 2
    f1, f2, coords, douts = make_case(B, Cn, H, W, L, r, seed=13, sigma=3.0)
    with pytest.raises(DvsError, match=r"2\^31"):
        raft_corr.CorrBlock(f1.to(gpu_device), f2.to(gpu_device), num_levels=L, radius=r)
    ref = {dt: A.grads(f1.to(dt), f2.to(dt), coords, douts, L, r) for dt in (torch.float64, torch.float32)}
    check_all("184x256", run_gpu(gpu_device, f1, f2, coords, douts, L, r), ref, L, r)


# ---- memory: a condition, not a measurement --------------------------------------------------------------------------------
def test_nothing_of_the_volume_s_size_is_allocated(gpu_device):
    """Two lookups forward and backward at 48 x 64 stay below a quarter of the all-pairs pyramid (which that form allocates twice:
    the pyramid and its gradient).  What this form needs: two outputs of 2.4 MB, the pooled rows, the position-major copies of
    NCHW maps (0.8 MB), and per lookup backward three feature-map-sized gradients plus autograd's sums -- 8.0 MB measured."""
    from deep_visual_slam_amd import raft_corr
    B, Cn, H, W, L, r = 1, 32, 48, 64, 4, 3
    f1, f2, coords, douts = make_case(B, Cn, H, W, L, r, n_lookups=2, seed=17)
    g1, g2 = f1.to(gpu_device).requires_grad_(True), f2.to(gpu_device).requires_grad_(True)
    cc, dd = [c.to(gpu_device) for c in coords], [d.to(gpu_device) for d in douts]
    limit = raft_corr.pyramid_bytes(B, H, W, L) // 4
    assert limit == 12533760
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    block = raft_corr.AlternateCorrBlock(g1, g2, num_levels=L, radius=r)
    outs = [block(c) for c in cc]
    d1, d2 = torch.autograd.grad(outs, [g1, g2], dd)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise %.2f MB, limit %.2f MB, altcorr_bytes %.2f MB" % (rise / 1e6, limit / 1e6,
                                                                        raft_corr.altcorr_bytes(B, Cn, H, W, L, r) / 1e6))
    assert rise < limit, (rise, limit)
    assert torch.isfinite(d1).all() and torch.isfinite(d2).all()


# ---- N lookups on one block: autograd sums their gradients ---------------------------------------------------------------------
def test_six_lookups_on_one_block(gpu_device):
    B, Cn, H, W, L, r, n = 1, 32, 32, 48, 4, 4, 6
    (f1, f2, coords, douts), ref = case(B, Cn, H, W, L, r, n, 5)
    check_all("six lookups", run_gpu(gpu_device, f1, f2, coords, douts, L, r), ref, L, r)


def test_outputs_and_dfmap1_repeat_bit_for_bit(gpu_device):
    """dfmap2 is summed with float atomics: both runs must be within the bound of fp64, bit equality is not asked of it."""
    (f1, f2, coords, douts), ref = case(2, 36, 17, 23, 4, 3, 2, 7)
    runs = [run_gpu(gpu_device, f1, f2, coords, douts, 4, 3) for _ in range(2)]
    for a, b in zip(runs[0][1] + [runs[0][2]], runs[1][1] + [runs[1][2]]):
        assert torch.equal(a, b)
    for k, run in enumerate(runs):
        check("run %d dfmap2" % k, run[3], ref[torch.float64][2], ref[torch.float32][2])


def test_precision_mode_does_not_reach_the_block(gpu_device):
    from deep_visual_slam_amd import _lib
    (f1, f2, coords, douts), _ = case(1, 128, 16, 17, 4, 3)
    want = run_gpu(gpu_device, f1, f2, coords, douts, 4, 3)
    _lib.set_precision("bf16")
    try:
        got = run_gpu(gpu_device, f1, f2, coords, douts, 4, 3)
    finally:
        _lib.set_precision("fp32")
    assert torch.equal(got[1][0], want[1][0]) and torch.equal(got[2], want[2])


def test_unsupported_inputs_raise(gpu_device):
    from deep_visual_slam_amd import raft_corr
    from deep_visual_slam_amd._lib import DvsError
    z = lambda *s, **k: torch.zeros(*s, device=gpu_device, **k)
    with pytest.raises(DvsError, match="fp32"):
        raft_corr.AlternateCorrBlock(z(1, 8, 16, 16, dtype=torch.float16), z(1, 8, 16, 16, dtype=torch.float16))
    with pytest.raises(DvsError, match="multiple of 4"):
        raft_corr.AlternateCorrBlock(z(1, 6, 16, 16), z(1, 6, 16, 16))
    with pytest.raises(DvsError, match="fewer than 2"):
        raft_corr.AlternateCorrBlock(z(1, 8, 15, 16), z(1, 8, 15, 16))
    with pytest.raises(DvsError, match="differ"):
        raft_corr.AlternateCorrBlock(z(1, 8, 16, 16), z(1, 8, 16, 20))
    block = raft_corr.AlternateCorrBlock(z(1, 8, 16, 16), z(1, 8, 16, 16))
    with pytest.raises(DvsError, match="raft.py:101"):
        block(z(1, 2, 16, 16).requires_grad_(True))
