"""CPU-side checks of the forward-backward consistency mask (csrc/flowcons.hip, raft_video.flow_consistency): the NumPy restatement
of tests/flowcons_ref.py against what the reference's own bilinear_sampler returned (tests/golden/flowcons.npz), its fp32 form
against its fp64 form, the occluder scene, and what can be checked of the entry without a device: the header declares it, the
binding lists it, the ABI is still 12, and every argument error is raised before any launch."""
import os
import re

import numpy as np
import pytest
import torch

import flowcons_ref as R
from conftest import ROOT, load_golden

FIXTURE = "flowcons.npz"
U = 2.0 ** -24            # the relative error of one fp32 operation


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


# ---- 1. the gather against the reference's bilinear_sampler -------------------------------------------------------------------------
GOLDEN = [(H, W, s) for H, W in R.GOLDEN_SIZES for s in R.GOLDEN_SCALES]


@pytest.mark.parametrize("H,W,scale", GOLDEN, ids=["%dx%d_%g" % c for c in GOLDEN])
def test_gather_is_the_reference_bilinear_sampler(rec, H, W, scale):
    """bu, bv of the restatement against bilinear_sampler(b, coords_grid + a, mask=True) on the pixels the reference's own mask
    marks strictly inside.  The two differ by the reference's round trip through normalised coordinates:

        t = 2 q / (W - 1) in 0 .. 2 (the division: <= U * 2), t - 1 (<= U / 2 * 2), grid_sample's (t' + 1) (<= U * 2), / 2 (exact),
        * (W - 1) (<= U * q), so that its pixel coordinate is off by at most (W - 1) / 2 * 2.5 U * 2 / 2 ... in all
        |dqx| <= 2.25 U (W - 1), |dqy| <= 2.25 U (H - 1)

    (about an ulp of the coordinate), which moves a bilinear sample by at most |dqx| Dx + |dqy| Dy, Dx / Dy the largest difference
    of horizontally / vertically adjacent elements of the sampled plane (the slope of a bilinear patch is bounded by its edges'
    and the interpolant is continuous across cells); each side's own interpolation is 6 roundings on terms that sum to at most
    max|p|.  bound = 2.25 U ((W - 1) Dx + (H - 1) Dy) + 12 U max|p|.
    Measured maximum over the ten cases: 0.12 of the bound (7x131 at scale 3: 3.3e-5 against 2.6e-4)."""
    k = R.golden_key(H, W, scale)
    a, b = rec[k + "/a"], rec[k + "/b"]
    want_a, want_b = (t[:1] for t in R.noise(H, W, scale))
    assert np.array_equal(R.bits(a), R.bits(want_a)) and np.array_equal(R.bits(b), R.bits(want_b))    # the seeded inputs stand
    r = R.direction(a, b)
    strict = rec[k + "/mask"].astype(bool)
    assert strict.shape == r.inside.shape and not (strict & ~r.inside).any()         # strictly inside implies inside
    worst = 0.0
    for plane, got in ((0, r.bu), (1, r.bv)):
        p = b[:, plane].astype(np.float64)
        Dx = np.abs(np.diff(p, axis=2)).max() if W > 1 else 0.0
        Dy = np.abs(np.diff(p, axis=1)).max() if H > 1 else 0.0
        bound = 2.25 * U * ((W - 1) * Dx + (H - 1) * Dy) + 12 * U * np.abs(p).max()
        err = np.abs(got.astype(np.float64) - rec[k + "/out"][:, plane])[strict]
        if err.size:
            print("%s plane %d: %d pixels, error %.3e, bound %.3e" % (k, plane, err.size, err.max(), bound))
            assert err.max() <= bound
            worst = max(worst, err.max() / bound)
    print("%s: %.2f of the bound" % (k, worst))


# ---- 2. fp32 against fp64 ---------------------------------------------------------------------------------------------------------------
FAMILIES = [(H, W) for H in R.HEIGHTS for W in (1, 5, 64, 131)] + [R.BIG]


@pytest.mark.parametrize("H,W", FAMILIES, ids=["%dx%d" % s for s in FAMILIES])
def test_fp32_restatement_against_fp64(H, W):
    """|excess32 - excess64| per pixel in units of 2^-23 (d + thr), against the count flowcons_ref.units derives from the
    operation count (3 + 6 A units, A the cancellation in sx = a.u + bu); no pixel of any case lies within max(16, its count)
    units of the threshold, so the two masks must be EQUAL and the comparison excuses nothing.
    Measured over these cases: at most 10.6 units (131x77; at most 0.57 of a pixel's own count), the nearest pixel 23.9 units
    from the threshold (7x131)."""
    worst = (0.0, 0.0, np.inf)
    for name, a, b in R.cases(H, W):
        if name == "special":                                                # NaN / inf: covered by the exact GPU comparison
            continue
        for r32, r64 in zip(R.consistency(a, b), R.consistency(a, b, dtype=np.float64)):
            assert r32.excess.dtype == np.float32 and r64.excess.dtype == np.float64
            assert np.array_equal(r32.inside, r64.inside)
            err, dist, count = R.units(r32, r64)
            near = int((dist < np.maximum(R.BAND_UNITS, count)).sum())
            ratio = float((err / np.maximum(count, 1e-300)).max())
            print("%dx%d %s: error %.2f units (%.2f of the count), nearest pixel %.1f units from the threshold, %d in the band"
                  % (H, W, name, err.max(), ratio, dist.min(), near))
            assert near == 0, name
            assert (err <= count).all(), name
            assert np.array_equal(r32.valid, r64.valid), name
            assert np.array_equal(np.isinf(r32.excess), np.isinf(r64.excess))
            worst = (max(worst[0], float(err.max())), max(worst[1], ratio), min(worst[2], float(dist.min())))
    print("%dx%d: worst error %.2f units, %.2f of the count, nearest %.1f units" % ((H, W) + worst))


def test_families_cover_valid_invalid_and_outside():
    """The inputs do what they are for: everything valid ... mostly outside, the closed border, the step past it, NaN and inf."""
    H, W = 7, 64
    by = {name: R.consistency(a, b) for name, a, b in R.cases(H, W)}
    share = lambda r: float(r.valid.mean())
    assert share(by["noise0.01"][0]) > 0.6 and 0 < (1 - by["noise0.01"][0].valid).sum()
    assert by["noise30"][0].inside.mean() < 0.5
    assert 0.0 < share(by["noise0.7"][0]) < 1.0 and 0.0 < share(by["smooth"][0]) < 1.0
    for r in by["zero"]:
        assert r.valid.all() and (r.excess == np.float32(-0.5)).all()          # border included
    assert by["edge"][0].inside.all() and not by["outside"][0].inside.any()
    assert np.isposinf(by["outside"][0].excess).all() and not by["outside"][0].valid.any()
    a, b = R.cases(H, W)[-1][1:]
    bad = ~np.isfinite(a).all(axis=1)
    assert bad.any() and np.isposinf(by["special"][0].excess[bad]).all() and not by["special"][0].valid[bad].any()
    for r in by["special"]:
        assert not np.isnan(r.excess).any()


# ---- 3. the occluder scene ----------------------------------------------------------------------------------------------------------------
def test_occluder_scene():
    a, b, want, want_bw = R.occluder()
    assert (1 - want).sum() == 5 * 8 and (1 - want_bw).sum() == 5 * 8
    fw, bw = R.consistency(a, b)
    assert np.array_equal(fw.valid, want) and np.array_equal(bw.valid, want_bw)
    assert fw.inside.all() and bw.inside.all()
    # integer flows, so every sample is a tap: background 0 - 0.5, the square 0 - (0.01 * 50 + 0.5), occluded 25 - (0.01 * 25 + 0.5)
    f = np.float32
    assert set(np.unique(fw.excess)) == {f(-0.5), f(0) - (f(0.01) * f(50) + f(0.5)), f(25) - (f(0.01) * f(25) + f(0.5))}


# ---- 4. header, binding, ABI, refusals ----------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry(built):
    src = open(os.path.join(ROOT, "include", "dvslam.h")).read()
    m = re.search(r"\bint\s+dvs_flow_consistency\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    assert m and m.group(1).count(",") + 1 == 18
    assert "dvs_flow_consistency" in built.exported_symbols() and len(built._SIGNATURES["dvs_flow_consistency"][1]) == 18
    assert hasattr(built.lib(), "dvs_flow_consistency")
    assert "thr = alpha*m + beta" in src and "x1 = min(x0+1, W-1)" in src             # the arithmetic is stated
    assert "Meister" in open(os.path.join(ROOT, "PAPERS.md")).read()


def test_abi_is_still_12(built):
    assert built.ABI_VERSION == 12 and built.lib().dvs_abi_version() == 12


P = 4096          # a non-NULL, 16-byte aligned "device pointer": nothing dereferences it before the checks fail


def _entry(l, a=P, a_image=70, a_plane=35, a_row=7, b=2 * P, b_image=70, b_plane=35, b_row=7, va=3 * P, vb=4 * P, ea=5 * P, eb=6 * P,
           N=2, H=5, W=7, alpha=0.01, beta=0.5):
    return l.dvs_flow_consistency(a, a_image, a_plane, a_row, b, b_image, b_plane, b_row, va, vb, ea, eb, N, H, W, alpha, beta, None)


BAD_CALLS = [
    ("NULL a", dict(a=None)),
    ("NULL b", dict(b=None)),
    ("misaligned a", dict(a=P + 2)),
    ("misaligned b", dict(b=P + 1)),
    ("misaligned excess", dict(eb=6 * P + 2)),
    ("N = 0", dict(N=0)),
    ("N = 65536", dict(N=65536)),
    ("H = 0", dict(H=0)),
    ("W = -1", dict(W=-1)),
    ("W past 2^24", dict(W=(1 << 24) + 1, H=1, a_row=1 << 25, a_plane=1 << 25, a_image=1 << 26, b_row=1 << 25, b_plane=1 << 25,
                         b_image=1 << 26)),
    ("too many lanes", dict(H=1 << 24, W=1 << 24, a_row=1 << 24, b_row=1 << 24)),
    ("a row stride < W", dict(a_row=6)),
    ("b row stride < W", dict(b_row=6)),
    ("a plane stride < the plane", dict(a_plane=34)),
    ("b image stride < two planes", dict(b_image=69)),
    ("stride out of range", dict(a_row=1 << 41, a_plane=1 << 45, a_image=1 << 47)),
    ("alpha < 0", dict(alpha=-0.01)),
    ("alpha NaN", dict(alpha=float("nan"))),
    ("beta inf", dict(beta=float("inf"))),
]


@pytest.mark.parametrize("name,kw", BAD_CALLS, ids=[b[0] for b in BAD_CALLS])
def test_entry_refuses_bad_arguments(built, name, kw):
    l = built.lib()
    assert _entry(l, **kw) == -1                     # DVS_ERR_INVALID: no launch was tried (this machine has no GPU to refuse one)
    assert b"dvs_flow_consistency" in l.dvs_last_error()


def test_messages_say_what_is_wrong_and_no_output_is_no_launch(built):
    l = built.lib()
    assert _entry(l, a_row=6) < 0 and b"a row stride 6 is below W=7" in l.dvs_last_error()
    assert _entry(l, b_image=69) < 0 and b"b image stride 69 is below" in l.dvs_last_error()
    assert _entry(l, va=None, vb=None, ea=None, eb=None) == 0               # nothing to write: returns before any launch


def test_flow_consistency_input_errors(built):
    from deep_visual_slam_amd import raft_video
    E = built.DvsError
    f = torch.zeros(2, 5, 7)
    with pytest.raises(E, match="flow_consistency: flow_fw: GPU tensors only .* no CPU path"):
        raft_video.flow_consistency(f, f)
    meta = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="meta")
    with pytest.raises(E, match="GPU tensors only"):
        raft_video.flow_consistency(meta(2, 5, 7), meta(2, 5, 7))
    import inspect
    params = inspect.signature(raft_video.flow_consistency).parameters
    assert list(params) == ["flow_fw", "flow_bw", "alpha", "beta", "excess"]
    assert (params["alpha"].default, params["beta"].default, params["excess"].default) == (0.01, 0.5, False)


class _Stand:
    """What gpu_arg reads of a tensor (is_cuda, dtype, dim(), shape, device): a GPU tensor's stand-in on a machine without one."""

    def __init__(self, shape, dtype=torch.float32, device="cuda:0"):
        self.shape, self.dtype, self.device, self.is_cuda = torch.Size(shape), dtype, torch.device(device), True

    def dim(self):
        return len(self.shape)

    def detach(self):
        return self


def test_flow_consistency_refuses_mismatches_before_any_launch(built, monkeypatch):
    """Shape, device and dtype mismatches between the two flows, and bad thresholds: raised by the argument checks, which read
    nothing but the tensors' descriptions."""
    from deep_visual_slam_amd import raft_video
    E = built.DvsError
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (_Stand, torch.Tensor)))
    monkeypatch.setattr(raft_video._lib, "lib", lambda: pytest.fail("the library was reached"))
    ok = _Stand((2, 2, 5, 7))
    for other, msg in ((_Stand((2, 2, 5, 8)), r"flow_fw \(2, 2, 5, 7\) on cuda:0, flow_bw \(2, 2, 5, 8\) on cuda:0"),
                       (_Stand((1, 2, 5, 7)), r"flow_bw \(1, 2, 5, 7\)"),
                       (_Stand((2, 2, 5, 7), device="cuda:1"), r"flow_bw \(2, 2, 5, 7\) on cuda:1"),
                       (_Stand((2, 2, 5, 7), dtype=torch.float64), r"flow_bw: fp32 only, got torch.float64"),
                       (_Stand((2, 3, 5, 7)), r"flow_bw: \[2,H,W\] or \[N,2,H,W\] expected, got \(2, 3, 5, 7\)"),
                       (_Stand((5, 7)), r"expected, got \(5, 7\)")):
        with pytest.raises(E, match=msg):
            raft_video.flow_consistency(ok, other)
    for kw in (dict(alpha=-1.0), dict(beta=float("nan")), dict(alpha=float("inf"))):
        with pytest.raises(E, match="must be finite and not negative"):
            raft_video.flow_consistency(ok, _Stand((2, 2, 5, 7)), **kw)


def test_stream_and_model_signatures(built):
    """The keywords of the issue, after the existing ones; a frame of a one-directional stream has the new fields, as None."""
    import inspect
    from deep_visual_slam_amd import raft, raft_video
    params = inspect.signature(raft_video.FlowStream.__init__).parameters
    assert list(params)[11:] == ["bidirectional", "fb_alpha", "fb_beta"]
    assert (params["bidirectional"].default, params["fb_alpha"].default, params["fb_beta"].default) == (False, 0.01, 0.5)
    frame = raft_video.FlowFrame(None, None, None)
    assert (frame.flow_low_bw, frame.flow_up_bw, frame.valid, frame.valid_bw) == (None, None, None, None)
    with pytest.raises(built.DvsError, match="host=True only"):
        frame.valid_host
    with pytest.raises(built.DvsError, match="fb_alpha"):
        raft_video.FlowStream(raft.SmallRAFT(), fb_alpha=-1.0)
    for cls in (raft.RAFT, raft.SmallRAFT):
        want = list(inspect.signature(cls.refine).parameters)
        assert list(inspect.signature(cls.refine_pair).parameters) == want
        assert inspect.signature(cls.refine_pair).parameters["iters"].default == 12
    model = raft.SmallRAFT().eval()
    with pytest.raises(built.DvsError, match=r"SmallRAFT.refine_pair: feat1.fmap: GPU tensors only"):
        model.refine_pair(object(), object())
