"""CPU-side checks of the rigid flow and the moving-object label (csrc/rigidflow.hip, raft_video.rigid_flow): the NumPy restatement
of tests/rigidflow_ref.py against what the reference's own BackprojectDepth and Project3D returned (tests/golden/rigidflow.npz), its
fp32 form against its fp64 form, the translating scene, and what can be checked of the entry without a device: the header declares
it, the binding lists it, the ABI is still 12, and every argument error is raised before any launch."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import rigidflow_ref as R
from conftest import ROOT, load_golden

FIXTURE = "rigidflow.npz"


@pytest.fixture(scope="module")
def rec():
    return load_golden(FIXTURE)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from deep_visual_slam_amd import _lib
    return _lib


# ---- 1. the geometry against the reference's BackprojectDepth and Project3D -----------------------------------------------------------
@pytest.mark.parametrize("H,W", R.GOLDEN, ids=["%dx%d" % s for s in R.GOLDEN])
def test_restatement_is_the_reference_view_synthesis(rec, H, W):
    """px, py of the restatement against Project3D(BackprojectDepth(depth, inv_K), K, T) in pixels, on EVERY pixel (the fixture's
    smallest cz is above rigidflow_ref.MIN_CZ, asserted where it is made and here), within rigidflow_ref.fixture_bound: twice the
    operation-count bound E through the partial derivatives of cx / den (the two sides may sum in different orders) plus the
    reference's normalise round trip, about an ulp of the coordinate.
    Measured maximum over the ten cases: 0.052 of the bound (5x131, whose largest error is 3.7e-5 of a pixel)."""
    k = R.golden_key(H, W)
    depth, K, iK, T, pix = (rec[k + "/" + name] for name in ("depth", "K", "inv_K", "T", "pix"))
    want = R.golden_inputs(H, W)
    for got, w in ((depth, want[0]), (K, want[3]), (iK, want[4])):
        assert np.array_equal(R.bits(got), R.bits(w))                                  # the seeded inputs stand
    assert T.dtype == np.float32 and T.shape == (1, 4, 4) and pix.dtype == np.float64 and pix.shape == (1, 2, H, W)
    r = R.rigid(depth, T, K, iK)
    assert float(r.cz.min()) > R.MIN_CZ
    bx, by = R.fixture_bound(depth, T, K, iK)
    ex, ey = np.abs(r.px.astype(np.float64) - pix[:, 0]), np.abs(r.py.astype(np.float64) - pix[:, 1])
    assert ex.shape == (1, H, W) and np.isfinite(ex).all() and np.isfinite(ey).all()   # no pixel is left out
    share = max(float((ex / bx).max()), float((ey / by).max()))
    print("%s: %d pixels, errors %.3e / %.3e, %.3f of the bound" % (k, ex.size, ex.max(), ey.max(), share))
    assert (ex <= bx).all() and (ey <= by).all()
    # and the rigid flow is that coordinate minus the pixel's own
    x, y = np.arange(W, dtype=np.float32)[None, None, :], np.arange(H, dtype=np.float32)[None, :, None]
    assert np.array_equal(R.bits(r.ru), R.bits(r.px - x)) and np.array_equal(R.bits(r.rv), R.bits(r.py - y))


# ---- 2. fp32 against fp64 ---------------------------------------------------------------------------------------------------------------
FAMILIES = [(H, W) for H in R.HEIGHTS for W in (1, 5, 64, 131)] + [R.BIG]


@pytest.mark.parametrize("H,W", FAMILIES, ids=["%dx%d" % s for s in FAMILIES])
def test_fp32_restatement_against_fp64(H, W):
    """The same formulas in fp64 from the fp32 inputs.  |ru32 - ru64| <= D per pixel and |excess32 - excess64| <= its count of
    units of 2^-23 (e2 + thr), both from the operation count (rigidflow_ref's docstring).  No pixel's px, py or cz lies within
    its bound of the border (scene redraws) and no pixel within max(16, its count) units of the threshold (measured redraws), so
    `inside` and the labels must be EQUAL and the comparison excuses nothing.
    Measured over these cases: rigid at most 0.16 of D (7x131), excess at most 0.15 of a pixel's own count (7x131; the count is
    dominated by 2 |ex| D, the rigid flow's own error, and runs to thousands of units where the flow is large); the nearest pixel
    954 units from the threshold (7x64)."""
    worst = [0.0, 0.0, 0.0, np.inf]
    for seed, (alpha, beta, eps) in enumerate(((R.ALPHA, R.BETA, R.EPS), (0.05, 0.25, 1e-3), (0.0, 0.0, 0.0))):
        s = R.scene(H, W, seed=seed, eps=eps)
        flow = R.measured(s, seed, alpha=alpha, beta=beta)
        valid = R.mask(H, W, s.N, seed) if seed == 1 else None
        r32 = R.rigid(s.depth, s.T, s.K, s.iK, flow, valid, alpha, beta, eps)
        r64 = R.rigid(s.depth, s.T, s.K, s.iK, flow, valid, alpha, beta, eps, np.float64)
        assert r32.excess.dtype == np.float32 and r64.excess.dtype == np.float64 and r32.ru.dtype == np.float32
        err, dist, count, Dx, Dy = R.units(s, flow, r32, r64, alpha)
        assert np.isfinite(r64.ru).all() and np.isfinite(r64.rv).all()
        eu, ev = np.abs(r32.ru.astype(np.float64) - r64.ru), np.abs(r32.rv.astype(np.float64) - r64.rv)
        share = max(float((eu / Dx).max()), float((ev / Dy).max()))
        near = int((dist < np.maximum(R.BAND_UNITS, count)).sum())
        ratio = float((err / np.maximum(count, 1e-300)).max())
        print("%dx%d seed %d: rigid %.2f of D, excess %.2f units (%.2f of the count), nearest pixel %.1f units from the threshold, "
              "%d judged of %d" % (H, W, seed, share, err.max(), ratio, dist.min(), int(r64.judged.sum()), r64.judged.size))
        assert (eu <= Dx).all() and (ev <= Dy).all()
        assert np.array_equal(r32.inside, r64.inside)
        assert near == 0 and (err <= count).all()
        assert np.array_equal(r32.label, r64.label)
        assert np.array_equal(np.isinf(r32.excess), np.isinf(r64.excess))
        worst = [max(worst[0], share), max(worst[1], float(err.max())), max(worst[2], ratio), min(worst[3], float(dist.min()))]
    print("%dx%d: rigid %.2f of D, excess %.2f units, %.2f of the count, nearest %.1f units" % ((H, W) + tuple(worst)))


def test_families_cover_static_moving_outside_and_behind():
    """The inputs do what they are for."""
    H, W = 7, 64
    by = {c[0]: (c, R.run(c)) for c in R.cases(H, W)}
    assert len(by) == 10
    flow = by["flow"][1]
    assert set(np.unique(flow.label)) == {0, 1, 2} and (flow.label == 1).sum() > (flow.label == 2).sum() > 0
    masked, valid = by["flow and valid"][1], by["flow and valid"][0][3]
    assert (masked.label[valid == 0] == 0).all() and np.isposinf(masked.excess[valid == 0]).all()
    assert np.array_equal(masked.label[valid != 0], flow.label[valid != 0])
    assert not hasattr(by["rigid only"][1], "label") and not hasattr(by["valid without flow"][1], "label")
    bad, depth = by["depths of 0, negative, NaN, inf"][1], by["depths of 0, negative, NaN, inf"][0][1].depth[:, 0]
    for kind in (depth == 0, depth < 0, np.isnan(depth), np.isposinf(depth)):
        assert kind.any()
    assert (R.bits(bad.ru[np.isnan(depth)]) == R.QNAN).all() and (bad.label[np.isnan(depth) | (depth < 0)] == 0).all()
    assert not np.isnan(bad.excess).any() and not np.isinf(bad.rigid).any()            # a non-finite component is THE quiet NaN
    assert set(np.unique(R.bits(bad.rigid)[np.isnan(bad.rigid)])) == {R.QNAN}
    behind = by["behind the camera"][1]
    assert 0.2 < (behind.cz <= 0).mean() < 0.9 and not behind.inside[behind.cz <= 0].any() and behind.inside.any()
    edge = by["edge"][1]
    assert (edge.px[0] == W - 1).all() and (edge.py[0] == H - 1).all() and edge.inside[0].all() and (edge.label[0] > 0).all()
    assert (edge.px[1] == np.nextafter(np.float32(W - 1), np.float32(np.inf))).all() and not edge.inside[1].any()
    assert (edge.py[1] == np.nextafter(np.float32(H - 1), np.float32(np.inf))).all() and (edge.label[1] == 0).all()
    assert edge.inside[2].all() and (edge.px[2] < W - 1).all()
    special, f = by["NaN and inf flow"][1], by["NaN and inf flow"][0][2]
    assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any() and not np.isnan(special.excess).any()
    assert (special.label[~np.isfinite(f).all(axis=1)] == 0).all()                     # inf - inf: e2 - thr is NaN, not judged
    assert by["eps = 0"][0][1].eps == 0.0 and by["other alpha, beta, eps"][0][4:] == (0.05, 0.25)


# ---- 3. the translating scene -----------------------------------------------------------------------------------------------------------
def test_translating_scene():
    """Constant depth, identity rotation, a translation along x: the rigid flow is fx * tx / d within the derived bound (here all
    numbers are dyadic, so it is exact), and a flow that equals it except on an 8x8 square displaced by (+5, 0) is labelled 2
    exactly on the square and 1 elsewhere inside."""
    s, flow, want, label = R.translating_scene()
    r = R.rigid(s.depth, s.T, s.K, s.iK, flow, eps=s.eps)
    Ex, Ey, _, _ = R.coordinate_error(s.depth, s.T, s.K, s.iK, s.eps)
    assert (np.abs(r.ru.astype(np.float64) - 32 * 0.5 / 4.0) <= Ex + R.U * 4.0).all() and (np.abs(r.rv) <= Ey).all()
    assert np.array_equal(R.bits(r.rigid), R.bits(want))
    assert np.array_equal(r.label, label) and (label == 2).sum() == 64 and (label == 0).sum() == 4 * 24
    f = np.float32
    static, moving = f(0) - (f(0.01) * f(32) + f(0.5)), f(25) - (f(0.01) * (f(81) + f(16)) + f(0.5))
    assert set(np.unique(r.excess)) == {static, moving, f(np.inf)}


# ---- 4. header, binding, ABI, refusals --------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry(built):
    src = open(os.path.join(ROOT, "include", "dvslam.h")).read()
    m = re.search(r"\bint\s+dvs_rigid_flow\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    assert m and m.group(1).count(",") + 1 == 21
    assert "dvs_rigid_flow" in built.exported_symbols() and len(built._SIGNATURES["dvs_rigid_flow"][1]) == 21
    assert hasattr(built.lib(), "dvs_rigid_flow")
    for line in ("P[i][j] = ((K[i][0]*T[0][j] + K[i][1]*T[1][j]) + K[i][2]*T[2][j]) + K[i][3]*T[3][j]", "den = cz + eps",
                 "inside = cz > 0 and 0 <= px <= W-1 and 0 <= py <= H-1", "thr = alpha*m + beta", "0x7FC00000"):
        assert line in src, line                                                       # the arithmetic is stated
    assert "GeoNet" in open(os.path.join(ROOT, "PAPERS.md")).read()
    kernel = open(os.path.join(ROOT, "deep-visual-slam_amd", "csrc", "rigidflow.hip")).read()
    assert "#pragma clang fp contract(off)" in kernel and "__shared__" not in kernel and "atomic" not in kernel.replace("no atomics", "")


def test_abi_is_still_12(built):
    assert built.ABI_VERSION == 12 and built.lib().dvs_abi_version() == 12


P = 1 << 20       # non-NULL, 16-byte aligned "device pointers" a MiB apart: nothing dereferences them before the checks fail


def _entry(l, depth=P, d_image=35, d_row=7, K=2 * P, iK=3 * P, T=4 * P, flow=5 * P, f_image=70, f_plane=35, f_row=7, valid=6 * P,
           rigid=7 * P, excess=8 * P, label=9 * P, N=2, H=5, W=7, alpha=0.01, beta=0.5, eps=1e-7):
    return l.dvs_rigid_flow(depth, d_image, d_row, K, iK, T, flow, f_image, f_plane, f_row, valid, rigid, excess, label, N, H, W,
                            alpha, beta, eps, None)


BAD_CALLS = [
    ("NULL depth", dict(depth=None)),
    ("NULL K", dict(K=None)),
    ("NULL inv_K", dict(iK=None)),
    ("NULL T", dict(T=None)),
    ("misaligned depth", dict(depth=P + 2)),
    ("misaligned T", dict(T=4 * P + 1)),
    ("misaligned flow", dict(flow=5 * P + 2)),
    ("misaligned rigid", dict(rigid=7 * P + 2)),
    ("misaligned excess", dict(excess=8 * P + 1)),
    ("N = 0", dict(N=0)),
    ("N = 65536", dict(N=65536)),
    ("H = 0", dict(H=0)),
    ("W = -1", dict(W=-1)),
    ("W past 2^24", dict(W=(1 << 24) + 1, H=1, d_row=1 << 25, d_image=1 << 25, f_row=1 << 25, f_plane=1 << 25, f_image=1 << 26)),
    ("too many lanes", dict(H=1 << 24, W=1 << 24, d_row=1 << 24, f_row=1 << 24)),
    ("depth row stride < W", dict(d_row=6)),
    ("depth image stride < the image", dict(d_image=34)),
    ("flow row stride < W", dict(f_row=6)),
    ("flow plane stride < the plane", dict(f_plane=34)),
    ("flow image stride < two planes", dict(f_image=69)),
    ("stride out of range", dict(d_row=1 << 41, d_image=1 << 45)),
    ("flow stride out of range", dict(f_row=1 << 41, f_plane=1 << 45, f_image=1 << 47)),
    ("alpha < 0", dict(alpha=-0.01)),
    ("alpha NaN", dict(alpha=float("nan"))),
    ("beta inf", dict(beta=float("inf"))),
    ("eps < 0", dict(eps=-1e-7)),
    ("eps NaN", dict(eps=float("nan"))),
    ("eps inf", dict(eps=float("inf"))),
    ("excess without flow", dict(flow=None, valid=None, label=None)),
    ("label without flow", dict(flow=None, valid=None, excess=None)),
    ("rigid overlaps depth", dict(rigid=P)),
    ("rigid overlaps the end of depth", dict(rigid=P + 4 * (35 + 4 * 7 + 6))),
    ("excess overlaps flow", dict(excess=5 * P + 16)),
    ("label overlaps valid", dict(label=6 * P + 2 * 5 * 7 - 1)),
    ("label overlaps T", dict(label=4 * P + 127)),
    ("rigid overlaps K", dict(rigid=2 * P - 8 * 2 * 5 * 7 + 4)),
    ("excess overlaps inv_K", dict(excess=3 * P + 64)),
]


@pytest.mark.parametrize("name,kw", BAD_CALLS, ids=[b[0] for b in BAD_CALLS])
def test_entry_refuses_bad_arguments(built, name, kw):
    l = built.lib()
    assert _entry(l, **kw) == -1                     # DVS_ERR_INVALID: no launch was tried (this machine has no GPU to refuse one)
    assert b"dvs_rigid_flow" in l.dvs_last_error()


def test_messages_say_what_is_wrong_and_no_output_is_no_launch(built):
    l = built.lib()
    assert _entry(l, d_row=6) < 0 and b"depth row stride 6 is below W=7" in l.dvs_last_error()
    assert _entry(l, f_image=69) < 0 and b"flow image stride 69 is below" in l.dvs_last_error()
    assert _entry(l, flow=None, valid=None, label=None) < 0 and b"excess and label need a flow" in l.dvs_last_error()
    assert _entry(l, rigid=P) < 0 and b"output rigid overlaps input depth" in l.dvs_last_error()
    assert _entry(l, label=6 * P + 69) < 0 and b"output label overlaps input valid" in l.dvs_last_error()
    assert _entry(l, rigid=None, excess=None, label=None) == 0                # nothing to write: returns before any launch
    assert _entry(l, flow=None, valid=None, rigid=None, excess=None, label=None) == 0
    assert _entry(l, flow=None, rigid=None, excess=None, label=None) == 0     # valid is read with a flow only


def test_rigid_flow_signature_and_cpu_tensors(built):
    from deep_visual_slam_amd import raft_video
    E = built.DvsError
    params = inspect.signature(raft_video.rigid_flow).parameters
    assert list(params) == ["depth", "T", "K", "inv_K", "flow", "valid", "alpha", "beta", "eps", "excess"]
    assert [params[k].default for k in list(params)[3:]] == [None, None, None, 0.01, 0.5, 1e-7, False]
    assert "torch.linalg.inv" in raft_video.rigid_flow.__doc__ and "bit-for-bit" in raft_video.rigid_flow.__doc__
    d, m = torch.ones(2, 1, 5, 7), torch.eye(4).repeat(2, 1, 1)
    with pytest.raises(E, match="rigid_flow: depth: GPU tensors only .* no CPU path"):
        raft_video.rigid_flow(d, m, m)
    meta = lambda *shape: torch.empty(shape, device="meta")
    with pytest.raises(E, match="GPU tensors only"):
        raft_video.rigid_flow(meta(2, 1, 5, 7), meta(2, 4, 4), meta(4, 4))


class _Stand:
    """What the argument checks read of a tensor (is_cuda, dtype, dim(), shape, device): a GPU tensor's stand-in on a machine
    without one."""

    def __init__(self, shape, dtype=torch.float32, device="cuda:0"):
        self.shape, self.dtype, self.device, self.is_cuda = torch.Size(shape), dtype, torch.device(device), True

    def dim(self):
        return len(self.shape)


def test_rigid_flow_refuses_mismatches_before_any_launch(built, monkeypatch):
    """Every shape, dtype or device mismatch and every bad threshold: raised by the argument checks, which read nothing but the
    tensors' descriptions; neither the library nor a tensor method that would copy is reached."""
    from deep_visual_slam_amd import raft_video
    E = built.DvsError
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (_Stand, torch.Tensor)))
    monkeypatch.setattr(raft_video._lib, "lib", lambda: pytest.fail("the library was reached"))
    S = _Stand
    ok = dict(depth=S((2, 1, 5, 7)), T=S((2, 4, 4)), K=S((4, 4)), inv_K=S((2, 4, 4)), flow=S((2, 2, 5, 7)),
              valid=S((2, 5, 7), dtype=torch.uint8))
    bad = [
        (dict(depth=S((2, 2, 5, 7))), r"depth: \[N,1,H,W\] or \[N,H,W\] expected, got \(2, 2, 5, 7\)"),
        (dict(depth=S((5, 7))), r"depth: .* got \(5, 7\)"),
        (dict(depth=S((2, 1, 5, 7), dtype=torch.float64)), r"depth: fp32 only, got torch.float64"),
        (dict(T=S((4, 4))), r"T: \[2,4,4\] expected, got \(4, 4\)"),
        (dict(T=S((3, 4, 4))), r"T: \[2,4,4\] expected, got \(3, 4, 4\)"),
        (dict(T=S((2, 4, 4), dtype=torch.float16)), r"T: fp32 only"),
        (dict(K=S((3, 3))), r"K: \[2,4,4\] or \[4,4\] expected, got \(3, 3\)"),
        (dict(K=S((1, 4, 4))), r"K: \[2,4,4\] or \[4,4\] expected, got \(1, 4, 4\)"),
        (dict(inv_K=S((2, 3, 3))), r"inv_K: \[2,4,4\] or \[4,4\] expected"),
        (dict(flow=S((2, 2, 5, 8))), r"flow: \[2,2,5,7\] expected, got \(2, 2, 5, 8\)"),
        (dict(flow=S((2, 5, 7))), r"flow: \[2,2,5,7\] expected"),
        (dict(flow=S((2, 2, 5, 7), dtype=torch.float64)), r"flow: fp32 only"),
        (dict(valid=S((2, 5, 7))), r"valid: uint8 \[2,5,7\] expected .* got torch.float32"),
        (dict(valid=S((2, 1, 5, 7), dtype=torch.uint8)), r"valid: uint8 \[2,5,7\] expected"),
        (dict(T=S((2, 4, 4), device="cuda:1")), r"T is on cuda:1, depth on cuda:0"),
        (dict(K=S((4, 4), device="cuda:1")), r"K is on cuda:1"),
        (dict(flow=S((2, 2, 5, 7), device="cuda:1")), r"flow is on cuda:1"),
        (dict(valid=S((2, 5, 7), dtype=torch.uint8, device="cuda:1")), r"valid is on cuda:1"),
        (dict(alpha=-1.0), ".* must be finite and not negative"),
        (dict(beta=float("nan")), ".* must be finite and not negative"),
        (dict(eps=float("inf")), ".* must be finite and not negative"),
        (dict(eps=-1e-7), ".* must be finite and not negative"),
        (dict(flow=None, valid=None, excess=True), "excess=True needs a flow"),
    ]
    for kw, msg in bad:
        with pytest.raises(E, match="rigid_flow: " + msg):
            raft_video.rigid_flow(**{**ok, **kw})
    with pytest.raises(E, match="GPU tensors only"):
        raft_video.rigid_flow(**{**ok, "valid": torch.ones(2, 5, 7, dtype=torch.uint8)})


def test_stream_signatures(built):
    """The rigid mode is RigidFlowStream: FlowStream's constructor keeps its signature, its frames carry the new fields as None."""
    from deep_visual_slam_amd import raft, raft_video
    params = inspect.signature(raft_video.RigidFlowStream.__init__).parameters
    assert list(params)[-4:-1] == ["rigid", "rigid_alpha", "rigid_beta"]
    assert (params["rigid"].default, params["rigid_alpha"].default, params["rigid_beta"].default) == (True, 0.01, 0.5)
    assert list(inspect.signature(raft_video.FlowStream.push).parameters) == ["self", "frame", "depth", "T", "K", "inv_K"]
    model = raft.SmallRAFT().eval()
    plain, rigid = raft_video.FlowStream(model), raft_video.RigidFlowStream(model, iters=3, bidirectional=True, rigid_alpha=0.05)
    assert plain.rigid is False and rigid.rigid is True and (rigid.iters, rigid.bidirectional, rigid.rigid_alpha) == (3, True, 0.05)
    assert raft_video.RigidFlowStream(model, rigid=False).rigid is False
    with pytest.raises(built.DvsError, match="rigid_alpha"):
        raft_video.RigidFlowStream(model, rigid_alpha=-1.0)
    frame = raft_video.FlowFrame(None, None, None)
    assert (frame.rigid, frame.motion) == (None, None)
    with pytest.raises(built.DvsError, match="host=True only"):
        frame.motion_host
