"""The layout contract of the ops / layers surface (ops.py): every tensor argument of every operator in every memory layout of the
view zoo (tests/layouts.py), and every cotangent layout autograd can hand the backwards.

One cell = one operator, one argument handed in as one kind of view (the others dense), against the same call with the view's
dense twin.  The standalone operators and the pose matrix (csrc/standalone.hip, csrc/pose.hip) use no float atomics and repeat
bit for bit: the two runs must be torch.equal, forward and gradients, and the dense run is judged against the fp64 oracle with
the tolerances of test_ops_gpu.py.  The fused loss chain adds with float atomics: both runs are judged against the fp64 oracle
with the helpers and tolerances of test_chain_gpu.py, and so do the supervised depth learner's fused losses (test_depth_learner_gpu.py's).
The uint8 input side (resize_u8, u8_to_f32_planar) is bit-exact, and so are nn_ops' pool and upsampling (csrc/pool.hip); its
convolutions are judged against torch's fp64 convolution by the tolerances of test_conv_gpu.py.  Shapes are the smallest at which a wrong stride changes the answer; H*W
is odd, so a batch slice of a planar tensor is not 16-byte aligned.  No argument here is an output: nothing may be refused."""
import numpy as np
import pytest
import torch

import layouts
import test_chain_gpu as TC
import test_depth_learner_gpu as TD
import raft_update_ref as U
import test_bn_gpu as TBN
import test_cloud_gpu as TCL
import test_networks_gpu as TN
from test_optim_gpu import ADAM_TOL
from test_ops_gpu import TOL
from test_pipeline_gpu import TO_TENSOR_ATOL

pytestmark = pytest.mark.gpu

B, H, W = 2, 17, 23


def _rand(*shape, seed=0, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _camera(batch, h, w):
    K = torch.tensor([[0.58 * w, 0, 0.5 * w, 0], [0, 1.92 * h, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float64)
    K = K[None].repeat(batch, 1, 1)
    K[1:, 0, 0] *= 1.1                                  # per-image intrinsics: a batch mix-up changes the answer
    return K.float(), torch.linalg.inv(K).float()


def _poses(batch, seed):
    from oracle import loss_chain as O
    aa = _rand(batch, 1, 3, seed=seed, lo=-0.05, hi=0.05)
    tr = _rand(batch, 1, 3, seed=seed + 1, lo=-0.1, hi=0.1)
    return aa, tr, O.transformation_from_parameters(aa.double(), tr.double()).float()


def _judge(table):
    """what -> (atol, rtol) of test_ops_gpu.TOL, by the name of the result ("out0", "d_x")."""
    def judge(what, got, want):
        atol, rtol = TOL[table[what]]
        np.testing.assert_allclose(got.double().numpy(), want.numpy(), atol=atol, rtol=rtol)
    return judge


def _cases():
    from deep_visual_slam_amd import layers as L
    from deep_visual_slam_amd import ops
    from oracle import loss_chain as O
    K, inv_K = _camera(B, H, W)
    aa, tr, T = _poses(B, 3)
    depth = _rand(B, 1, H, W, seed=5, lo=0.5, hi=5.0)
    points = O.backproject(depth.double(), inv_K.double()).float()
    img, img2 = _rand(B, 3, H, W, seed=6), _rand(B, 3, H, W, seed=7)
    cases = {}
    for inv in (False, True):
        cases["pose_to_mat" + ("_inv" if inv else "")] = layouts.Case(
            lambda axisangle, translation, inv=inv: L.transformation_from_parameters(axisangle, translation, invert=inv),
            {"axisangle": aa, "translation": tr},
            lambda axisangle, translation, inv=inv: O.transformation_from_parameters(axisangle, translation, invert=inv),
            _judge({"out0": "pose/M", "d_axisangle": "pose/grad", "d_translation": "pose/grad"}), grads=("axisangle", "translation"))
    cases["backproject"] = layouts.Case(
        lambda depth, inv_K: L.BackprojectDepth(B, H, W)(depth, inv_K), {"depth": depth, "inv_K": inv_K}, O.backproject,
        _judge({"out0": "backproject/cam", "d_depth": "warp/d_depth"}), grads=("depth",))
    cases["backproject_1x4x4"] = layouts.Case(
        lambda depth, inv_K: ops.backproject(depth, inv_K), {"depth": depth, "inv_K": inv_K[:1].clone()},
        lambda depth, inv_K: O.backproject(depth, inv_K.expand(B, 4, 4)),
        _judge({"out0": "backproject/cam", "d_depth": "warp/d_depth"}), grads=("depth",))
    cases["project"] = layouts.Case(
        lambda points, K, T: L.Project3D(B, H, W)(points, K, T), {"points": points, "K": K, "T": T},
        lambda points, K, T: O.project(points, K, T, H, W),
        _judge({"out0": "project/grid", "d_points": "warp/d_depth", "d_T": "warp/d_T"}), grads=("points", "T"))
    cases["project_1x4x4"] = layouts.Case(
        lambda points, K, T: ops.project(points, K, T, H, W), {"points": points, "K": K[:1].clone(), "T": T[:1].clone()},
        lambda points, K, T: O.project(points, K.expand(B, 4, 4), T.expand(B, 4, 4), H, W),
        _judge({"out0": "project/grid", "d_points": "warp/d_depth", "d_T": "warp/d_T"}), grads=("points", "T"))
    cases["ssim"] = layouts.Case(
        lambda x, y: L.SSIM()(x, y), {"x": img, "y": img2}, O.ssim,
        _judge({"out0": "ssim/out", "d_x": "ssim/grad", "d_y": "ssim/grad"}), grads=("x", "y"))
    cases["smooth_loss"] = layouts.Case(
        lambda disp, img: L.get_smooth_loss(disp, img), {"disp": _rand(B, 1, H, W, seed=8, lo=0.05, hi=0.95), "img": img}, O.smooth_loss,
        _judge({"out0": "smooth/out", "d_disp": "smooth/grad"}), grads=("disp",))
    return cases


# ---- the fused loss chain: float atomics, judged against the fp64 oracle -----------------------------------------------------------
def _chain_ref(target, src_l, src_r, K, inv_K, T_l, T_r, noise, **disps):
    """oracle.loss_chain.loss_chain from the camera matrices on (its own pieces, the same order): the per-scale losses."""
    from oracle import loss_chain as O
    disps = [disps["disp%d" % s] for s in range(len(disps))]
    _, _, Hh, Ww = target.shape
    losses = []
    for s, d in enumerate(disps):
        disp_up = O.upsample_bilinear(d, Hh, Ww)
        _, depth = O.disp_to_depth(disp_up, 0.1, 10.0)
        cam = O.backproject(depth, inv_K)
        color = [O.grid_sample_border(src, O.project(cam, K, T, Hh, Ww)) for src, T in ((src_l, T_l), (src_r, T_r))]
        reproj = torch.cat([O.reprojection_loss(c, target, 0.85) for c in color], 1)
        ident = torch.cat([O.reprojection_loss(src, target, 0.85) for src in (src_l, src_r)], 1) + noise[s] * 0.00001
        to_opt, _ = torch.min(torch.cat([ident, reproj], 1), dim=1, keepdim=True)
        mean_disp = torch.clamp(disp_up.mean(2, True).mean(3, True), min=0.001)
        losses.append(to_opt.mean() + 1e-3 * O.smooth_loss(disp_up / (mean_disp + 1e-7), target) / (2 ** s))
    return torch.stack(losses)


def _chain_fn(target, src_l, src_r, K, inv_K, T_l, T_r, noise, **disps):
    from deep_visual_slam_amd import ops
    return ops.loss_chain(target, src_l, src_r, K, inv_K, T_l, T_r, [disps["disp%d" % s] for s in range(len(disps))], noise=noise)[0]


def _chain_case(batch, h, w, scales):
    from deep_visual_slam_amd import synth
    sample = synth.parity_sample(batch, h, w, seed=77)
    disps = synth.parity_disps(batch, h, w, seed=3)[:scales] if scales > 1 else [_rand(batch, 1, h, w, seed=9, lo=0.05, hi=0.95)]
    from oracle import loss_chain as O
    poses = synth.parity_poses(batch, seed=5)
    T_l = O.transformation_from_parameters(poses[0][:, 0].double(), poses[1][:, 0].double(), invert=True).float()
    T_r = O.transformation_from_parameters(poses[2][:, 0].double(), poses[3][:, 0].double(), invert=False).float()
    g = torch.Generator().manual_seed(7)
    inputs = {"target": sample[("target_image", 0)], "src_l": sample[("source_left", 0)], "src_r": sample[("source_right", 0)],
              "K": sample[("K", 0)], "inv_K": sample[("inv_K", 0)], "T_l": T_l, "T_r": T_r,
              "noise": torch.randn(scales, batch, 2, h, w, generator=g)}
    for s in range(scales):
        inputs["disp%d" % s] = disps[s].contiguous()
    npix = batch * h * w

    def judge(what, got, want):
        # test_chain_gpu.test_chain_vs_oracle's judgement: the loss scalars, the disparity gradients by close_frac (argmin / clamp
        # flips), and what sums over every pixel (there the pose gradients, here the gradients of the matrices they make) by
        # close_pose
        if what == "out0":
            TC.close(got, want, *TC.LOSS_TOL)
        elif what.startswith("d_disp"):
            TC.close_frac(got, want, **TC.GRAD_TOL)
        else:
            TC.close_pose(got, want, npix)
    return layouts.Case(_chain_fn, inputs, _chain_ref, judge, grads=("T_l", "T_r") + tuple("disp%d" % s for s in range(scales)),
                        exact=False)


# ---- the supervised depth learner's fused losses: float atomics, judged against the fp64 oracle -----------------------------------
def _depth_case():
    from deep_visual_slam_amd import ops
    from oracle import depth_loss as OD
    sizes = [(H, W), (9, 12)]
    inputs = {"gt_depth": _rand(B, 1, H, W, seed=21, lo=0.2, hi=8.2), "rgb": _rand(B, 3, H, W, seed=22),
              "valid_mask": (_rand(B, 1, H, W, seed=23) < 0.7).to(torch.uint8)}
    for s, (h, w) in enumerate(sizes):
        inputs["pred%d" % s] = _rand(B, 1, h, w, seed=24 + s, lo=0.2, hi=5.2)
    names = tuple("pred%d" % s for s in range(len(sizes)))

    def fn(gt_depth, rgb, valid_mask, **preds):
        return ops.depth_multiscale_losses([preds[n] for n in names], gt_depth, rgb, valid_mask)

    def ref(gt_depth, rgb, valid_mask, **preds):
        _, _, _, silogs, smooths = OD.multi_scale_loss([preds[n] for n in names], gt_depth, rgb, valid_mask.bool())
        return torch.stack(silogs), torch.stack(smooths)

    def judge(what, got, want):                                 # test_depth_learner_gpu.test_multi_scale_loss_vs_oracle's judgement
        if what.startswith("out"):
            assert bool(((got.double() - want).abs() < TD.LOSS_RTOL * want.abs()).all()), (what, got, want)
        else:
            TD.grad_close(got, want)
    return layouts.Case(fn, inputs, ref, judge, grads=names, exact=False)


# ---- the input side: uint8 frames (csrc/preprocess.hip), bit-exact ------------------------------------------------------------------
def _pipeline_cases():
    from deep_visual_slam_amd import input_pipeline as P
    from oracle import input_pipeline as OI
    frames = torch.randint(0, 256, (3, 11, 8, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(31))

    def same_bytes(what, got, want):
        assert got.dtype == torch.uint8 and torch.equal(got, want), what

    def to_tensor_rule(what, got, want):
        assert float((got.double() - want).abs().max()) <= TO_TENSOR_ATOL, what
    return {
        "resize_u8": layouts.Case(lambda frames: P.resize_u8(frames, 6, 12), {"frames": frames},
                                  lambda frames: torch.from_numpy(np.stack([OI.pil_resize_bilinear(f, 6, 12) for f in frames.numpy()])),
                                  same_bytes),
        "u8_to_f32_planar": layouts.Case(lambda frames: P.u8_to_f32_planar(frames), {"frames": frames},
                                         lambda frames: OI.to_tensor(frames), to_tensor_rule),      # ToTensor itself, in fp32: what the
                                                                                                    # one-ulp tolerance is stated against
    }


# ---- nn_ops: the convolution routes, the pool and the upsampling (float atomics in the weight gradients) ------------------------------
def _nn_cases():
    import torch.nn.functional as F
    from deep_visual_slam_amd import nn_ops
    h, w = 7, 9

    def conv_rule(what, got, want):                             # test_conv_gpu's: 2e-5 / 1e-4 of the tensor's max (raft_update_ref.check_rel)
        U.check_rel(what.replace("d_", "d/"), got, want)

    def filt(co, ci, k, seed):
        return torch.randn(co, ci, k, k, generator=torch.Generator().manual_seed(seed)) * (2.0 / (ci * k * k)) ** 0.5
    x16, x64, x32 = (torch.randn(B, c, h, w, generator=torch.Generator().manual_seed(50 + c)) for c in (16, 64, 32))
    bias = lambda n, seed: 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(seed))
    cases = {}
    cases["conv3x3_s1"] = layouts.Case(lambda x, weight: nn_ops.conv2d(x, weight, None, 1, 1), {"x": x16, "weight": filt(16, 16, 3, 61)},
                                       lambda x, weight: F.conv2d(x, weight, None, 1, 1), conv_rule, grads=("x", "weight"), exact=False)
    cases["conv3x3_s2"] = layouts.Case(lambda x, weight, bias: nn_ops.conv2d(x, weight, bias, 2, 1),
                                       {"x": x16, "weight": filt(64, 16, 3, 62), "bias": bias(64, 63)},
                                       lambda x, weight, bias: F.conv2d(x, weight, bias, 2, 1), conv_rule, grads=("x", "weight", "bias"),
                                       exact=False)
    cases["conv1x1"] = layouts.Case(lambda x, weight, bias: nn_ops.conv2d(x, weight, bias, 1, 0, act="relu"),
                                    {"x": x64, "weight": filt(16, 64, 1, 64), "bias": bias(16, 65)},
                                    lambda x, weight, bias: F.relu(F.conv2d(x, weight, bias)), conv_rule, grads=("x", "weight", "bias"),
                                    exact=False)
    cases["conv_head"] = layouts.Case(lambda x, weight, bias: nn_ops.conv2d(x, weight, bias, 1, reflect_pad=1, act="sigmoid"),
                                      {"x": x16, "weight": filt(1, 16, 3, 66), "bias": bias(1, 67)},
                                      lambda x, weight, bias: torch.sigmoid(F.conv2d(F.pad(x, (1,) * 4, mode="reflect"), weight, bias)),
                                      conv_rule, grads=("x", "weight", "bias"), exact=False)
    skip = torch.randn(B, 16, 2 * h, 2 * w, generator=torch.Generator().manual_seed(68))
    cases["conv_decoder"] = layouts.Case(
        lambda x, x2, weight, bias: nn_ops.conv2d(x, weight, bias, 1, reflect_pad=1, act="elu", x2=x2),
        {"x": x32, "x2": skip, "weight": filt(16, 48, 3, 69), "bias": bias(16, 70)},
        lambda x, x2, weight, bias: F.elu(F.conv2d(F.pad(torch.cat([F.interpolate(x, scale_factor=2, mode="nearest"), x2], 1), (1,) * 4,
                                                         mode="reflect"), weight, bias)),
        conv_rule, grads=("x", "x2", "weight", "bias"), exact=False)
    cases["max_pool_3x3_s2"] = layouts.Case(lambda x: nn_ops.max_pool_3x3_s2(x), {"x": x16}, lambda x: F.max_pool2d(x, 3, 2, 1), conv_rule,
                                            grads=("x",))
    cases["upsample_nearest2x"] = layouts.Case(lambda x: nn_ops.upsample_nearest2x(x), {"x": x16},
                                               lambda x: F.interpolate(x, scale_factor=2, mode="nearest"), conv_rule, grads=("x",))
    return cases


def _bn_cases():
    """conv -> BatchNorm2d -> + residual -> ReLU in train mode (batch statistics: column sums by float atomics) and in eval mode
    with autograd (fixed statistics), judged as test_bn_gpu.test_conv_bn_act judges: rel() under FWD_REL / GRAD_REL."""
    import torch.nn.functional as F
    from deep_visual_slam_amd import nn_ops
    Cn, h, w = 16, 7, 9
    g = torch.Generator().manual_seed(80)
    x, res = torch.randn(B, Cn, h, w, generator=g), torch.randn(B, Cn, h, w, generator=g)
    wt = torch.randn(Cn, Cn, 3, 3, generator=g) * 0.08
    gamma, beta = torch.linspace(0.5, 1.5, Cn), torch.linspace(-0.3, 0.3, Cn)
    rmean, rvar = torch.linspace(-0.2, 0.2, Cn), torch.linspace(0.5, 2.0, Cn)

    def module(train, dev):
        bn = torch.nn.BatchNorm2d(Cn)
        with torch.no_grad():
            bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rmean), bn.running_var.copy_(rvar)
        return bn.to(dev).train(train)

    def judge(what, got, want):
        e, b = TBN.rel(got.double(), want), TBN.FWD_REL if what.startswith("out") else TBN.GRAD_REL
        print("%s: rel %.3e, bound %.1e" % (what, e, b))
        assert bool(torch.isfinite(got).all()) and e < b, (what, e, b)
    cases = {}
    for train in (True, False):
        cases["conv_bn_act_" + ("train" if train else "eval")] = layouts.Case(
            lambda x, weight, residual, train=train: nn_ops.conv_bn_act(x, weight, module(train, x.device), 1, 1, relu=True, residual=residual),
            {"x": x, "weight": wt, "residual": res},
            lambda x, weight, residual, train=train: F.relu(F.batch_norm(F.conv2d(x, weight, None, 1, 1), rmean.double().clone(),
                                                                         rvar.double().clone(), gamma.double(), beta.double(),
                                                                         training=train, eps=1e-5) + residual),
            judge, grads=("x", "weight", "residual"), exact=False)
    return cases


# ---- pointcloud: the record kernels and the pose chain (csrc/cloud.hip: no float atomics, bit-exact) -------------------------------------
def _cloud_cases():
    from deep_visual_slam_amd import pointcloud
    import cloud_ref
    Hc, Wc = 6, 10
    g = torch.Generator().manual_seed(90)
    depth = torch.rand(B, 1, Hc, Wc, generator=g) * 9 + 0.2
    depth[torch.rand(B, 1, Hc, Wc, generator=g) < 0.25] = 0.0
    image = torch.rand(B, 3, Hc, Wc, generator=g)
    K = torch.tensor([[0.6 * Wc, 0, 0.48 * Wc, 0], [0, 0.8 * Hc, 0.51 * Hc, 0], [0, 0, 1, 0], [0, 0, 0, 1]])[None].repeat(B, 1, 1)
    K[1, 0, 0] *= 1.1
    _, _, M = _poses(B, 91)
    inputs = {"depth": depth, "image": image, "K": K, "M": M}
    n_max = Hc * Wc

    def cloud_case(z_range):
        def fn(depth, image, K, M):
            out = TCL.nan_filled(B, n_max, depth.device)            # compact mode leaves records past count[b] untouched
            recs, count = pointcloud.depth_to_cloud(depth, image, K, M, z_range=z_range, out=out)
            return recs.view(torch.int32), count

        def judge(what, got, want):
            """test_cloud_gpu's check per image: the count, the coordinates under its bound, the colour bits, the untouched tail."""
            if what == "out1":
                return                                              # judged with the records
            d, im, k, m = (inputs[n].numpy() for n in ("depth", "image", "K", "M"))
            for b in range(B):
                want64, col, idx = cloud_ref.cloud(d[b, 0], im[b], k[b], m[b], z_range=z_range)
                ref32, _, _ = cloud_ref.cloud(d[b, 0], im[b], k[b], m[b], np.float32, z_range=z_range)
                xyz, rgb = TCL.split(got[b].view(torch.float32), idx.size)
                TCL.check_cloud(xyz, rgb, want64, ref32, col)
                assert bool((got[b, idx.size:] == TCL.NAN_PATTERN).all())

        def ref(depth, image, K, M):                                # shapes only: judge() compares with cloud_ref itself
            return torch.zeros(B, n_max, 4, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)

        def count_judge(what, got, want):
            if what == "out1":
                d, im, k, m = (inputs[n].numpy() for n in ("depth", "image", "K", "M"))
                assert got.tolist() == [cloud_ref.cloud(d[b, 0], im[b], k[b], m[b], z_range=z_range)[2].size for b in range(B)]
            else:
                judge(what, got, want)
        return layouts.Case(fn, inputs, ref, count_judge)
    cases = {"depth_to_cloud_dense": cloud_case(None), "depth_to_cloud_compact": cloud_case((0.0, 6.0))}

    T = torch.stack([_poses(1, 92 + i)[2][0] for i in range(5)])

    def chain(T):
        return pointcloud.PoseChain(T.device).step(T)

    def chain_ref(T):
        world, out = np.eye(4), []
        for t in T.numpy():
            world = world @ t
            out.append(world.copy())
        poses = torch.from_numpy(np.stack(out))
        return poses, poses.clone(), torch.from_numpy(np.stack([cloud_ref.tq(p) for p in out]))

    def chain_judge(what, got, want):
        """test_cloud_gpu.test_pose_chain's judgement: the poses (and M, which equals them without a `left`) and the translations
        under its bound; the quaternions unit, qw >= 0."""
        ref32, _ = cloud_ref.pose_chain(T.numpy(), dtype=np.float32)
        w64, _ = cloud_ref.pose_chain(T.numpy())
        lim = max(3.0 * float(np.abs(ref32.astype(np.float64) - w64).max()), 64 * TCL.EPS * float(np.abs(w64).max()))
        g = got.double().numpy()
        if what == "out2":
            assert float(np.abs(g[:, :3] - w64[:, :3, 3]).max()) <= lim
            assert bool((g[:, 6] >= 0).all()) and float(np.abs(np.linalg.norm(g[:, 3:], axis=1) - 1).max()) <= 4 * TCL.EPS
        else:
            assert float(np.abs(g - w64).max()) <= lim
    cases["pose_chain"] = layouts.Case(chain, {"T": T}, chain_ref, chain_judge)
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
        _CASES["loss_chain_17x23"] = _chain_case(B, H, W, 1)
        _CASES["loss_chain_48x64_s2"] = _chain_case(B, 48, 64, 2)
        _CASES["depth_multiscale_losses"] = _depth_case()
        _CASES.update(_pipeline_cases())
        _CASES.update(_nn_cases())
        _CASES.update(_bn_cases())
        _CASES.update(_cloud_cases())
    return _CASES


@pytest.mark.parametrize("case,arg,kind", layouts.input_cells(cases()))
def test_an_argument_in_any_layout_gives_the_dense_result(gpu_device, case, arg, kind):
    cases()[case].check_input(gpu_device, arg, kind)


@pytest.mark.parametrize("case,kind", layouts.cotangent_cells(cases()))
def test_a_cotangent_in_any_layout_gives_the_dense_gradients(gpu_device, case, kind):
    cases()[case].check_cotangent(gpu_device, kind)


@pytest.mark.parametrize("case", list(cases()))
def test_all_arguments_as_views_at_once(gpu_device, case):
    cases()[case].check_all_at_once(gpu_device)


# ---- whole models: the input images as views ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["crop", "cl"])
@pytest.mark.parametrize("model", ["depthnet", "posenet"])
def test_a_network_reads_image_views_as_it_reads_dense_images(gpu_device, model, kind):
    """ResnetEncoder(18) + the depth decoder, and PoseNet, at 64x96 in eval mode: images handed in as a crop of a padded frame and
    in channels_last memory give the dense-input result within the networks' forward tolerance (test_networks_gpu.FORWARD_REL)."""
    from deep_visual_slam_amd.depthnet import DepthNet
    from deep_visual_slam_amd.posenet_single import PoseNet
    torch.manual_seed(0)
    if model == "depthnet":
        net, x = DepthNet(18, pretrained=False), _rand(B, 3, 64, 96, seed=41)
    else:
        net, x = PoseNet(18, pretrained=False, num_input_images=2), _rand(B, 6, 64, 96, seed=42)
    net = net.to(gpu_device).eval()
    view = layouts.make(x.to(gpu_device), kind)
    with torch.no_grad():
        got, want = net(view), net(layouts.dense(view))
    pairs = [(got[("disp", s)], want[("disp", s)]) for s in range(4)] if model == "depthnet" else list(zip(got, want))
    for a, b in pairs:
        assert a.shape == b.shape and bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0
        assert TN.rel(a, b) < TN.FORWARD_REL


# ---- dp.FusedAdam over an arena built from parameters that were views ---------------------------------------------------------------
def test_fused_adam_over_parameters_that_were_views(gpu_device):
    """FlatParams moves every parameter into its arena (which the optimiser kernel writes: it is the package's own dense,
    aligned allocation, never a caller's view).  A 37 -> 19 -> 5 MLP whose parameters were a crop, a transposed tensor, a view
    at an offset and a batch slice steps, bit for bit, as the MLP with dense parameters does (csrc/optim.hip repeats exactly), and
    the dense one follows torch.optim.Adam within test_optim_gpu's tolerance."""
    from deep_visual_slam_amd import dp

    def mlp(kinds=None):
        torch.manual_seed(0)
        m = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5)).to(gpu_device)
        for p, kind in zip(m.parameters(), kinds or ()):
            p.data = layouts.make(p.data, kind)
            assert p.data_ptr() % 16 or not p.is_contiguous()
        return m
    ref, dense, views = mlp(), mlp(), mlp(("crop", "offset", "transposed", "batch_slice"))
    adam = torch.optim.Adam(ref.parameters(), lr=1e-3)
    opts = [dp.FusedAdam(dp.FlatParams(dp.trainable_parameters(m)), lr=1e-3) for m in (dense, views)]
    g = torch.Generator().manual_seed(1)
    for step in range(3):
        x = torch.randn(8, 37, generator=g).to(gpu_device)
        adam.zero_grad()
        ref(x).pow(2).mean().backward()
        adam.step()
        for m, opt in zip((dense, views), opts):
            m(x).pow(2).mean().backward()
            opt.step(grad_scale=1.0, zero_grad=True)
    for r, a, b in zip(ref.parameters(), dense.parameters(), views.parameters()):
        assert a.is_contiguous() and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        assert torch.equal(a.detach().cpu(), b.detach().cpu())
        assert torch.allclose(a, r, **ADAM_TOL)
