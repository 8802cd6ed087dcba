/*
 * dvslam.h -- C-ABI of libdvslam_hip.so: the MI355X (gfx950) hot path of the Monodepth2-style VO
 * training step of chansoopark98/Deep-Visual-SLAM.
 *
 * The reference has no FFI/plugin layer: its boundary is the Python operator surface
 * (model/layers.py, vo/learner_func.py, vo/learner_new.py, model/{resnet_encoder,depthnet,
 * posenet_single}.py).  This library sits directly under that surface; each entry point cites the
 * reference code (file:line under the reference repo) whose arithmetic it replaces.  The binding a
 * maintainer adds on the reference side is a ctypes stub, shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, a negative dvs_status on error; dvs_last_error() gives
 *     the message of the last failure on the calling thread;
 *   - all pointers are DEVICE pointers to fp32, NCHW-contiguous buffers owned by the caller unless
 *     a parameter is documented as host; nothing is allocated or freed inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are asynchronous,
 *     re-entrant and keep no thread-local state besides the error string (the reference's
 *     backward runs on PyTorch's autograd thread);
 *   - sizes are ints; B = batch, H/W = full-resolution image size.
 *
 * History
 *   ABI 12 removes names and adds no capability: where an operation had gained a parameter under a second, suffixed entry
 *   point (_slots, _ws, _res, _ymask), the full signature now carries the short name and the suffixed twin is gone.  The
 *   "(ABI n)" marks below say when a capability arrived (5 .. 11: each added entry points or fields and removed none).
 */
#ifndef DVSLAM_H
#define DVSLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    DVS_OK = 0,
    DVS_ERR_INVALID = -1,   /* bad argument (null pointer, non-positive size, unsupported shape) */
    DVS_ERR_LAUNCH = -2,    /* hipLaunch / runtime failure, see dvs_last_error() */
    DVS_ERR_UNSUPPORTED = -3
} dvs_status;

#define DVS_MAX_SCALES 4

/* ---------------------------------------------------------------------------------------------
 * library
 * ------------------------------------------------------------------------------------------- */
const char* dvs_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int dvs_abi_version(void);
/* Name of the code-object architecture the kernels were compiled for ("gfx950"). */
const char* dvs_arch(void);

/* Deterministic forward (test / debugging mode, off by default): with on != 0 no forward or data-gradient launch is split
 * over K with float atomics and the BatchNorm partial sums are added in one fixed order, so a forward pass repeats bit
 * for bit and two runs take the same ReLU / maxpool branches (their gradients then differ by smooth rounding noise only;
 * DESIGN.md section 6).  The BatchNorm batch statistics must then come from dvs_bn_bwd_reduce(dz = y, z = NULL, y,
 * a table with mean = 0, invstd = 1) instead of the convolution's atomic statistics epilogue (the Python side does that). */
int dvs_set_deterministic(int on);
int dvs_get_deterministic(void);

/* Arithmetic of the implicit-GEMM convolutions (ABI 8; process-wide, 0 by default).  mode 0: fp32 operands on the fp32 matrix
 * cores -- the reference's default precision and what every parity statement of this library is made for.  mode 1: bf16 operands
 * (rounded to nearest-even as they are staged into LDS), fp32 accumulation, fp32 tensors in HBM on both sides -- the counterpart
 * of the reference's `use_amp` branch (vo/train.py:44,177-185: torch.autocast + GradScaler around the same modules); forward,
 * data and weight gradient of dvs_conv2d_* take it (the stems on bf16 kernels of their own), the dvs_conv3x3_bf16_* entry points
 * below exist for it; the Winograd kernels (not used in the mode), the row-ring kernels of the 16-channel layers, the heads,
 * BatchNorm, the loss chain and the optimiser stay fp32.  Results then differ from mode 0 by bf16 operand rounding (2^-9 relative per product, averaging down over
 * K): separately toleranced in tests/test_bf16_gpu.py, never the headline precision. */
int dvs_set_precision(int mode);
int dvs_get_precision(void);

/* Peak probes (ABI 7; measurement aids of bench.py's `measured_peaks`, timed by the caller with events on `stream`):
 *   dvs_peak_probe_mfma: one wave per SIMD on every CU runs 4 * iters independent v_mfma_f32_32x32x2_f32 from registers; *flops
 *                        (host) = the flops the launch executes.  scratch: any device buffer of >= 4 bytes (never written).
 *   dvs_peak_probe_copy: a 16-byte-per-lane streaming copy of `bytes` (multiple of 16) from src to dst: 2 * bytes of HBM traffic. */
int dvs_peak_probe_mfma(float* scratch, int iters, double* flops, void* stream);
int dvs_peak_probe_copy(const void* src, void* dst, size_t bytes, void* stream);

/* Per-kernel timing with HIP events recorded on the launch stream around each main kernel (used by
 * bench.py for the roofline line; off by default).  dvs_profile_enable(1) clears the counters;
 * dvs_profile_read synchronises the recorded events of one slot and returns the accumulated
 * kernel time and launch count.  Slot names are the kernel names seen by rocprofv3. */
int dvs_profile_enable(int on);
int dvs_profile_slots(void);
const char* dvs_profile_slot_name(int slot);
int dvs_profile_read(int slot, double* total_ms, long* launches);
/* Algorithmic work of the launches recorded in a slot: flops for the MFMA kernels (2*M*N*K of each
 * convolution), 0 for kernels whose byte count the caller derives from the problem size. */
int dvs_profile_work(int slot, double* work);

/* ---------------------------------------------------------------------------------------------
 * a13  Adam over a flat fp32 arena: one pass replaces torch.optim.Adam(params, lr) + zero_grad of
 *      the reference trainer (vo/train.py:114-117,175,192).  torch.optim.Adam arithmetic (no weight
 *      decay, no amsgrad): m,v updates, bias corrections, p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2)+eps).
 *      grad is multiplied by grad_scale first (1/world_size after a sum all-reduce); zero_grad != 0
 *      clears grad in the same pass.  All four buffers hold n floats and are 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
int dvs_adam_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                  float beta1, float beta2, float eps, int step, float grad_scale, int zero_grad,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * a1-a3  convolutions of ResnetEncoder / DepthNet decoder / PoseNet decoder as implicit GEMMs on the
 *        fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32).
 *        replaces nn.Conv2d inside torchvision BasicBlock (model/resnet_encoder.py:83-111),
 *        Conv3x3 / ConvBlock (model/layers.py:106-136), the decoder's upsample + concat
 *        (model/depthnet.py:79-88, model/layers.py:196-199) and PoseNet's head
 *        (model/posenet_single.py:174-202).
 *   Layout: activations NHWC (torch channels_last of the reference's NCHW tensors), weights
 *   [Cout][kh][kw][Cin] (torch channels_last of the reference's [Cout,Cin,kh,kw] parameter).
 *   Output size: Ho = (H + 2 pad - kh)/stride + 1 (same for W).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int B, H, W, Cin, Cout;
    int kh, kw, stride;
    int pad;        /* implicit padding on every side */
    int pad_mode;   /* 0 = zeros (nn.Conv2d padding), 1 = nn.ReflectionPad2d(pad) in front of the conv;
                       dvs_conv2d_dgrad only: 2 = H x W is an already reflection-padded input, pad = 0 (dvs_reflect_fold follows) */
} dvs_conv_desc;

typedef struct {
    /* input-side fusion (applied while the im2col slice is gathered) */
    const float* x2;        /* non-NULL: input = concat(upsample_nearest2x(x [B,H/2,W/2,C1]), x2 [B,H,W,Cin-C1]) */
    int C1;
    const float* in_scale;  /* non-NULL: x <- x * in_scale[c] + in_shift[c] (folded BatchNorm / input normalisation) */
    const float* in_shift;
    int in_relu;            /* then ReLU */
    int nchw_planar;        /* x is a planar [B,Cin,H,W] image (encoder conv1); any Cin */
    /* output-side fusion */
    int act;                /* 0 none, 1 ReLU, 2 ELU(alpha=1), 3 sigmoid, 4 GELU (erf form; forward only: the ViT MLP of
                               model/depth_anything_v2/dinov2_layers/mlp.py:35-41) */
    float* stats;           /* non-NULL: [2][Cout], += per-channel sum and sum of squares of the raw
                               (pre-bias, pre-activation) output: BatchNorm batch statistics */
    int stat_groups;        /* 0 / 1: one set of statistics; 2: stats is [2][2][Cout], the first and second half of
                               the batch counted separately -- PoseNet runs its two frame pairs as one batch of 2B
                               and the reference's two calls (vo/learner_new.py:113-114) normalise each pair alone */
    const float* residual;  /* non-NULL: [B,Ho,Wo,Cout] added before the activation: y = act(conv + bias + residual) --
                               the BasicBlock tail relu(bn2(conv2(.)) + identity) with an eval-mode BatchNorm folded
                               into w / bias (inference path of model/resnet_encoder.py:100-111) */
    int stat_slots;         /* (ABI 5) 0 / 1: one table; a power of two <= 64: stats is [stat_slots][G][2][Cout] and output tile t
                               adds into copy t % stat_slots -- a 1x1 downsample convolution is all epilogue, and ~900 tiles
                               adding to the same 2 x Cout addresses serialise in the L2; dvs_bn_fwd adds the copies up.
                               Not for the planar (conv1) input. */
} dvs_conv_fusion;

/* y [B,Ho,Wo,Cout] = act(conv(x, w) + bias); `f` may be NULL (no fusion). */
int dvs_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, const dvs_conv_desc* d,
                   const dvs_conv_fusion* f, void* stream);

/* Backward of dvs_conv2d_fwd.
 *   dvs_conv2d_pack_wt: wt[ci][kh][kw][co] = w[co][kh][kw][ci], the [N][K] operand of the data gradient.
 *   dvs_conv2d_dgrad:   dx [B,H,W,Cin] = conv_transpose(dy * act'(y_out), w).  `d` describes the FORWARD
 *                       conv; stride 1 or 2; pad_mode 1 only for ReflectionPad2d(1) + 3x3 (the reflection's
 *                       gradient fold is done in the gather).  y_out/dact: forward output and its
 *                       activation code (0 = dy is already the pre-activation gradient).  For an
 *                       upsample+concat forward, dx is the gradient of the concatenated [B,H,W,Cin] input.
 *   dvs_conv2d_wgrad:   dw [Cout][Ktot] += sum_pixels (dy * act'(y_out)) x im2col(x), dbias [Cout] += column
 *                       sums (NULL = skip); both are accumulated with atomics, the caller zero-fills.  `f`
 *                       carries the forward's input-side fusion (x2/C1, in_scale/in_shift/in_relu,
 *                       nchw_planar; act/stats ignored).  With nchw_planar dw is packed [Cout][Cin][kh][8].
 *   Channel counts must be multiples of 4 (NHWC 16-byte gathers). */
/* Winograd F(2x2, 3x3) for the stride-1 / pad-1 3x3 convolutions of the ResNet BasicBlocks (torchvision BasicBlock conv1/conv2
 * as used by model/resnet_encoder.py:94-111): 16 products per 2x2 outputs instead of 36 on the fp32 matrix cores.
 *   dvs_wino_weights:     u [K][4][N][4] = G g G^T of every (input, output) channel pair of w [Cout][3][3][Cin];
 *                         flip = 0: K = Cin, N = Cout (forward); flip = 1: K = Cout, N = Cin, filter rotated by 180 degrees (the
 *                         data gradient of the same convolution is dvs_conv3x3_wino_fwd(dy, u_flip) with Cin/Cout swapped).
 *   dvs_wino_weights_batch: both orientations of n weights in one launch; table rows {w, u, u_flip (pointers), Cout, Cin,
 *                         first workgroup, 0 (int32)} sorted by first workgroup, ceil(Cout*Cin/256) workgroups per entry.
 *   dvs_conv3x3_wino_fwd: y [B,H,W,Cout] = [relu](conv3x3(x [B,H,W,Cin]) [+ res] + bias) (res: NULL or a tensor of y's shape -- the
 *                         skip path's gradient when the call is a BasicBlock's conv1 data gradient); stats (NULL = skip)
 *                         [stat_slots][stat_groups][2][Cout] += per-channel sum / sum of squares of the raw output, as
 *                         dvs_conv2d_fwd's epilogue does: stat_slots copies of the table (a power of two <= 64, 1 = one table,
 *                         zero-filled by the caller), workgroup w adds into copy w % stat_slots and dvs_bn_fwd / dvs_bn_finalize
 *                         add the copies up.  The kernel runs one workgroup per CU whose last act is these atomics; with one
 *                         copy, thousands of same-address atomics serialise in the L2 and each workgroup's CU waits for them.
 *                         Cin % 16 == 0, Cout % 4 == 0, tensors < 2 GiB.  as_dgrad: count the launch in the data-gradient
 *                         profile slot.
 *   dvs_conv3x3_wino_gen: the same kernel behind the decoder's gathers (model/layers.py:26-41 Conv3x3 = ReflectionPad2d(1) + 3x3,
 *                         model/depth_decoder.py:52-62 upsample + concat): logical input [B,H,W,C1+C2] = cat(x [, x2]) where x is
 *                         [B,H/2,W/2,C1] when `upsample` (nearest 2x in the gather) and x2 [B,H,W,C2] the skip (NULL / C2 = 0:
 *                         none); reflect = 1: ReflectionPad2d(1), else zero padding; org = 1: y [B,H,W,Cout]; org = 2: the full
 *                         correlation y [B,H+2,W+2,Cout] (the padded-domain data gradient that dvs_reflect_fold folds back);
 *                         act: 0 none, 1 ReLU, 2 ELU.  C1 % 8 == 0, (C1+C2) % 16 == 0, Cout % 4 == 0.
 *   dvs_conv3x3_wino_wgrad: dw [Cout][3][3][Cin] += the weight gradient of that convolution from x [B,H,W,Cin] and dy [B,H,W,Cout]
 *                         (dL/dg = G^T [sum over tiles (A dY A^T) o (B^T d B)] G), the tile range split over about
 *                         target_workgroups (0 = default) workgroups that add into dw with float atomics (plain adds when
 *                         one workgroup owns a block).  Cin % 32 == 0, Cout % 32 == 0, tensors < 1 GiB (ABI 7: its offsets carry two mask bits).
 *                         dw may be shared with other launches only through float atomics: with one tile range per block (small
 *                         problems) the kernel adds with plain read-modify-writes, so no OTHER launch may touch the same dw block
 *                         concurrently (one stream per weight tensor, as the Python side keeps it).
 *                         Ordered form (ABI 7): with a partial-sum `workspace` (device, `workspace_bytes` >= what
 *                         dvs_conv3x3_wino_wgrad_workspace returns for the same sizes) every workgroup stores its 32 x 32 x 9 block
 *                         there and a second kernel adds the blocks into dw in split order: no float atomics on dw, bit-identical
 *                         results run to run (the deterministic backward).  workspace = NULL (workspace_bytes 0): the atomic form. */
int dvs_wino_weights(const float* w, float* u, int Cout, int Cin, int flip, void* stream);
int dvs_conv3x3_wino_gen(const float* x, const float* x2, const float* u, const float* bias, float* y, int B, int H, int W, int C1, int C2,
                         int Cout, int Ho, int Wo, int org, int upsample, int reflect, int act, int as_dgrad, void* stream);
size_t dvs_conv3x3_wino_wgrad_workspace(int B, int H, int W, int Cin, int Cout, int target_workgroups);
int dvs_conv3x3_wino_wgrad(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout, int target_workgroups,
                           float* workspace, size_t workspace_bytes, void* stream);
/*   dvs_conv3x3_wino_wgrad_gen (ABI 6): the same weight gradient behind the decoder's gathers (the inputs dvs_conv3x3_wino_gen reads
 *   with reflect = 1, org = 1): dw [Cout][3][3][C1+C2] += d/dw of conv3x3(ReflectionPad2d(1)(cat(x [, x2]))) from dy [B,H,W,Cout],
 *   x [B,H/2,W/2,C1] when `upsample` (nearest 2x) else [B,H,W,C1], x2 [B,H,W,C2] the skip (NULL / C2 = 0: none; only with
 *   `upsample`).  dact = 0: dy is the gradient in front of the activation (dvs_act_bwd took the derivative and the bias gradient);
 *   dact = 1 (ReLU) / 2 (ELU): dy is multiplied by act'(y_out) as it is loaded (y_out [B,H,W,Cout] = the forward output) and
 *   dbias [Cout] (NULL: none) += its column sums.  One launch per source, each adding into its channel range of dw.
 *   C1, C2, Cout % 32 == 0, H, W >= 2 (even with `upsample`), tensors < 1 GiB; the same exclusivity rule for dw as above.
 *   workspace / workspace_bytes as in dvs_conv3x3_wino_wgrad, sized for the larger of the two sources (Cin = max(C1, C2)).  Replaces
 *   the weight / bias gradient of model/layers.py:26-41 Conv3x3 (+ ELU of ConvBlock, :106-118) inside model/depth_decoder.py:52-62. */
int dvs_conv3x3_wino_wgrad_gen(const float* x, const float* x2, const float* dy, const float* y_out, float* dw, float* dbias, int B, int H,
                               int W, int C1, int C2, int Cout, int upsample, int dact, int target_workgroups, float* workspace,
                               size_t workspace_bytes, void* stream);
int dvs_wino_weights_batch(const void* table, int n_entries, int total_workgroups, void* stream);
int dvs_conv3x3_wino_fwd(const float* x, const float* u, const float* bias, const float* res, float* y, float* stats, int stat_groups,
                         int stat_slots, int B, int H, int W, int Cin, int Cout, int relu, int as_dgrad, void* stream);
/*   bf16 mode (ABI 8, dvs_set_precision(1)): the stride-1 / zero-pad-1 3x3 convolution on v_mfma_f32_32x32x16_bf16 with the input
 *   patch of a workgroup (8 x 16 output pixels + halo, 64 channels at a time) kept in LDS as bf16 -- every tap reads the same image
 *   (csrc/conv_p16.hip).  dvs_conv3x3_bf16_pack: w fp32 [Cout][3][3][Cin] -> out bf16 [9][K/16][N][16] (9 K N 2 bytes); flip = 0:
 *   K = Cin, N = Cout (forward); flip = 1: K = Cout, N = Cin, taps rotated (data gradient).  dvs_conv3x3_bf16_fwd: y [B,H,W,N] =
 *   conv3x3(x [B,H,W,K]) [+ res]; stats / stat_groups / stat_slots as in dvs_conv3x3_wino_fwd (fp32 sums of the fp32 results);
 *   as_dgrad only labels the profile slot.  K % 64 == 0, N % 64 == 0, tensors < 2 GiB.  Same module as dvs_conv3x3_wino_fwd. */
/*   dvs_conv3x3_bf16_wgrad: dw [Cout][3][3][Cin] += the weight gradient of that convolution from x [B,H,W,Cin] and dy [B,H,W,Cout], bf16
 *   operands (both k-strided, fetched with ds_read_b64_tr_b16), fp32 accumulation, float atomics into dw (about target_workgroups
 *   workgroups, 0 = default; a workgroup owns a 32 x 32 x 9 block and a range of patches).  Cin % 32 == 0, Cout % 32 == 0. */
int dvs_conv3x3_bf16_wgrad(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout, int target_workgroups, void* stream);
/*   dvs_conv3x3_bf16_gen: the patch kernels behind the decoder's gathers -- arguments as dvs_conv3x3_wino_gen (x / x2 / C1 / C2 / Ho / Wo /
 *   org / upsample / reflect / act), wpack from dvs_conv3x3_bf16_pack over K = C1 + C2 (its N padded to 32 columns).  C1, C2, N
 *   multiples of 64: 64-channel chunks, 64 / 128 output channels per workgroup; otherwise multiples of 16: the thin kernel (32 output
 *   channels per workgroup, the chunk's weights in LDS).  dact != 0 (thin kernel, one plain source): x is a gradient dY and y_out the
 *   forward output of the same shape, the staged operand is dY * act'(y_out) (1 ReLU, 2 ELU). */
int dvs_conv3x3_bf16_gen(const float* x, const float* x2, const void* wpack, const float* bias, float* y, int B, int H, int W, int C1, int C2,
                         int N, int Ho, int Wo, int org, int upsample, int reflect, int act, int as_dgrad, const float* y_out, int dact,
                         void* stream);
/*   dvs_conv3x3_bf16_wgrad_gen: the same behind the decoder's gathers (arguments as dvs_conv3x3_wino_wgrad_gen, + reflect): dw
 *   [Cout][3][3][C1+C2] += d/dw of conv3x3(pad(cat(x [, x2]))), dy optionally multiplied by act'(y_out) as it is staged (dact) with
 *   dbias += its column sums.  C1, C2, Cout multiples of 16 (C1 of 32 when there is a second source). */
int dvs_conv3x3_bf16_wgrad_gen(const float* x, const float* x2, const float* dy, const float* y_out, float* dw, float* dbias, int B, int H, int W,
                               int C1, int C2, int Cout, int upsample, int reflect, int dact, int target_workgroups, void* stream);
int dvs_conv3x3_bf16_pack(const float* w, void* out, int Cout, int Cin, int flip, void* stream);
int dvs_conv3x3_bf16_fwd(const float* x, const void* wpack, const float* res, float* y, float* stats, int stat_groups, int stat_slots, int B,
                         int H, int W, int K, int N, int as_dgrad, void* stream);
int dvs_conv2d_pack_wt(const float* w, float* wt, int Cout, int Cin, int kh, int kw, void* stream);
/*   dvs_conv2d_pack_wt_batch: the same transpose for many weights in one launch.  `table` (device memory) = n_entries
 *   records { const float* w; float* wt; int Cout, Cin, taps, wg_begin; } (32 bytes each), wg_begin = number of
 *   workgroups of the records before it, a record needs taps * ceil(Cin/32) * ceil(Cout/32) workgroups;
 *   total_workgroups = their sum.  The weights change once per optimiser step: dp.FusedAdam repacks right after it. */
int dvs_conv2d_pack_wt_batch(const void* table, int n_entries, int total_workgroups, void* stream);
/*   dvs_act_bwd: dz = dy * act'(y) over n floats (n % 4 == 0), act as in dvs_conv_fusion -- the pre-activation gradient
 *   as a tensor; dvs_conv2d_dgrad / _wgrad are then called with dact = 0 (nn.ELU / ReLU / Sigmoid backward of
 *   model/layers.py:106-118 done once instead of in both gathers).  dbias (NULL = skip): [C] += column sums of dz, the
 *   bias gradient of the [.., C] tensor (C/4 must divide 256), so that dvs_conv2d_wgrad can be called without dbias. */
int dvs_act_bwd(const float* dy, const float* y, float* dz, size_t n, int act, float* dbias, int C, void* stream);
/*   dvs_reflect_fold: second half of a reflection-padded conv's data gradient computed on the PADDED domain.  g_padded
 *   [B][H+2][W+2][C] is the gradient w.r.t. ReflectionPad2d(1)(input) -- dvs_conv2d_dgrad of the equivalent unpadded
 *   ("valid") conv on an (H+2) x (W+2) input, zero padding, which the LDS-DMA kernel serves; this folds the mirrored
 *   border back (padded row 0 -> row 1, row H+1 -> row H-2, same for columns) and, for an upsample(+concat) input
 *   (C1 > 0), sums channels < C1 over 2x2 blocks into dx [B][H/2][W/2][C1] and stores channels >= C1 to dx_skip
 *   [B][H][W][C-C1]; C1 == 0: dx [B][H][W][C].  (model/layers.py:121-136 backward, model/depthnet.py:79-85.) */
int dvs_reflect_fold(const float* g_padded, float* dx, float* dx_skip, int B, int H, int W, int C, int C1, void* stream);
/*   dx_skip / C1 (upsample+concat forward only, else NULL / 0): the gradient is split in the epilogue --
 *   channels [0,C1) are summed over each 2x2 block into dx = [B,H/2,W/2,C1] with atomics (caller zero-fills dx),
 *   channels [C1,Cin) are stored to dx_skip = [B,H,W,Cin-C1]; C1 == Cin (upsample only) needs no dx_skip.
 *   residual (ABI 5; NULL = none; C1 must be 0): dx = data gradient + residual [B,H,W,Cin].  Where a tensor feeds
 *   several consumers -- a BasicBlock input read by conv1, the 1x1 downsample branch and, in DepthNet, the decoder's skip
 *   connection (torchvision BasicBlock through model/resnet_encoder.py:94-111, model/depthnet.py:79-85) -- autograd would add
 *   the consumers' gradients in one more pass over the tensor each; the gradient already computed is added in this kernel's
 *   epilogue instead.  Same for dvs_conv2d_head_bwd (dx_residual) and dvs_maxpool3x3s2_bwd (residual) below. */
int dvs_conv2d_dgrad(const float* dy, const float* wt, float* dx, const dvs_conv_desc* d, const float* y_out,
                     int dact, float* dx_skip, int C1, const float* residual, void* stream);
/*   dvs_conv2d_wgrad, ordered form (ABI 7): with a slab workspace of >= dvs_conv2d_wgrad_workspace(...) bytes every workgroup of the
 *   split-K implicit GEMM stores its partial tile with plain stores and a second kernel adds the splits into dw in split order -- no
 *   float atomics on dw (they run at a fifth of the plain-store rate on this chip and make the result depend on timing).  The stem
 *   and the thin full-resolution decoder layers have no slab path (workspace size 0: the workspace is ignored); a bias gradient
 *   (dbias) still rides on atomics.  workspace = NULL (workspace_bytes 0): the atomic form. */
size_t dvs_conv2d_wgrad_workspace(const dvs_conv_desc* d, const dvs_conv_fusion* f, int dact, int with_bias);
int dvs_conv2d_wgrad(const float* x, const float* dy, float* dw, float* dbias, const dvs_conv_desc* d, const dvs_conv_fusion* f,
                     const float* y_out, int dact, float* workspace, size_t workspace_bytes, void* stream);

/* Narrow output heads (Cout in {1,2,6,8}, Cin % 4 == 0, stride 1, "same" size: 2*pad == k-1) on the vector
 * ALUs: DepthNet's dispconv layers (model/depthnet.py:57-58,86-88) and PoseNet's last 1x1
 * (model/posenet_single.py:165).  `act` as in dvs_conv_fusion.  bwd: dx (NULL = skip), dw/dbias accumulated
 * with atomics (caller zero-fills); y / dy are the forward output and its gradient; dx_residual (NULL = none; needs dx):
 * dx = data gradient + dx_residual [B,H,W,Cin]. */
int dvs_conv2d_head_fwd(const float* x, const float* w, const float* bias, float* y, const dvs_conv_desc* d, int act,
                        void* stream);
int dvs_conv2d_head_bwd(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw,
                        float* dbias, const dvs_conv_desc* d, int act, const float* dx_residual, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a1  the ResNet stem's MaxPool2d(kernel_size=3, stride=2, padding=1) on NHWC tensors
 *     (torchvision resnet18.maxpool reached through model/resnet_encoder.py:104).
 *     x, dx: [B,H,W,C]; y, dy: [B,Ho,Wo,C] with Ho = (H-1)/2+1; idx: [B,Ho,Wo,C] bytes, the winning tap
 *     ky*3+kx (first maximum in scan order, as torch); C % 4 == 0.  bwd writes every element of dx:
 *     dx = maxpool gradient + residual [B,H,W,C] (NULL = none): the stem output feeds the pool and DepthNet's finest skip.
 * ------------------------------------------------------------------------------------------- */
int dvs_maxpool3x3s2_fwd(const float* x, float* y, unsigned char* idx, int B, int H, int W, int C, void* stream);
int dvs_maxpool3x3s2_bwd(const float* dy, const unsigned char* idx, float* dx, const float* residual, int B, int H, int W, int C,
                         void* stream);
/* `upsample` of model/layers.py:196-199 (F.interpolate(scale_factor=2, mode="nearest")) as a standalone operator on NHWC
 * tensors: x, dx [B,H,W,C]; y, dy [B,2H,2W,C]; C % 4 == 0.  The backward is the 2x2 block sum.  (The decoder itself never
 * materialises the upsampled tensor: dvs_conv_fusion.x2 / C1 gather it inside the convolution.) */
int dvs_upsample2x_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream);
int dvs_upsample2x_bwd(const float* dy, float* dx, int B, int H, int W, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a1  training-mode BatchNorm2d (+ residual add, + ReLU) of the ResNet BasicBlocks on NHWC tensors
 *     (torchvision BasicBlock tail used by model/resnet_encoder.py:100-111).
 *
 *     Shapes.  M = pixels (rows) per group, C % 4 == 0 and C/4 divides 256 (C in {4, 8, 16 .. 1024}).  groups G >= 1 (PoseNet
 *     evaluates its two frame pairs as one batch, each half normalised on its own): ONE launch serves G independent
 *     sub-batches of M rows each, stored back to back -- tensors [G*M][C], sums [G][2][C].  gamma / beta / running statistics /
 *     gradient sinks are shared by the groups (running statistics get the G updates in order).
 *     `stats` = [stat_slots][G][2][C]: per-channel sum / sum of squares of y as accumulated by the producing convolution's
 *     epilogue (dvs_conv2d_fwd, dvs_conv3x3_wino_fwd), stat_slots >= 1 copies that are added up on load; count = M.
 *     `fin` = [G][4][C]: rows scale, shift, mean, invstd of every group -- written by the forward, read by the backward.
 *
 *     Forward.
 *       finalize : mean, invstd = rsqrt(biased var + eps); scale = gamma*invstd; shift = beta - mean*scale, written to the
 *                  group-0 rows scale / shift / mean / invstd of a [G][4][C] table (group g at + g*4*C);
 *                  running_mean/var updated with `momentum` (unbiased var), NULL = leave them;
 *                  *num_batches_tracked (int64, NULL = skip) is incremented, as nn.BatchNorm2d does.
 *       apply_fwd: z = [relu](y*scale + shift [+ residual | + residual*res_scale + res_shift]); scale / shift (and res_scale /
 *                  res_shift) = group-0 rows of a [G][4][C] table.
 *       fwd      : finalize + apply_fwd in ONE launch (what the training forward uses); `fin` out; res_scale / res_shift =
 *                  group-0 rows of the downsample branch's own table, produced by dvs_bn_finalize.
 *
 *     Backward, two passes over the tensors.
 *       bwd_reduce: du = dz * mask (du NULL = do not store); sums[0][c] += sum du, sums[1][c] += sum du * xhat (= d beta,
 *                  d gamma); caller zero-fills sums.  Each workgroup writes one partial row into `workspace`
 *                  (dvs_bn_bwd_workspace bytes; 0 = unsupported shape), a second small kernel adds the rows into sums
 *                  (same-address float atomics serialise at ~85 ns each; one ordered sum under dvs_set_deterministic).
 *       bwd_apply: dy = gamma * invstd * (du - sums0/M - xhat * sums1/M); dgamma_acc / dbeta_acc (both or neither, NULL =
 *                  skip): d gamma += sums1, d beta += sums0, i.e. the parameter gradients are accumulated in place (what
 *                  autograd's AccumulateGrad would do with one more launch each).
 *       The mask: ymask == 0: [z > 0] (z NULL = no ReLU, no mask); rows 0 / 1 of `fin` are not read.  ymask != 0: ReLU without a
 *       residual (bn1 of a BasicBlock, the stem): z > 0 is recomputed from y with the forward's own expression
 *       max(y*scale + shift, 0), so the backward neither reads z nor writes / re-reads du (both must be NULL in bwd_reduce):
 *       5 tensor passes instead of 7; bwd_apply is handed dz in du's place and masks it again.
 *       A caller without a forward table builds one: (mean, invstd) = (0, 1) makes bwd_reduce a plain column sum of dz and
 *       dz * y (the deterministic batch statistics; the eval-mode affine map's parameter gradients).
 *       bwd      : (ABI 5) reduce + apply without the kernel in between that adds the per-workgroup partial rows: `slot_table` =
 *                  dvs_bn_bwd_slot_floats(C, groups) zero-filled floats ([G][32][2][C]); workgroup w of the reduce pass adds its
 *                  partial sums into copy w % 32 and every workgroup of the apply pass adds the copies up.  z / du / ymask as
 *                  above.  sums_out (NULL = skip): [G][2][C] = sum(du), sum(du * xhat) for callers that hand d beta / d gamma
 *                  to autograd.  The deterministic mode keeps bwd_reduce / bwd_apply with their ordered sum.
 *
 *     Stem tail (ABI 5): relu(bn1(conv1(x))) -> MaxPool2d(3, 2, 1) of model/resnet_encoder.py:102-104 without the tensor in between.
 *       relu_maxpool_fwd: y [B,H,W,C] = raw conv1 output, fin from dvs_bn_finalize (group = image / (B/G)); pooled [B,Ho,Wo,C]
 *                  and idx (one byte per element, winning tap ky*3+kx, first maximum in scan order) as dvs_maxpool3x3s2_fwd
 *                  would give on z = relu(y*scale+shift); z [B,H,W,C] is written only when non-NULL (DepthNet's finest skip
 *                  connection reads it; PoseNet never does).
 *       relu_maxpool_bwd: dz = maxpool gradient (gathered from dpool / idx, never stored) + dz_extra (NULL or [B,H,W,C]: the
 *                  gradient of z's other consumer), ReLU mask recomputed from y; sums [G][2][C] receive sum(dz), sum(dz*xhat)
 *                  (written, not accumulated); dy [B,H,W,C] = training-mode BatchNorm backward; dgamma_acc / dbeta_acc as in
 *                  bwd_apply.  workspace: dvs_bn_bwd_slot_floats(C, G) ZERO-FILLED floats (the slot table of bwd).
 * ------------------------------------------------------------------------------------------- */
int dvs_bn_finalize(const float* stats, int stat_slots, double count, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float momentum, float eps, float* scale, float* shift, float* mean,
                    float* invstd, int C, long long* num_batches_tracked, int groups, void* stream);
int dvs_bn_apply_fwd(const float* y, const float* scale, const float* shift, const float* residual,
                     const float* res_scale, const float* res_shift, float* z, size_t M, int C, int relu, int groups,
                     void* stream);
int dvs_bn_fwd(const float* y, const float* stats, int stat_slots, double count, const float* gamma, const float* beta,
               float* running_mean, float* running_var, float momentum, float eps, long long* num_batches_tracked,
               float* fin, const float* residual, const float* res_scale, const float* res_shift, float* z, size_t M,
               int C, int relu, int groups, void* stream);
size_t dvs_bn_bwd_workspace(size_t M, int C, int groups);
int dvs_bn_bwd_reduce(const float* dz, const float* z, const float* y, const float* fin, int ymask, float* du, float* sums,
                      float* workspace, size_t M, int C, int groups, void* stream);
int dvs_bn_bwd_apply(const float* du, const float* y, const float* fin, int ymask, const float* gamma, const float* sums, float* dy,
                     size_t M, int C, float* dgamma_acc, float* dbeta_acc, int groups, void* stream);
int dvs_bn_bwd_slot_floats(int C, int groups);
int dvs_bn_bwd(const float* dz, const float* z, const float* y, const float* fin, int ymask, const float* gamma, float* du, float* dy,
               float* slot_table, float* sums_out, size_t M, int C, float* dgamma_acc, float* dbeta_acc, int groups, void* stream);
int dvs_bn_relu_maxpool_fwd(const float* y, const float* fin, float* z, float* pooled, unsigned char* idx, int B, int H, int W, int C,
                            int groups, void* stream);
int dvs_bn_relu_maxpool_bwd(const float* dpool, const unsigned char* idx, const float* dz_extra, const float* y, const float* fin,
                            const float* gamma, float* sums, float* workspace, float* dy, int B, int H, int W, int C,
                            float* dgamma_acc, float* dbeta_acc, int groups, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a4  axis-angle + translation -> 4x4 camera motion
 *     replaces transformation_from_parameters / rot_from_axisangle / get_translation_matrix
 *     (vo/learner_func.py:29-104 == model/layers.py:28-103).
 *     axisangle, translation: [B,3]; M, dM: [B,4,4]; invert as in the reference (R^T . T(-t)).
 * ------------------------------------------------------------------------------------------- */
int dvs_pose_to_mat_fwd(const float* axisangle, const float* translation, int invert,
                        float* M, int B, void* stream);
int dvs_pose_to_mat_bwd(const float* axisangle, const float* translation, int invert,
                        const float* dM, float* d_axisangle, float* d_translation,
                        int B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a5-a12  fused view-synthesis loss chain
 *     replaces MonodepthTrainer._generate_images_pred + _compute_losses
 *     (vo/learner_new.py:132-258) and the operators they call: F.interpolate bilinear
 *     (learner_new.py:136-140), disp_to_depth (learner_func.py:16-26), BackprojectDepth
 *     (:106-135), Project3D (:137-159), F.grid_sample border/align_corners (learner_new.py:165-170),
 *     SSIM (learner_func.py:177-207), _compute_reprojection_loss (learner_new.py:60-74), auto-mask
 *     min (learner_new.py:212-244), disparity normalisation + get_smooth_loss
 *     (learner_new.py:246-252, learner_func.py:161-174).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int B, H, W;
    int num_scales;          /* 1..4; scale s has a [B,1,hs[s],ws[s]] disparity map */
    int hs[DVS_MAX_SCALES];
    int ws[DVS_MAX_SCALES];
    int auto_mask;           /* learner_new.py:37,212-231 */
    float min_depth, max_depth;      /* learner_new.py:39-40 */
    float ssim_ratio;                /* learner_new.py:38 */
    float smoothness_ratio;          /* learner_new.py:36 */
} dvs_chain_cfg;

typedef struct {
    /* inputs */
    const float* target;             /* [B,3,H,W]  sample[("target_image",0)] */
    const float* source[2];          /* [B,3,H,W]  0: ("source_left",0) frame -1, 1: ("source_right",0) frame +1 */
    const float* disp[DVS_MAX_SCALES]; /* [B,1,hs,ws] outputs[("disp",s)] */
    const float* K;                  /* [B,4,4]    sample[("K",0)] */
    const float* inv_K;              /* [B,4,4]    sample[("inv_K",0)] */
    const float* T[2];               /* [B,4,4]    outputs[("cam_T_cam",0,-1/+1)] */
    const float* noise;              /* [S,B,2,H,W] standard-normal tie-break noise (x1e-5 applied
                                        inside), or NULL: counter-based Philox noise from `seed` */
    uint64_t seed;
    /* workspace (sizes from dvs_chain_workspace) */
    float* partials;                 /* per-block partial sums */
    uint8_t* sel;                    /* [B,H,W] argmin of the 4-way min, 2 bits per scale */
    float* stats;                    /* [B,S,4] per-image sums {min-loss, disp_up, Gx, Gy}, followed by a per-image camera
                                        table (inv_K[:3,:3], (K.T_-1)[:3,:], (K.T_+1)[:3,:]) and RGBA-packed copies of the two
                                        source frames (2*B*H*W*16 bytes) that the forward call writes and the backward call
                                        reads: allocate dvs_chain_workspace's stats_bytes and keep it until the backward */
    /* outputs */
    float* losses;                   /* [S] losses["loss/s"] */
    /* optional materialised tensors of the reference's `outputs` dict (NULL = skip) */
    float* disp_up[DVS_MAX_SCALES];  /* [B,1,H,W]   ("disp_up",s) */
    float* depth[DVS_MAX_SCALES];    /* [B,1,H,W]   ("depth",s) */
    float* grid[DVS_MAX_SCALES][2];  /* [B,H,W,2]   ("sample",f,s) */
    float* color[DVS_MAX_SCALES][2]; /* [B,3,H,W]   ("color",f,s) */
} dvs_chain_fwd_io;

typedef struct {
    const float* d_losses;           /* [S] upstream gradient of losses["loss/s"] */
    float* d_disp[DVS_MAX_SCALES];   /* [B,1,hs,ws]; overwritten (zero-filled inside where needed) */
    float* d_T[2];                   /* [B,4,4] gradient wrt cam_T_cam(-1/+1) */
    float* bwd_partials;             /* workspace */
    int scale_begin, scale_end;      /* scales [begin, end) handled by this call; 0, 0 = all of them */
    int phase;                       /* 0: gradient kernel + d_T reduction; 1: gradient kernel only; 2: d_T reduction only
                                        (after calls with phase 1 have covered every scale) -- lets a caller launch the
                                        scales on different streams and hand d disp_0 to the decoder's backward first */
} dvs_chain_bwd_io;

/* Bytes of each workspace buffer for a configuration (host out-params). */
int dvs_chain_workspace(const dvs_chain_cfg* cfg, size_t* partials_bytes, size_t* sel_bytes,
                        size_t* stats_bytes, size_t* bwd_partials_bytes);
int dvs_chain_fwd(const dvs_chain_cfg* cfg, const dvs_chain_fwd_io* io, void* stream);
/* Needs the same inputs/workspace as the forward call it differentiates (sel, stats filled). */
int dvs_chain_bwd(const dvs_chain_cfg* cfg, const dvs_chain_fwd_io* io, const dvs_chain_bwd_io* g,
                  void* stream);

/* ---------------------------------------------------------------------------------------------
 * Standalone (un-fused) operators for callers that use model/layers.py piecewise
 * ------------------------------------------------------------------------------------------- */
/* BackprojectDepth.forward (vo/learner_func.py:130-135): depth [B,1,H,W], inv_K [B,4,4] ->
 * cam_points [B,4,H*W] (row 3 = 1).  bwd: d_depth = sum_{r<3} d_cam[r] * (inv_K[:3,:3].[x,y,1])[r]. */
int dvs_backproject_fwd(const float* depth, const float* inv_K, float* cam_points, int B, int H, int W,
                        void* stream);
int dvs_backproject_bwd(const float* d_cam_points, const float* inv_K, float* d_depth, int B, int H,
                        int W, void* stream);

/* Project3D.forward (vo/learner_func.py:148-159): points [B,4,H*W], K,T [B,4,4] -> grid [B,H,W,2]
 * normalised to [-1,1].  bwd: d_points [B,4,H*W], d_T [B,4,4]; workspace bytes from
 * dvs_project_bwd_workspace. */
int dvs_project_fwd(const float* points, const float* K, const float* T, float* grid, int B, int H,
                    int W, float eps, void* stream);
size_t dvs_project_bwd_workspace(int B, int H, int W);
int dvs_project_bwd(const float* points, const float* K, const float* T, const float* d_grid,
                    float* d_points, float* d_T, float* workspace, int B, int H, int W, float eps,
                    void* stream);

/* SSIM.forward (vo/learner_func.py:193-207) on `planes` = B*C independent [H,W] planes:
 * clamp((1 - SSIM)/2, 0, 1) with ReflectionPad2d(1) + AvgPool2d(3,1).  bwd: d_x and/or d_y (either
 * may be NULL). */
int dvs_ssim_fwd(const float* x, const float* y, float* out, int planes, int H, int W, void* stream);
int dvs_ssim_bwd(const float* x, const float* y, const float* d_out, float* d_x, float* d_y,
                 int planes, int H, int W, void* stream);

/* get_smooth_loss (vo/learner_func.py:161-174): disp [B,1,H,W], img [B,C,H,W] -> out[1] (device
 * scalar).  bwd: d_disp = d_out[0] * d out / d disp (the image is data). */
size_t dvs_smooth_workspace(int B, int H, int W);
int dvs_smooth_fwd(const float* disp, const float* img, float* out, float* workspace, int B, int C,
                   int H, int W, void* stream);
int dvs_smooth_bwd(const float* disp, const float* img, const float* d_out, float* d_disp, int B,
                   int C, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * the supervised depth learner's multi-scale loss, depth/depth_learner.py:51-117
 *     (DepthLearner.multi_scale_loss: F.interpolate bilinear of each scale's depth to (H, W), get_smooth_loss on the
 *     mean-normalised map, silog_loss over the valid pixels).  One forward launch for all scales, one backward launch.
 *       pred_depth[s] [B,1,hs,ws] (disp_to_depth already applied, as the reference's pred_depths list),
 *       gt_depth [B,1,H,W], valid_mask [B,1,H,W] bytes (non-zero = valid), rgb [B,3,H,W];
 *       out [2*S] (device): silog_s for s < S, then smooth_s;  d_out [2*S]: their upstream gradients;
 *       d_pred_depth[s] [B,1,hs,ws], overwritten.  workspace: dvs_depth_loss_workspace bytes, filled by the forward
 *       call and read by the backward call.  No valid pixel at all gives NaN, as the reference's mean over nothing does.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int B, H, W;
    int num_scales;
    int hs[DVS_MAX_SCALES];
    int ws[DVS_MAX_SCALES];
    float variance_focus;            /* 0.85, depth_learner.py:80 */
} dvs_depth_loss_cfg;
size_t dvs_depth_loss_workspace(const dvs_depth_loss_cfg* cfg);
int dvs_depth_loss_fwd(const dvs_depth_loss_cfg* cfg, const float* const* pred_depth, const float* gt_depth,
                       const unsigned char* valid_mask, const float* rgb, float* workspace, float* out, void* stream);
int dvs_depth_loss_bwd(const dvs_depth_loss_cfg* cfg, const float* const* pred_depth, const float* gt_depth,
                       const unsigned char* valid_mask, const float* rgb, float* workspace, const float* d_out,
                       float* const* d_pred_depth, void* stream);

/* ---------------------------------------------------------------------------------------------
 * the input side of the path, vo/dataset/common.py:38-92, behind the H2D copy
 *   dvs_u8_to_f32_planar: src uint8 [N,H,W,3] (RGB, or BGR with bgr != 0) -> dst fp32 [N,3,H,W] (RGB planes) / 255:
 *       transforms.ToTensor of common.py:77; with bgr the preprocessing of slam/network.py:42-50.  H*W % 4 == 0,
 *       src 4-byte and dst 16-byte aligned.
 *   dvs_color_jitter: torchvision ColorJitter (common.py:31-37,79-81) in place on images fp32 [N,3,H,W] in [0,1].
 *       records (device): N x { int order[4]; float factor[4]; } -- order = adjustment ids in application order
 *       (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none), factor[id] = that adjustment's factor (hue: the shift
 *       in [-0.5, 0.5]).  Images that share a record's values get the same jitter (the reference jitters the three frames
 *       of a sample together); the contrast step's mean gray level is per image.  workspace: dvs_color_jitter_workspace
 *       bytes.
 *   dvs_resample_u8: one pass of PIL's Image.resize(size, Image.BILINEAR) on uint8 frames [N,h,w,3] (common.py:38-44:
 *       antialiased triangle filter, 22-bit integer coefficients, uint8 rounding after each pass) -- bit exact.  axis 0
 *       resamples along x ([N,h,in_w,3] -> [N,h,out_w,3]), axis 1 along y; bounds [out_n][2] = (first input index, tap
 *       count), coef [out_n][ksize] integer taps, both built on the host exactly as Pillow does
 *       (input_pipeline.pil_bilinear_tables).  A full resize = the x pass, then the y pass.
 */
int dvs_resample_u8(const unsigned char* src, unsigned char* dst, const int* bounds, const int* coef, int ksize, int N, int in_h,
                    int in_w, int out_h, int out_w, int axis, void* stream);
int dvs_u8_to_f32_planar(const unsigned char* src, float* dst, int N, int H, int W, int bgr, void* stream);
size_t dvs_color_jitter_workspace(int N, int H, int W);
int dvs_color_jitter(float* images, const void* records, float* workspace, int N, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a14 / SURVEY.md 8(f) rank 1: Depth-Anything-V2 ViT-S (BASELINE.json configs[4]) -- forward kernels beside the
 *     implicit-GEMM engine (the token GEMMs are dvs_conv2d_fwd calls on [1,1,M,K] tensors).
 *   dvs_attention_fwd: out [B,N,heads*64] = softmax(q k^T * scale) v per head from qkv [B,N,3,heads,64] (the output of the
 *       qkv Linear; lse may be NULL), model/depth_anything_v2/dinov2_layers/attention.py:49-62; flash style on the fp32 matrix cores.
 *   dvs_layernorm_fwd: nn.LayerNorm(C, eps) over the last dimension of x [M,C] (block.py:53,67; dinov2.py:166).
 *   dvs_vit_patchify: image [B,3,H,W] -> rows [B*(H/p)*(W/p)][k_padded], row = one patch in (ci, ky, kx) order, zero padded
 *       to k_padded (>= 3 p p, % 4 == 0): the A operand of PatchEmbed.proj (patch_embed.py:69-82).
 *   dvs_vit_assemble: x [B,Np+1,C] = cat(cls_token, patch_tokens [B,Np,C]) + pos_embed [Np+1,C] (dinov2.py:219-229).
 *   dvs_resize_bilinear_ac: F.interpolate(mode="bilinear", align_corners=True) of an NHWC map [B,h,w,C] to [B,H,W,C]
 *       (util/blocks.py:143, dpt.py:145).
 *   dvs_deconv_shuffle: y [B,h*k,w*k,Cout] from g [B,h,w,k*k*Cout] = the 1x1 product of the input with the ConvTranspose2d
 *       weight arranged [(a*k+c)*Cout+co][ci]: nn.ConvTranspose2d(kernel_size=k, stride=k) of dpt.py:60-73.
 * ------------------------------------------------------------------------------------------- */
int dvs_attention_fwd(const float* qkv, float* out, float* lse, int B, int N, int heads, int head_dim, float scale, void* stream);
int dvs_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, int M, int C, float eps, void* stream);
/* Backward halves (training of the encoder swap).  lse [B,heads,N]: log-sum-exp of every score row, written by
 * dvs_attention_fwd when non-NULL.  dvs_attention_bwd: d_qkv [B,N,3,heads,64] from d_out [B,N,heads*64] (delta [B,heads,N] is
 * scratch); two recomputing kernels in the forward's register layout, no atomics.  dvs_layernorm_bwd: dx, and
 * dgamma_acc / dbeta_acc += (caller zero-fills or accumulates).  dvs_act_fwd / dvs_act_bwd_in: ReLU (1) / GELU (4) as
 * their own passes, the derivative taken from the activation's INPUT.  dvs_resize_bilinear_ac_bwd: dx [B,h,w,C] (zero-filled
 * inside) from dy [B,H,W,C].  dvs_deconv_unshuffle: the inverse permutation of dvs_deconv_shuffle. */
int dvs_attention_bwd(const float* qkv, const float* out, const float* d_out, const float* lse, float* delta, float* d_qkv, int B,
                      int N, int heads, int head_dim, float scale, void* stream);
int dvs_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma_acc, float* dbeta_acc, int M, int C,
                      float eps, void* stream);
int dvs_act_fwd(const float* x, float* y, size_t n, int act, void* stream);
int dvs_act_bwd_in(const float* x, const float* dy, float* dx, size_t n, int act, void* stream);
int dvs_resize_bilinear_ac_bwd(const float* dy, float* dx, int B, int h, int w, int H, int W, int C, void* stream);
int dvs_deconv_unshuffle(const float* dy, float* dg, int B, int h, int w, int k, int Cout, void* stream);
int dvs_vit_patchify(const float* image, float* rows, int B, int H, int W, int patch, int k_padded, void* stream);
int dvs_vit_assemble(const float* patch_tokens, const float* cls_token, const float* pos_embed, float* x, int B, int num_patches,
                     int C, void* stream);
int dvs_resize_bilinear_ac(const float* x, float* y, int B, int h, int w, int H, int W, int C, void* stream);
int dvs_deconv_shuffle(const float* g, float* y, int B, int h, int w, int k, int Cout, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (ABI 9) output stage of the inference path: world pose chain and coloured point cloud
 *     replaces the per-frame host work of the three inference callers after the two networks:
 *       ros2_ws/src/vo_visualizer/vo_visualizer/visualizer_node.py:26-56,128-191 (meshgrid, back-projection, colours,
 *         create_pointcloud2's 16-byte records, world_pose @ T, quaternion of the world pose),
 *       vo/predict.py:69-98 + vo/utils/visualization.py:157-193 (the same + world_pose @ points + the y flip),
 *       vo/eval_traj.py:85-121,138-147 (z > 0 mask in pixel order, K^-1, T_global @ points, T_global @= T_local).
 *
 *   Per kept pixel (v, u) of image b, in fp32:
 *       z = depth[b,0,v,u]     or, from_disp:  z = 1 / (1/max_depth + (1/min_depth - 1/max_depth) * disp[b,0,v,u])
 *       x = (u - cx) / fx * z,  y = (v - cy) / fy * z         fx, fy, cx, cy read on the device from K[b]
 *       p = M[b] . (x, y, z, 1)                               M = NULL: camera frame
 *       record = { p.x, p.y, p.z, bit-cast<float>(r << 16 | g << 8 | b) },  c = (uint8) clamp(image[b,c,v,u] * 255, 0, 255)
 *   Kept pixels: (i * stride_y, j * stride_x); capacity per image n_max = ceil(H / stride_y) * ceil(W / stride_x).
 *   compact = 0: every kept pixel is written, record k is kept pixel k in row-major order, count[b] = n_max.
 *   compact = 1: only pixels with z_lo < z and (z_hi > 0: z < z_hi) are written, contiguous from records[b][0] in row-major
 *       pixel order (numpy boolean-mask order); count[b] is their number; nothing at or beyond records[b][count[b]] is
 *       touched.  Needs `workspace` (dvs_cloud_workspace bytes, device).  index (optional): v * W + u of every record.
 *   depth_or_disp [B,1,H,W], image [B,3,H,W], K [B,k_row_stride,k_row_stride] (3 or 4), M [B,4,4] or NULL,
 *   records [B,n_max,4] (16-byte aligned), count [B] int32, index [B,n_max] int32 or NULL.  All device memory.
 *
 *   dvs_pose_chain: world <- world . T[b] for b = 0 .. B-1; after step b: poses[b] = world, M[b] = left . world (left NULL:
 *       M[b] = world), tq[b] = (tx, ty, tz, qx, qy, qz, qw) of world with a unit quaternion, qw >= 0.  T [B,4,4], left [4,4] or
 *       NULL, world [4,4] updated in place (persistent device state), poses / M [B,4,4] or NULL, tq [B,7] or NULL.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int B, H, W;
    int stride_y, stride_x;          /* >= 1 */
    int from_disp;                   /* 1: the input is ("disp", 0) and disp_to_depth (model/layers.py:16-26) is applied inside */
    int compact;
    int k_row_stride;                /* 3 or 4 */
    float min_depth, max_depth;      /* from_disp only */
    float z_lo, z_hi;                /* compact only; z_hi <= 0: no upper bound */
} dvs_cloud_cfg;
int dvs_cloud_capacity(const dvs_cloud_cfg* cfg, int* n_max);
size_t dvs_cloud_workspace(const dvs_cloud_cfg* cfg);
int dvs_cloud_fwd(const dvs_cloud_cfg* cfg, const float* depth_or_disp, const float* image, const float* K, const float* M,
                  float* records, int* count, int* index, void* workspace, void* stream);
int dvs_pose_chain(const float* T, const float* left, float* world, float* poses, float* M, float* tq, int B, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (ABI 10) RAFT correlation block: all-pairs volume, average-pool pyramid, windowed bilinear lookup, and their backward
 *     replaces model/raft/core/corr.py:12-60 (CorrBlock) with bilinear_sampler, model/raft/core/utils/utils.py:57-71, as
 *     model/raft/core/raft.py:82-102 uses them (fp32 whatever the autocast state, coordinates detached).
 *
 *   N = H * W positions p, q in row-major order; level i has h_i x w_i = (H >> i) x (W >> i) cells, n_i = h_i * w_i.
 *       V_0[b][p][q] = sum_c fmap1[b][c][p] * fmap2[b][c][q] / sqrt(C)
 *       V_i[b][p][.] = avg_pool2d(V_{i-1}[b][p][.], 2, stride 2)                                       (corr.py:25-27)
 *       out[b][i * (2r+1)^2 + a * (2r+1) + e][p] = bilinear sample of V_i[b][p] at (x / 2^i + a - r, y / 2^i + e - r),
 *           (x, y) = coords[b][0..1][p], pixel coordinates (align_corners), zero padding, floor for negative values.  The x
 *           offset is the slow index (corr.py:37-43 stacks meshgrid(dy, dx) onto (x, y)).  A coordinate that is not finite, or
 *           further than r + 2 outside the map, samples nothing: every tap of that pixel and level is 0.
 *   Pyramid buffer: level i is a contiguous [B * N][n_i] matrix at float offset level_offsets[i]; pyramid_floats in all.
 *   Feature maps: position-major [B][N][C] (the memory of a channels_last tensor) or, with fmap*_nchw = 1, [B][C][N], which is
 *       transposed once into the workspace.  C % 4 == 0, 16-byte aligned.  Every level needs >= 2 rows and columns (the
 *       reference returns NaN below that), N * N < 2^31, num_levels <= 8, radius <= 8.
 *   The workspace (dvs_corr_sizes, device, 16-byte aligned) is written by dvs_corr_build and must reach dvs_corr_volume_bwd
 *       unchanged: it holds the pooled rows of fmap2 and the position-major copies.
 *   dvs_corr_lookup_fwd: out [B][L * (2r+1)^2][N], or out_nhwc = 1: [B][N][L * (2r+1)^2].
 *   dvs_corr_lookup_bwd: dpyramid (the pyramid's layout) += the gradient of one lookup; the caller zeroes it once and every
 *       lookup of the block adds into it (one owner per element: no atomics, bit-reproducible).  No gradient for coords
 *       (raft.py:101 detaches them).
 *   dvs_corr_volume_bwd: dfmap1, dfmap2 [B][N][C] (overwritten) from the accumulated dpyramid, the pool backward included.
 *   dvs_set_precision does not affect these kernels.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int B, C, H, W;
    int num_levels, radius;
    int fmap1_nchw, fmap2_nchw;      /* 0: [B][N][C] read in place, 1: [B][C][N] */
} dvs_corr_cfg;
int dvs_corr_sizes(const dvs_corr_cfg* cfg, size_t* pyramid_floats, size_t* level_offsets, size_t* workspace_bytes);
int dvs_corr_build(const dvs_corr_cfg* cfg, const float* fmap1, const float* fmap2, float* pyramid, void* workspace, void* stream);
int dvs_corr_lookup_fwd(const dvs_corr_cfg* cfg, const float* pyramid, const float* coords, float* out, int out_nhwc, void* stream);
int dvs_corr_lookup_bwd(const dvs_corr_cfg* cfg, const float* coords, const float* dout, int dout_nhwc, float* dpyramid,
                        void* stream);
int dvs_corr_volume_bwd(const dvs_corr_cfg* cfg, const float* dpyramid, const float* fmap1, const float* fmap2, void* workspace,
                        float* dfmap1, float* dfmap2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (ABI 11) RAFT correlation block, on-the-fly form: the lookup without the volume
 *     replaces AlternateCorrBlock, model/raft/core/corr.py:63-91, and the kernels behind it, model/raft/alt_cuda_corr/; unlike the
 *     reference's Python, which never wires alt_cuda_corr.backward into autograd, the gradients of both feature maps are here.
 *
 *   With N, h_i, w_i, coords and the channel order as above, and f2_i = avg_pool2d applied i times to fmap2 (2 x 2, stride 2):
 *       s_i(p, q) = sum_c fmap1[b][c][p] * f2_i[b][c][q] / sqrt(C)
 *       out[b][i * (2r+1)^2 + a * (2r+1) + e][p] = bilinear blend, zero padding, of s_i(p, .) at (x / 2^i + a - r, y / 2^i + e - r)
 *   Pooling is linear, so this is the function dvs_corr_build + dvs_corr_lookup_fwd compute; only the (2r+2)^2 values s_i(p, q) that
 *   a pixel's taps touch are formed, inside the lookup, and nothing of size N * N exists.  Non-finite and far-outside coordinates
 *   give exact zeros as above.
 *   Same dvs_corr_cfg and limits (C % 4 == 0, num_levels <= 8, radius <= 8, >= 2 rows and columns on every level, B * N * C < 2^31)
 *       EXCEPT N * N < 2^31, which is replaced by B * L * (2r+1)^2 * N < 2^31.  dvs_altcorr_sizes checks them all.
 *   pooled: the rows of f2_1 .. f2_{L-1}, [B][n_1 + .. + n_{L-1}][C], pooled_floats floats (4 when L = 1: nothing is stored, the
 *       buffer only needs an address), 16-byte aligned.  dpooled has the same layout.
 *   workspace (workspace_bytes, device, 16-byte aligned): the position-major copies of feature maps given as [B][C][N]; written by
 *       dvs_altcorr_pool, read by dvs_altcorr_fwd and dvs_altcorr_bwd.
 *   dvs_altcorr_pool:   transposes fmap*_nchw maps into the workspace and writes `pooled`.  Once per pair of feature maps.
 *   dvs_altcorr_fwd:    out [B][L * (2r+1)^2][N], or out_nhwc = 1: [B][N][L * (2r+1)^2].  Fixed summation order: bit-reproducible.
 *   dvs_altcorr_bwd:    the gradient of ONE lookup for the cotangent dout (layout as out).
 *                           dfmap1 [B][N][C] is overwritten; one owner per element and a fixed order: bit-reproducible.
 *                           dfmap2 [B][N][C] and dpooled are ADDED into with fp32 atomic adds (the windows of many pixels share a
 *                           row); the caller zeroes them.  Their last bits depend on the arrival order: NOT bit-reproducible.
 *                       No gradient for coords.
 *   dvs_altcorr_unpool: dfmap2 [B][N][C] += the average-pool backward of dpooled (one owner per element: bit-reproducible given
 *                       its input).
 *   dvs_set_precision does not affect these kernels.
 * ------------------------------------------------------------------------------------------- */
int dvs_altcorr_sizes(const dvs_corr_cfg* cfg, size_t* pooled_floats, size_t* workspace_bytes);
int dvs_altcorr_pool(const dvs_corr_cfg* cfg, const float* fmap1, const float* fmap2, float* pooled, void* workspace, void* stream);
int dvs_altcorr_fwd(const dvs_corr_cfg* cfg, const float* fmap1, const float* fmap2, const float* pooled, const void* workspace,
                    const float* coords, float* out, int out_nhwc, void* stream);
int dvs_altcorr_bwd(const dvs_corr_cfg* cfg, const float* fmap1, const float* fmap2, const float* pooled, const void* workspace,
                    const float* coords, const float* dout, int dout_nhwc, float* dfmap1, float* dfmap2, float* dpooled, void* stream);
int dvs_altcorr_unpool(const dvs_corr_cfg* cfg, const float* dpooled, float* dfmap2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 11: four new entry points, nothing existing changes) ConvGRU gate arithmetic
 *     replaces the elementwise half of ConvGRU.forward, model/raft/core/update.py:23-31 (torch.cat, torch.sigmoid, torch.tanh,
 *     r*h, (1-z)*h + z*q); the three convolutions stay convolutions (dvs_conv2d_*), split by input-channel block.
 *
 *   P = B*H*W pixel rows of channels_last tensors, hd = hidden channels (hd % 4 == 0).  Row-major fp32 matrices, 16-byte aligned:
 *       a_h [P][2hd]  conv(h), columns (z, r)             a_x [P][3hd]  conv(motion features), columns (z, r, q)
 *       c   [P][3hd]  conv(inp) + (bz, br, bq)            a_q [P][hd]   conv(r * h)
 *   dvs_gru_gates_fwd:  z = sigmoid((a_h[:, :hd] + a_x[:, :hd]) + c[:, :hd]),  r likewise on the next hd columns,  rh = r * h
 *   dvs_gru_blend_fwd:  q = tanh((a_q + a_x[:, 2hd:]) + c[:, 2hd:]),  h_new = (1 - z) * h + z * q
 *   dvs_gru_blend_bwd:  for g = dL/dh_new:  dq = g * z * (1 - q^2),  dz = g * (q - h) * z * (1 - z),  dh_a = g * (1 - z)
 *                       writes dpre[:, :hd] = dah[:, :hd] = dz,  dpre[:, 2hd:] = dq (also as the matrix dq [P][hd]),  dh_a [P][hd]
 *   dvs_gru_gates_bwd:  for d_rh = dL/d(r*h):  dr = d_rh * h * r * (1 - r),  dh = dh_a + d_rh * r
 *                       writes dpre[:, hd:2hd] = dah[:, hd:] = dr,  dh [P][hd]
 *   After both backward calls dpre [P][3hd] is the gradient of a_x and of c, dah [P][2hd] that of a_h, dq that of a_q.
 *   expf / tanhf of the HIP math library; saturated pre-activations give exact 0, 1, -1 limits (subnormals kept), never a NaN.
 *   Every output element is written once by one thread, no atomics: bit-reproducible.  64-bit element offsets.
 *   DVS_ERR_INVALID for a null or misaligned pointer, hidden <= 0, hidden % 4 != 0, P == 0.
 *   dvs_set_precision does not affect these kernels.
 * ------------------------------------------------------------------------------------------- */
int dvs_gru_gates_fwd(const float* a_h, const float* a_x, const float* c, const float* h, float* z, float* r, float* rh, size_t P,
                      int hidden, void* stream);
int dvs_gru_blend_fwd(const float* a_q, const float* a_x, const float* c, const float* z, const float* h, float* q, float* h_new,
                      size_t P, int hidden, void* stream);
int dvs_gru_blend_bwd(const float* g, const float* z, const float* q, const float* h, float* dpre, float* dah, float* dq, float* dh_a,
                      size_t P, int hidden, void* stream);
int dvs_gru_gates_bwd(const float* d_rh, const float* h, const float* r, const float* dh_a, float* dpre, float* dah, float* dh,
                      size_t P, int hidden, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 11: new entry points only) Instance norm with the Bottleneck tail fused
 *     replaces nn.InstanceNorm2d + ReLU + the residual add + ReLU of BottleneckBlock.forward, model/raft/core/extractor.py:107-116,
 *     and, with norm = 0, the same tail of the 'none' encoder.
 *
 *   fp32 NHWC activations [N][HW][C], C % 4 == 0 (4 .. 1024), HW >= 2, N <= 65535, 16-byte aligned.
 *       z   = norm ? (y - mean[n][c]) * invstd[n][c] : y        mean, biased variance over the HW pixels of image n, eps = 1e-5,
 *       z   = relu ? max(z, 0) : z                              no affine parameters, no running statistics
 *       out = residual ? max(residual + z, 0) : z               residual == NULL: none
 *   table [N][2][C] (mean, invstd), written by the forward with norm = 1 and read by the backward; NULL allowed with norm = 0.
 *   dvs_inorm_bwd: for dout = dL/dout, with `out` the forward's output (and dresidual) exactly when there was a residual:
 *       g  = residual ? dout * [out > 0] : dout                 written to dresidual
 *       du = relu ? g * [z > 0] : g                             z recomputed from y and the table by the forward's own expression
 *       dy = norm ? invstd * (du - mean_hw(du) - xhat * mean_hw(du * xhat)) : du
 *   Statistics: per slice of dvs_inorm_slice_pixels() = 1024 pixels the mean first, then the squared deviations around it; the
 *       slices' (count, mean, M2) are merged with Chan's formula.  No sum of squares minus squared mean, no atomics, a fixed
 *       order: bit-reproducible, and an image's result does not depend on the other images of the batch.
 *   workspace: dvs_inorm_workspace(N, HW, C) bytes (0 for invalid arguments), device memory, 16-byte aligned, needed with norm = 1;
 *       the backward may reuse the forward's.
 *   DVS_ERR_INVALID, before any launch, for a null or misaligned pointer, C % 4 != 0, HW < 2, N or HW out of range, a workspace
 *       that is too small.  dvs_set_precision does not affect these kernels.
 * ------------------------------------------------------------------------------------------- */
int dvs_inorm_slice_pixels(void);
size_t dvs_inorm_workspace(int N, size_t HW, int C);
int dvs_inorm_fwd(const float* y, const float* residual, float* out, float* table, void* workspace, size_t workspace_bytes, int N,
                  size_t HW, int C, int norm, int relu, void* stream);
int dvs_inorm_bwd(const float* dout, const float* y, const float* out, const float* table, float* dy, float* dresidual,
                  void* workspace, size_t workspace_bytes, int N, size_t HW, int C, int norm, int relu, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 11: new entry points only) upflow8
 *     replaces upflow8, model/raft/core/utils/utils.py:80-82: 8 * F.interpolate(flow, 8x, mode='bilinear', align_corners=True)
 *
 *   flow [N][2][h][w] (flow_nchw = 1) or [N][h][w][2] (flow_nchw = 0, channels_last memory); out [N][2][8h][8w] planar.
 *   torch's index arithmetic in fp32: scale = (in - 1) / (out - 1), src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1),
 *   l1 = src - i0, l0 = 1 - l1; the factor 8 is applied to the finished blend.
 *   dvs_upflow8_bwd: dflow (layout by dflow_nchw, overwritten) = the adjoint applied to dout [N][2][8h][8w]: a gather with the
 *   forward's weights, fixed order, no atomics.  Both directions are bit-reproducible.
 *   N <= 65535, h, w >= 1, 64 * h * w < 2^31; 16-byte aligned pointers.  DVS_ERR_INVALID before any launch otherwise.
 * ------------------------------------------------------------------------------------------- */
int dvs_upflow8_fwd(const float* flow, float* out, int N, int h, int w, int flow_nchw, void* stream);
int dvs_upflow8_bwd(const float* dout, float* dflow, int N, int h, int w, int dflow_nchw, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 12: new entry points only) FlowPoseNet's pooling head
 *     replaces nn.ReLU, nn.AdaptiveAvgPool2d(1), self.fc and * self.pose_scale, model/posenet_single.py:116-122 and 137-142
 *
 *   y [N][P][C] fp32: the NHWC memory of the last regressor convolution, P = h * w; W [J][C]; b [J] or NULL.
 *       a(v)        = relu ? max(v, 0) : v
 *       mean[n][c]  = (1/P) sum_p a(y[n][p][c])                          [N][C], kept for the backward
 *       out[n][j]   = scale * (b[j] + sum_c W[j][c] * mean[n][c])        [N][J]
 *   dvs_pool_fc_bwd: for dout = dL/dout [N][J]
 *       g[n][c]     = (scale/P) sum_j dout[n][j] * W[j][c]
 *       dy[n][p][c] = g[n][c] * (relu ? [y > 0] : 1)                     y == 0 gives 0, as torch does
 *       dW[j][c]    = scale * sum_n dout[n][j] * mean[n][c]              written, not accumulated
 *       db[j]       = scale * sum_n dout[n][j]                           db == NULL: not computed
 *   Per slice of dvs_pool_fc_slice_pixels() = 256 pixels one mean per channel (workspace [N][S][C]); a second launch folds the
 *       slice means in ascending order and computes the J dot products by a fixed tree.  No atomics, a fixed order: bit-reproducible,
 *       and a sample's out, mean and dy do not depend on the other samples of the batch.
 *   C % 4 == 0 (4 .. 1024), 1 <= J <= 16, 1 <= N <= 65535, 1 <= P < 2^31; 16-byte aligned pointers.
 *   workspace: dvs_pool_fc_workspace(N, P, C) bytes (0 for invalid arguments), device memory, needed by the forward only.
 *   DVS_ERR_INVALID, before any launch, for a null or misaligned pointer, C, J, N or P out of range, a workspace that is too small.
 * ------------------------------------------------------------------------------------------- */
int dvs_pool_fc_slice_pixels(void);                                      /* model/posenet_single.py:117 */
size_t dvs_pool_fc_workspace(int N, long long P, int C);                 /* model/posenet_single.py:117 */
int dvs_pool_fc_fwd(const float* y, const float* W, const float* b, float* out, float* mean, void* workspace, size_t workspace_bytes,
                    int N, long long P, int C, int J, int relu, float scale, void* stream);   /* model/posenet_single.py:137-142 */
int dvs_pool_fc_bwd(const float* dout, const float* y, const float* mean, const float* W, float* dy, float* dW, float* db, int N,
                    long long P, int C, int J, int relu, float scale, void* stream);   /* autograd of model/posenet_single.py:137-142 */

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 12: new entry points only) Convex 8x flow upsampling
 *     replaces RAFT.upsample_flow, model/raft/core/raft.py:170-181 (view, softmax, F.unfold, mul, sum, permute, reshape) and the
 *     `.25 *` of BasicUpdateBlock.forward, model/raft/core/update.py:135
 *
 *   flow [N][2][h][w] planar; mask [N][h][w][576] NHWC, channel k*64 + i*8 + j with tap k = ky*3 + kx; out [N][2][8h][8w] planar.
 *       p_k                    = softmax_k(mask_scale * mask[n][y][x][k*64 + i*8 + j])          the maximum subtracted first
 *       out[n][ch][8y+i][8x+j] = sum_k p_k * 8 * flow[n][ch][y+ky-1][x+kx-1]                    0 outside the map
 *   dvs_convex_up_bwd: for dout = dL/dout, with the softmax recomputed from the mask and t_k = sum_ch dout_ch * 8 * flow_ch(tap k):
 *       dmask[k]               = mask_scale * p_k * (t_k - sum_k' p_k' t_k')                    [N][h][w][576], overwritten
 *       s[n][y][x][k][ch]      = sum_ij p_k * dout_ch                                           the workspace
 *       dflow[n][ch][y'][x']   = 8 * sum_k s[n][y'-ky+1][x'-kx+1][k][ch]                        in-range neighbours, ascending k
 *   expf of the HIP math library on fp32 values; the nine-term sums and the normalisation are carried in fp64 registers and
 *   rounded to fp32 once, so a one-hot softmax returns 8 * flow of its tap exactly and a constant flow its constant.
 *   The mask is read once per direction.  No atomics, a fixed order: both directions are bit-reproducible.  64-bit element offsets.
 *   workspace: dvs_convex_up_workspace(N, h, w) = N*h*w*18*4 bytes (0 for invalid arguments), device memory, backward only.
 *   dflow or dmask (not both) may be NULL: that gradient is not computed; the workspace is needed, and read, with dflow only.
 *   1 <= N <= 65535, h, w >= 1, 64 * h * w < 2^31, finite mask_scale; 16-byte aligned pointers.  DVS_ERR_INVALID, before any
 *   launch, for a null or misaligned pointer, a shape out of range, a workspace that is too small.
 *   dvs_set_precision does not affect these kernels.
 * ------------------------------------------------------------------------------------------- */
size_t dvs_convex_up_workspace(int N, int h, int w);
int dvs_convex_up_fwd(const float* flow, const float* mask, float* out, int N, int h, int w, float mask_scale, void* stream);
int dvs_convex_up_bwd(const float* dout, const float* flow, const float* mask, float* dflow, float* dmask, void* workspace,
                      size_t workspace_bytes, int N, int h, int w, float mask_scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 12: new entry points only) Shift-stack: the five taps of a (1,5) / (5,1) convolution along the channels
 *     lets SepConvGRU's convolutions, model/raft/core/update.py:36-42, run as 1x1 convolutions with K = 5 * Cin
 *
 *   x [N][H][W][C] NHWC, C % 4 == 0; (dy, dx) = (0, 1) for axis 0 (taps along W), (1, 0) for axis 1 (taps along H).
 *       x5[n][y][x][t*C + c] = x[n][y + dy*(t-2)][x + dx*(t-2)][c]   for t = 0 .. 4, 0 outside the map          [N][H][W][5C]
 *   dvs_shift_stack_bwd, the adjoint:
 *       dx[n][y][x][c] = sum_t dx5[n][y - dy*(t-2)][x - dx*(t-2)][t*C + c]   over the in-range sources, in ascending t
 *   A (1,5) convolution with padding (0,2) and filter Wt [Cout][Cin][1][5] is the 1x1 convolution of x5 (axis 0) with
 *   Wt.permute(0,3,2,1).reshape(Cout, 5*Cin, 1, 1); a (5,1) one likewise with axis 1 and the H tap.
 *   One lane moves 16 bytes; no atomics, every element written once: bit-reproducible.  64-bit element offsets.
 *   DVS_ERR_INVALID, before any launch, for a null or misaligned pointer, N, H, W < 1, C <= 0, C % 4 != 0, axis not 0 or 1.
 *   dvs_set_precision does not affect these kernels.
 * ------------------------------------------------------------------------------------------- */
int dvs_shift_stack_fwd(const float* x, float* x5, int N, int H, int W, int C, int axis, void* stream);
int dvs_shift_stack_bwd(const float* dx5, float* dx, int N, int H, int W, int C, int axis, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 12: new entry points only) Warm start: the previous pair's low-resolution flow pushed forward
 *     replaces forward_interpolate, model/raft/core/utils/utils.py:26-54 (a host copy and two scipy griddata(method='nearest') calls)
 *
 *   flow, out [N][2][h][w] fp32 planar, channel 0 = dx, 1 = dy; P = h * w.  Per image, with (xj, yj) the integer grid:
 *       x1[j] = xj + dx[j],  y1[j] = yj + dy[j]                  in fp64 (int64 grid + fp32 flow, as NumPy promotes them)
 *       valid[j]  iff  0 < x1[j] < w  and  0 < y1[j] < h          strictly; a NaN or infinite flow is never valid
 *       d2(i, j)  = (x1[j] - xi)^2 + (y1[j] - yi)^2               fp64, each operation rounded on its own
 *       out[:, i] = flow[:, j*],  j* = the valid j with the smallest d2(i, j), the LOWEST j among equal d2
 *   The reference's KD-tree defines no answer at an exact tie; the lowest row-major source index is this package's definition.
 *   An image without a valid source returns zeros.  The reference has no flow to give there (griddata on zero points returns NaN
 *   under SciPy 1.15); zeros, a cold start, are this package's extension.
 *   A brute-force search, P * P distances per image: a workgroup owns 64 grid pixels, its 16 waves share each tile of 1024 sources
 *   staged in LDS and their answers are merged by the same (d2, j) order, so no split or tile size can change a bit of the result.
 *   No atomics, no workspace; an image's result does not depend on the other images of the batch.
 *   1 <= N <= 65535, h, w >= 1, 1 <= P <= 65536 (the measured time at the cap: DESIGN.md section 21);
 *   4-byte aligned pointers (one image of a batch is a valid argument); out must not overlap flow.  DVS_ERR_INVALID, before any
 *   launch, otherwise.
 *   dvs_set_precision does not affect this entry.
 * ------------------------------------------------------------------------------------------- */
int dvs_forward_interp(const float* flow, float* out, int N, int h, int w, void* stream);   /* utils/utils.py:26-54 */

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 12: new entry points only) Flow colouring
 *     replaces flow_to_image and flow_uv_to_colors, model/raft/core/utils/flow_viz.py:109-132 and 70-106, as called from
 *     model/raft/raft.py:26-68 (a host copy of the full-resolution flow and a NumPy pass)
 *
 *   flow: fp32, u of pixel (n, y, x) at flow[n * 2 * plane_stride + y * row_stride + x] and v one plane_stride further (element
 *   strides), so the un-padded view of a padded [N][2][Hp][Wp] flow is read in place: plane_stride = Hp * Wp, row_stride = Wp.
 *   radmax [N] fp32; out [N][H][W][3] uint8, dense.  clip_flow < 0: no clipping.  Per image, the reference's arithmetic ladder under
 *   NumPy >= 2 scalar promotion (a Python float beside a float32 array stays float32):
 *     fp32, every operation rounded on its own (no contraction), division and square root correctly rounded:
 *       u, v     = clip(u, 0, clip_flow), clip(v, 0, clip_flow)          the lower bound IS 0, as in flow_viz.py:124
 *       radmax   = max over the image of sqrt(u*u + v*v)                 dvs_flow_radmax; a NaN wins, as in np.max
 *       den      = radmax + 1e-5f;  u = u / den;  v = v / den;  rad = sqrt(u*u + v*v)
 *       a        = atan2f(-v, -u) / 3.14159274f;  fk = (a + 1) / 2 * 54
 *     fp64:
 *       k0 = floor(fk);  k1 = k0 + 1, 55 -> 0;  f = fk - k0;  c = wheel / 255.0
 *       col      = (1 - f) * c[k0] + f * c[k1];   col = rad <= 1 ? 1 - rad * (1 - col) : 0.75 * col;   byte = floor(255 * col)
 *   bgr = 1 stores the channels in reverse.  atan2f is the HIP math library's: the one operation of the ladder that is correctly
 *   rounded on neither side, so a byte whose value sits on a floor() boundary may differ by one from NumPy's (tests/test_flowstage_gpu.py
 *   states the rule).  The 55 x 3 wheel is computed from the six segment lengths 15, 6, 4, 11, 13, 6; k0 is clamped to 0 .. 54 before
 *   it indexes the table and the byte to 0 .. 255, so no input value (NaN, infinity) can read or write outside.
 *   dvs_flow_radmax: a zero-fill launch (a kernel, so that a captured graph orders it) and one launch; the only atomic is an INTEGER atomicMax on the bit pattern of a
 *   non-negative fp32, and a maximum is exact in any order: the result does not depend on the launch geometry.
 *   dvs_flow_to_image: reads radmax from device memory (no host synchronisation between the two calls); 8 bytes read and 3 written
 *   per pixel; a lane stores four pixels as three dwords, and reads them as two float4 where W, both strides and the pointer are
 *   multiples of 4 elements / 16 bytes.
 *   1 <= N <= 65535, H, W >= 1, N * H * W < 2^31, row_stride >= W, plane_stride >= (H - 1) * row_stride + W, clip_flow not NaN,
 *   bgr 0 or 1; flow and radmax 4-byte, out 16-byte aligned.  DVS_ERR_INVALID, before any launch, otherwise.
 *   dvs_set_precision does not affect these entries.
 * ------------------------------------------------------------------------------------------- */
int dvs_flow_radmax(const float* flow, long long plane_stride, long long row_stride, int N, int H, int W, float clip_flow,
                    float* radmax, void* stream);                                           /* utils/flow_viz.py:123-128 */
int dvs_flow_to_image(const float* flow, long long plane_stride, long long row_stride, const float* radmax, unsigned char* out, int N,
                      int H, int W, float clip_flow, int bgr, void* stream);              /* utils/flow_viz.py:70-106, 129-132 */

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 12: new entry points only) Frame ingest: a decoder's uint8 frame as the RAFT encoders' first operand
 *     replaces load_image's .float() and /= 255.0 (model/raft/raft.py:22-23), InputPadder.pad (model/raft/core/utils/utils.py:7-21),
 *     2 * image - 1.0 (model/raft/core/raft.py:70-71, 188-190) and the NHWC / zero-channel form conv1 reads, in one launch
 *
 *   src: uint8, N frames of H x W pixels of 3 bytes (RGB; BGR with bgr = 1), pixel (n, y, x) at src + n * image_stride +
 *   y * row_stride + 3 * x (byte strides), so a crop of a larger frame and a batch slice are read in place.
 *   dst: fp32 [N][Hp][Wp][4] dense, Hp = top + H + bottom, Wp = left + W + right.  fp32, every operation rounded on its own (no
 *   contraction), the division correctly rounded (the reference divides on the host):
 *       q               = float(src[n, clamp(y - top, 0, H - 1), clamp(x - left, 0, W - 1), bgr ? 2 - c : c]) / 255.0f
 *       dst[n, y, x, c] = 2.0f * q - 1.0f          c < 3; 2 * q is exact
 *       dst[n, y, x, 3] = 0
 *   which is bit for bit what the reference's chain gives on the CPU (ATen's device-side tensor / scalar may multiply by a
 *   reciprocal and is not the yardstick).  The replicate padding is the clamp; no branch on the border.
 *   A lane owns four consecutive output pixels of a row and stores each as one 16-byte vector; it reads their 12 source bytes as
 *   three dwords where src, both strides, W and left are multiples of 4, single bytes otherwise.  No LDS, no atomics, no
 *   workspace; a frame's result does not depend on the other frames of the batch.
 *   1 <= N <= 65535, H, W >= 1, every pad in 0 .. 7, row_stride >= 3 * W, image_stride >= (H - 1) * row_stride + 3 * W, bgr 0 or 1,
 *   Hp * ceil(Wp / 4) < 2^31; dst 16-byte aligned, src at any byte.  DVS_ERR_INVALID, before any launch, otherwise.
 *   dvs_set_precision does not affect this entry.
 * ------------------------------------------------------------------------------------------- */
int dvs_frame_ingest(const unsigned char* src, long long image_stride, long long row_stride, float* dst, int N, int H, int W,
                     int left, int right, int top, int bottom, int bgr, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 12: new entry points only) Forward-backward consistency of two flows: a validity / occlusion mask per pixel
 *     the criterion of UnFlow (Meister et al. 2018, eq. 2): |w_f + w_b(x + w_f)|^2 < alpha (|w_f|^2 + |w_b(x + w_f)|^2) + beta;
 *     the gather is bilinear_sampler (model/raft/core/utils/utils.py:57-71) in pixel coordinates, without its normalise round trip;
 *     replaces a grid_sample and half a dozen elementwise launches per frame
 *
 *   a, b: fp32 flows of N images of H x W pixels, a on image 1's grid and b on image 2's; u of pixel (n, y, x) of a at
 *   a[n * a_image_stride + y * a_row_stride + x] and v one a_plane_stride further (element strides; b alike), so the un-padded view
 *   of a padded [N][2][Hp][Wp] flow is read in place.  valid_a, valid_b: uint8 [N][H][W]; excess_a, excess_b: fp32 [N][H][W]; all
 *   dense, each may be NULL (all four NULL: nothing is launched).  One launch computes both directions; for pixel (x, y) of
 *   direction a, in fp32, every operation rounded on its own (no contraction), in exactly this order:
 *       qx = float(x) + a.u(x,y)          qy = float(y) + a.v(x,y)
 *       inside = 0 <= qx <= W-1  and  0 <= qy <= H-1          (closed; false for NaN)
 *       x0 = floor(qx), y0 = floor(qy), wx = qx - x0, wy = qy - y0, x1 = min(x0+1, W-1), y1 = min(y0+1, H-1)
 *       s(p) = (p[y0,x0]*(1-wx) + p[y0,x1]*wx)*(1-wy) + (p[y1,x0]*(1-wx) + p[y1,x1]*wx)*wy      for p = b.u, b.v  ->  bu, bv
 *       sx = a.u + bu, sy = a.v + bv
 *       d   = sx*sx + sy*sy
 *       m   = (a.u*a.u + a.v*a.v) + (bu*bu + bv*bv)
 *       thr = alpha*m + beta
 *       excess = d - thr                  (+inf where not inside, and where d - thr is NaN: a non-finite sample of b)
 *       valid  = inside and excess <= 0
 *   Direction b is the same arithmetic with the roles swapped.  The border is closed: a zero flow is valid on the whole image; a
 *   clamped tap carries weight 0 and a pixel that is not inside reads nothing of its partner, so nothing outside the two views is
 *   read.  A lane owns four consecutive pixels of a row: two 16-byte loads, one dword of mask bytes and one 16-byte store of excess
 *   where W, all six strides and every pointer allow, single elements otherwise.  No atomics, no workspace, no LDS; every output
 *   element is written once: the result repeats bit for bit, does not depend on the launch geometry, and an image's result does
 *   not depend on the other images of the batch.
 *   1 <= N <= 65535, 1 <= H, W <= 2^24, H * ceil(W / 4) < 2^31 - 256, row stride >= W, plane stride >= (H - 1) * row stride + W,
 *   image stride >= plane stride + (H - 1) * row stride + W, alpha and beta finite and >= 0; 4-byte aligned pointers; the outputs
 *   must not overlap the flows.  DVS_ERR_INVALID, before any launch, otherwise.
 *   dvs_set_precision does not affect this entry.
 * ------------------------------------------------------------------------------------------- */
int dvs_flow_consistency(const float* a, long long a_image_stride, long long a_plane_stride, long long a_row_stride, const float* b,
                         long long b_image_stride, long long b_plane_stride, long long b_row_stride, unsigned char* valid_a,
                         unsigned char* valid_b, float* excess_a, float* excess_b, int N, int H, int W, float alpha, float beta,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 12: new entry points only) Rigid flow from depth and pose, and a moving-object label for a measured flow
 *     the flow a static scene shows under this depth and this camera motion: the reference's BackprojectDepth and Project3D
 *     (vo/learner_func.py:106-159) in pixel coordinates, without the normalise round trip; the residual of a measured flow
 *     against it (GeoNet, Yin and Shi 2018) with the threshold form of dvs_flow_consistency;
 *     replaces two batched matmuls, a divide, a grid and half a dozen elementwise launches per frame
 *
 *   depth: fp32, N images of H x W pixels, d of pixel (n, y, x) at depth[n * depth_image_stride + y * depth_row_stride + x]
 *   (element strides).  K, inv_K, T: fp32 [N][4][4], dense, the reference's conventions; T maps points of the flow's SOURCE
 *   camera (the one depth belongs to) into the target camera.  flow (optional): fp32, u of pixel (n, y, x) at
 *   flow[n * flow_image_stride + y * flow_row_stride + x] and v one flow_plane_stride further, so the un-padded view of a padded
 *   [N][2][Hp][Wp] flow is read in place.  valid (optional, read with a flow only): uint8 [N][H][W], dense, the mask of
 *   dvs_flow_consistency.  rigid: fp32 [N][2][H][W]; excess: fp32 [N][H][W]; label: uint8 [N][H][W]; all dense, each may be NULL
 *   (all three NULL: nothing is launched); excess and label need a flow.  In fp32, every operation rounded on its own (no
 *   contraction), in exactly this order, iK = inv_K:
 *     per image:
 *       P[i][j] = ((K[i][0]*T[0][j] + K[i][1]*T[1][j]) + K[i][2]*T[2][j]) + K[i][3]*T[3][j]          i < 3
 *     per pixel (x, y), d = depth:
 *       rx = (iK[0][0]*x + iK[0][1]*y) + iK[0][2]                ry, rz: rows 1, 2
 *       X = d*rx, Y = d*ry, Z = d*rz
 *       cx = ((P[0][0]*X + P[0][1]*Y) + P[0][2]*Z) + P[0][3]     cy, cz: rows 1, 2
 *       den = cz + eps
 *       px = cx / den, py = cy / den                             (the correctly rounded quotient, not a reciprocal)
 *       ru = px - x, rv = py - y                                 (rigid; a non-finite component is stored as the quiet NaN 0x7FC00000)
 *       inside = cz > 0 and 0 <= px <= W-1 and 0 <= py <= H-1    (closed; false for NaN)
 *     with flow = (fu, fv):
 *       ex = fu - ru, ey = fv - rv, e2 = ex*ex + ey*ey
 *       m   = (fu*fu + fv*fv) + (ru*ru + rv*rv)
 *       thr = alpha*m + beta
 *       excess = e2 - thr                 (+inf where not inside, where valid is given and 0, and where e2 - thr is NaN)
 *       label  = 0 (not judged) where excess is +inf by that rule, 1 (static) where excess <= 0, 2 (moving) otherwise
 *   P is computed by every lane from uniform loads: one launch, no workspace.  A lane owns four consecutive pixels of a row:
 *   16-byte loads of depth and flow, 16-byte stores of rigid and excess and one dword of label bytes where W, every stride and
 *   every pointer allow, single elements otherwise.  No atomics, no LDS; every output element is written once: the result repeats
 *   bit for bit, does not depend on the launch geometry, and an image's result does not depend on the other images of the batch.
 *   1 <= N <= 65535, 1 <= H, W <= 2^24, H * ceil(W / 4) < 2^31 - 256, row strides >= W, depth image stride >= (H - 1) * row stride + W,
 *   flow plane stride >= (H - 1) * row stride + W, flow image stride >= plane stride + (H - 1) * row stride + W, alpha, beta and eps
 *   finite and >= 0; 4-byte aligned fp32 pointers; no output may overlap an input.  DVS_ERR_INVALID, before any launch, otherwise.
 *   Only `stream` is used; dvs_set_precision does not affect this entry.
 * ------------------------------------------------------------------------------------------- */
int dvs_rigid_flow(const float* depth, long long depth_image_stride, long long depth_row_stride, const float* K, const float* inv_K,
                   const float* T, const float* flow, long long flow_image_stride, long long flow_plane_stride, long long flow_row_stride,
                   const unsigned char* valid, float* rigid, float* excess, unsigned char* label, int N, int H, int W, float alpha,
                   float beta, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * (added under ABI 12: new entry points only) Camera pose from a measured flow and the depth of its source frame
 *     the inverse of dvs_rigid_flow: the T under which a static scene of this depth shows this flow.  A dense reprojection-error
 *     Gauss-Newton fit on SE(3) with Huber weights (iteratively re-weighted least squares), the per-pair form of the reference's
 *     CPU back end (slam/optimizer.py:222-319: g2o, EdgeProjectD3VO under RobustKernelHuber)
 *
 *   depth, K, inv_K, flow, valid: as dvs_rigid_flow (depth and flow through their strides, valid dense uint8 or NULL); flow is
 *   required.  T0: fp32 [N][4][4], the initial guess; T: fp32 [N][4][4], the fit (T may be exactly T0: fitted in place).
 *   status: int [N], 0 where every iteration took its step, 1 otherwise.  normal (optional): double [N][30], the sums at the final
 *   T.  workspace: dvs_pose_fit_workspace(N, H, W) bytes, 8-byte aligned, holds nothing between calls.
 *   ACCUMULATE, one launch for all N images.  In fp32, every operation rounded on its own (no contraction), in exactly this order,
 *   iK = inv_K, per pixel (x, y), d = depth, (fu, fv) = flow:
 *       rx = (iK[0][0]*x + iK[0][1]*y) + iK[0][2]                ry, rz: rows 1, 2
 *       X = d*rx, Y = d*ry, Z = d*rz
 *       qx = ((T[0][0]*X + T[0][1]*Y) + T[0][2]*Z) + T[0][3]     qy, qz: rows 1, 2
 *       cx = ((K[0][0]*qx + K[0][1]*qy) + K[0][2]*qz) + K[0][3]  cy, cz: rows 1, 2
 *       den = cz + eps
 *       px = cx / den, py = cy / den                             (the correctly rounded quotient)
 *       tx = x + fu, ty = y + fv                                 (the measured target)
 *       ex = px - tx, ey = py - ty                               (the residual)
 *       judged = d finite and d > 0, fu and fv finite, valid NULL or non-zero, cz > 0, 0 <= tx <= W-1, 0 <= ty <= H-1 (closed),
 *                ex and ey finite
 *       e2 = ex*ex + ey*ey
 *       w  = 1 if e2 <= huber*huber, else huber / sqrt(e2)       (sqrt and quotient correctly rounded; huber = +inf: w = 1)
 *       A[r][k] = (K[r][k] - p_r*K[2][k]) / den                  r = 0, 1 with p_0 = px, p_1 = py;  k = 0, 1, 2
 *       J[r] = (A[r][0], A[r][1], A[r][2], A[r][2]*qy - A[r][1]*qz, A[r][0]*qz - A[r][2]*qx, A[r][1]*qx - A[r][0]*qy)
 *     J is the derivative of (px, py) for a left perturbation T <- exp(xi) T, xi = (nu, omega), translation first.  Every judged
 *     pixel gives one fp32 term to each of 30 sums; the term is widened and ADDED IN fp64:
 *       sum[idx(i, j)] += w * (J[0][i]*J[0][j] + J[1][i]*J[1][j])    0 <= i <= j < 6; idx counts the upper triangle row by row: 0 .. 20
 *       sum[21 + i]    += w * (J[0][i]*ex + J[1][i]*ey)              i < 6
 *       sum[27] += w * e2,  sum[28] += w,  sum[29] += 1              (the cost, the weights, the judged count)
 *     A lane owns four consecutive pixels of a row (16-byte loads where W, every stride and every pointer allow, single elements
 *     otherwise) and walks the image with a grid stride; the workgroups per image depend on (H, W) alone.  A 64-lane butterfly,
 *     the four waves through LDS, one row of 30 doubles per workgroup into the workspace.  No atomics, no memset: the sums repeat
 *     bit for bit, in both load forms, and an image's sums do not depend on the other images of the batch.
 *   UPDATE, one launch, one workgroup per image, fp64 (no contraction): the rows are staged in LDS and added in row order, H and g are sums 0 .. 20 and
 *   21 .. 26,
 *       A = H + damping * diag(H);  A = L L^T (Cholesky);  L y = -g;  L^T xi = y
 *       theta2 = (wx*wx + wy*wy) + wz*wz with omega = (wx, wy, wz), W = [omega]x
 *       theta2 <  1e-4: a = (1 - theta2/6) + theta2^2/120, b = (1/2 - theta2/24) + theta2^2/720, c = (1/6 - theta2/120) + theta2^2/5040
 *       otherwise:      a = sin(theta)/theta, b = (1 - cos(theta))/theta2, c = (theta - sin(theta))/(theta2*theta)
 *       R = (I + a W) + b W^2,  V = (I + b W) + c W^2,  t = V nu;  T <- [R t; 0 1] T, rounded to fp32
 *     The step is SKIPPED for an image -- T keeps its bits for this and every later iteration of the call, status = 1 -- when
 *     fewer than 6 pixels were judged, a sum, xi or the new T is not finite, or a pivot of the Cholesky is not positive.
 *   The entry issues `iters` (accumulate, update) pairs; with `normal` one more accumulate at the final T, whose ordered sums are
 *   stored there (iters = 0: the sums at T0; T = T0, status = 0).
 *   N, H, W, strides and alignment as dvs_rigid_flow; 0 <= iters <= 64; huber > 0 (+inf allowed, NaN not); damping and eps finite
 *   and >= 0; workspace_bytes >= dvs_pose_fit_workspace (0 for a shape the entry refuses); T and status 4-byte, normal and workspace
 *   8-byte aligned; no output may overlap an input or another output, except T == T0.  DVS_ERR_INVALID, before any launch, otherwise.
 *   Only `stream` is used; dvs_set_precision does not affect this entry.
 * ------------------------------------------------------------------------------------------- */
size_t dvs_pose_fit_workspace(int N, int H, int W);
int dvs_pose_fit(const float* depth, long long depth_image_stride, long long depth_row_stride, const float* K, const float* inv_K,
                 const float* T0, const float* flow, long long flow_image_stride, long long flow_plane_stride, long long flow_row_stride,
                 const unsigned char* valid, float* T, int* status, double* normal, void* workspace, size_t workspace_bytes, int N, int H,
                 int W, int iters, float huber, float damping, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_H */
