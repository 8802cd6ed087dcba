// Convex 8x upsampling of a flow field (RAFT.upsample_flow, model/raft/core/raft.py:170-181) and its gradients, in one pass over
// the mask each way.
//
//   flow [N][2][h][w] planar (coords1 - coords0), mask [N][h][w][576] NHWC (what the 1x1 mask convolution writes), channel
//   c = k*64 + i*8 + j with tap k = ky*3 + kx, sub-row i, sub-column j;  out [N][2][8h][8w] planar.
//       p_k              = softmax_k(mask_scale * mask[n][y][x][k*64 + i*8 + j])        (the maximum subtracted first)
//       out[n][ch][8y+i][8x+j] = sum_k p_k * 8 * flow[n][ch][y+ky-1][x+kx-1]            (0 outside the map: F.unfold(padding=1))
//
// The reference walks the mask with view -> softmax -> unfold -> mul -> sum -> permute -> reshape, about ten passes over mask-sized
// tensors forward and backward; here the mask is read once per direction and `0.25 *` (update.py:135) is mask_scale, applied on load.
//
// Forward.  A wave is the 8x8 block of one low-resolution pixel, lane = i*8 + j, so each of the nine taps is one contiguous
// 256-byte read.  A workgroup is four waves = four adjacent x.  A wave's 64 results are eight 32-byte pieces of eight different
// output rows, so the stores go through LDS: the four waves put their blocks side by side into a [2][8][32] tile (rows padded to 40
// floats: bank-conflict free both ways) and after one barrier each wave stores two whole 128-byte row segments per channel.
//
// Arithmetic.  expf of the HIP math library on fp32 inputs; the nine weights are summed, normalised and applied in fp64 registers
// and the result is rounded to fp32 once.  Measured: the backward, which has the most fp64 work, runs within
// 20 % of a copy of its bytes, so this is not what bounds the kernels (36 bytes in, 8 out per lane).  It makes two
// properties exact instead of likely: a one-hot softmax returns 8 * flow of its tap bit for bit, and a constant flow comes back as
// that constant (sum_k p_k = 1 to 1e-16, not to nine fp32 roundings).
//
// Backward.  The softmax is recomputed from the mask (the only saved tensor).  With t_k = sum_ch dout_ch * 8 * flow_ch(tap k):
//       dmask[k] = mask_scale * p_k * (t_k - sum_k' p_k' t_k')
//   and the gradient of flow without atomics, in two kernels:
//       s[n][y][x][k][ch] = sum_ij p_k * dout_ch            one wave per pixel, 64-lane DPP reduction, written to the workspace
//       dflow[n][ch][y'][x'] = 8 * sum_k s[n][y'-ky+1][x'-kx+1][k][ch]   a gather over the in-range neighbours, ascending k
//   dout is read as eight 32-byte pieces per wave; the four waves of a workgroup are adjacent in x, so the pieces of one row are
//   one 128-byte line.  dmask is written 256 contiguous bytes per wave and tap: no LDS in this direction.
//
// Every output element is written once by one thread, no atomics: both directions repeat bit for bit.  64-bit element offsets.
#include "common.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int kTaps = 9;
constexpr int kSub = 64;                    // 8 x 8 sub-pixels: one wave
constexpr int kMaskC = kTaps * kSub;        // 576
constexpr int kPix = 4;                     // low-resolution pixels (adjacent x) per workgroup
constexpr int kThreads = kPix * kSub;
constexpr int kTileRow = 40;                // floats per LDS tile row: 32 used, padded so that rows i and i + 1 are 8 banks apart
constexpr int kWs = kTaps * 2;              // workspace floats per pixel

struct Shape {
    int N, h, w, bx;    // bx = ceil(w / kPix) workgroups per row
    float scale;
};

// 8 * flow of the nine taps of pixel (y, x), both channels; zeros outside the map
__device__ __forceinline__ void load_taps(const Shape& s, const float* __restrict__ flow, int n, int y, int x, float (&f)[kTaps][2]) {
    const size_t plane = (size_t)s.h * s.w;
    const float* f0 = flow + (size_t)n * 2 * plane;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        const bool in = yy >= 0 && yy < s.h && xx >= 0 && xx < s.w;
        const size_t o = in ? (size_t)yy * s.w + xx : 0;
        f[k][0] = in ? 8.0f * f0[o] : 0.0f;
        f[k][1] = in ? 8.0f * f0[plane + o] : 0.0f;
    }
}

// e_k = exp(v_k - max v) of this lane's nine mask values and r = 1 / sum_k e_k
__device__ __forceinline__ void softmax_parts(const float* __restrict__ m, float scale, float (&e)[kTaps], double& r) {
    float v[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; ++k) v[k] = scale * m[k * kSub];
    float mx = v[0];
#pragma unroll
    for (int k = 1; k < kTaps; ++k) mx = fmaxf(mx, v[k]);
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
        e[k] = expf(v[k] - mx);
        sum += (double)e[k];
    }
    r = 1.0 / sum;                          // sum >= 1: the maximum's own term
}

__global__ void __launch_bounds__(kThreads)
convex_up_fwd_kernel(Shape s, const float* __restrict__ flow, const float* __restrict__ mask, float* __restrict__ out) {
    __shared__ float tile[2][8][kTileRow];
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int n = blockIdx.y, y = (int)(blockIdx.x / (unsigned)s.bx), x0 = (int)(blockIdx.x % (unsigned)s.bx) * kPix;
    const int x = x0 + wv;
    if (x < s.w) {
        float f[kTaps][2], e[kTaps];
        double r;
        load_taps(s, flow, n, y, x, f);
        softmax_parts(mask + (((size_t)n * s.h + y) * s.w + x) * kMaskC + lane, s.scale, e, r);
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            a0 += (double)e[k] * (double)f[k][0];
            a1 += (double)e[k] * (double)f[k][1];
        }
        tile[0][lane >> 3][wv * 8 + (lane & 7)] = (float)(a0 * r);
        tile[1][lane >> 3][wv * 8 + (lane & 7)] = (float)(a1 * r);
    }
    __syncthreads();
    const int row = threadIdx.x >> 5, col = threadIdx.x & 31;
    const int X = x0 * 8 + col, W8 = 8 * s.w;
    if (X < W8) {                           // columns of pixels past the right edge were never written to the tile
#pragma unroll
        for (int ch = 0; ch < 2; ++ch)
            out[(((size_t)n * 2 + ch) * (8 * (size_t)s.h) + (8 * (size_t)y + row)) * W8 + X] = tile[ch][row][col];
    }
}

__global__ void __launch_bounds__(kThreads)
convex_up_bwd_kernel(Shape s, const float* __restrict__ dout, const float* __restrict__ flow, const float* __restrict__ mask,
                     float* __restrict__ dmask, float* __restrict__ ws) {
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int n = blockIdx.y, y = (int)(blockIdx.x / (unsigned)s.bx), x = (int)(blockIdx.x % (unsigned)s.bx) * kPix + wv;
    if (x >= s.w) return;                   // whole waves leave; there is no barrier below
    float f[kTaps][2], e[kTaps];
    double r;
    load_taps(s, flow, n, y, x, f);
    const size_t pixel = ((size_t)n * s.h + y) * s.w + x;
    softmax_parts(mask + pixel * kMaskC + lane, s.scale, e, r);
    const size_t W8 = 8 * (size_t)s.w;
    const size_t o = ((size_t)n * 2 * (8 * (size_t)s.h) + (8 * (size_t)y + (lane >> 3))) * W8 + 8 * (size_t)x + (lane & 7);
    const float d0 = dout[o], d1 = dout[o + 8 * (size_t)s.h * W8];
    double p[kTaps], t[kTaps], dot = 0.0;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
        p[k] = (double)e[k] * r;
        t[k] = (double)d0 * (double)f[k][0] + (double)d1 * (double)f[k][1];
        dot += p[k] * t[k];
    }
    if (dmask) {                            // (kernel arguments: the same branch in every wave)
        float* dm = dmask + pixel * kMaskC + lane;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) dm[k * kSub] = (float)((double)s.scale * p[k] * (t[k] - dot));
    }
    if (ws) {
        float* w = ws + pixel * kWs;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const float pk = (float)p[k];
            const float s0 = dvs::wave_sum_lane63(pk * d0), s1 = dvs::wave_sum_lane63(pk * d1);
            if (lane == 63) *reinterpret_cast<float2*>(w + 2 * k) = make_float2(s0, s1);
        }
    }
}

__global__ void __launch_bounds__(kThreads) convex_up_dflow_kernel(Shape s, const float* __restrict__ ws, float* __restrict__ dflow) {
    const unsigned hw = (unsigned)s.h * (unsigned)s.w;                 // 64 * h * w < 2^31
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= 2u * hw) return;
    const int n = blockIdx.y, ch = (int)(i / hw);
    const unsigned rem = i - (unsigned)ch * hw;
    const int y = (int)(rem / (unsigned)s.w), x = (int)(rem - (unsigned)y * (unsigned)s.w);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
        const int yy = y - (k / 3) + 1, xx = x - (k % 3) + 1;          // the pixel whose tap k is (y, x)
        if (yy < 0 || yy >= s.h || xx < 0 || xx >= s.w) continue;
        acc += ws[((((size_t)n * s.h + yy) * s.w + xx) * kTaps + k) * 2 + ch];
    }
    dflow[(size_t)n * 2 * hw + i] = 8.0f * acc;
}

int make_shape(const char* who, int N, int h, int w, float scale, Shape* s) {
    DVS_REQUIRE(N >= 1 && N <= 65535, "%s: N=%d maps must be in 1 .. 65535 (one grid row each)", who, N);
    DVS_REQUIRE(h >= 1 && w >= 1, "%s: h=%d, w=%d must be positive", who, h, w);
    DVS_REQUIRE((long long)h * w * 64 < (1ll << 31), "%s: 8h * 8w = %lld output pixels per map exceed 2^31 - 1", who, (long long)h * w * 64);
    DVS_REQUIRE(std::isfinite(scale), "%s: mask_scale must be finite", who);
    s->N = N;
    s->h = h;
    s->w = w;
    s->bx = (w + kPix - 1) / kPix;
    s->scale = scale;
    return DVS_OK;
}

size_t ws_bytes(int N, int h, int w) { return (size_t)N * (size_t)h * (size_t)w * kWs * sizeof(float); }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

size_t dvs_convex_up_workspace(int N, int h, int w) {
    Shape s;
    if (make_shape("dvs_convex_up_workspace", N, h, w, 1.0f, &s)) return 0;
    return ws_bytes(N, h, w);
}

int dvs_convex_up_fwd(const float* flow, const float* mask, float* out, int N, int h, int w, float mask_scale, void* stream) {
    DVS_REQUIRE(flow && mask && out, "dvs_convex_up_fwd: null pointer");
    DVS_REQUIRE(aligned16(flow) && aligned16(mask) && aligned16(out), "dvs_convex_up_fwd: misaligned pointer");
    Shape s;
    if (int rc = make_shape("dvs_convex_up_fwd", N, h, w, mask_scale, &s)) return rc;
    hipLaunchKernelGGL(convex_up_fwd_kernel, dim3((unsigned)s.bx * (unsigned)h, (unsigned)N), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), s, flow, mask, out);
    return dvs::check_launch("dvs_convex_up_fwd");
}

int dvs_convex_up_bwd(const float* dout, const float* flow, const float* mask, float* dflow, float* dmask, void* workspace,
                      size_t workspace_bytes, int N, int h, int w, float mask_scale, void* stream) {
    DVS_REQUIRE(dout && flow && mask, "dvs_convex_up_bwd: null pointer");
    DVS_REQUIRE(dflow || dmask, "dvs_convex_up_bwd: null pointer: dflow and dmask are both NULL, nothing to compute");
    DVS_REQUIRE(!dflow || workspace, "dvs_convex_up_bwd: null pointer: dflow needs the workspace");
    DVS_REQUIRE(aligned16(dout) && aligned16(flow) && aligned16(mask) && aligned16(dflow) && aligned16(dmask) && aligned16(workspace),
                "dvs_convex_up_bwd: misaligned pointer");
    Shape s;
    if (int rc = make_shape("dvs_convex_up_bwd", N, h, w, mask_scale, &s)) return rc;
    DVS_REQUIRE(!dflow || workspace_bytes >= ws_bytes(N, h, w),
                "dvs_convex_up_bwd: workspace of %zu bytes, dvs_convex_up_workspace asks for %zu", workspace_bytes, ws_bytes(N, h, w));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(convex_up_bwd_kernel, dim3((unsigned)s.bx * (unsigned)h, (unsigned)N), dim3(kThreads), 0, st, s, dout, flow, mask,
                       dmask, dflow ? static_cast<float*>(workspace) : nullptr);
    if (int rc = dvs::check_launch("dvs_convex_up_bwd")) return rc;
    if (!dflow) return DVS_OK;
    const unsigned items = 2u * (unsigned)h * (unsigned)w;
    hipLaunchKernelGGL(convex_up_dflow_kernel, dim3((items + kThreads - 1) / kThreads, (unsigned)N), dim3(kThreads), 0, st, s,
                       static_cast<const float*>(workspace), dflow);
    return dvs::check_launch("dvs_convex_up_bwd");
}

}  // extern "C"
