// upflow8 (model/raft/core/utils/utils.py:80-82): 8 * F.interpolate(flow, 8x, mode='bilinear', align_corners=True), and its adjoint.
//
// Input  [N][2][h][w] planar, or [N][h][w][2] (the memory of a channels_last tensor, which is what the flow head writes).
// Output [N][2][8h][8w] planar, what the reference returns.
//
// Index arithmetic is torch's, in fp32 (tap() below): scale = (in - 1) / (out - 1), or 0 when out == 1; src = scale * dst;
// i0 = (int)src; i1 = i0 + (i0 < in - 1); l1 = src - i0; l0 = 1 - l1.  The factor 8 multiplies the finished blend.
//
// Forward: one thread per output pixel and both channels; consecutive threads are consecutive along W, so the stores coalesce.
// Backward: a gather.  One thread per low-resolution element sums the high-resolution gradients whose i0 / i1 name it, with the
// weights tap() gives -- the forward's own function.  The candidate rows (columns) come from exact integer arithmetic on
// (y -+ 1) * (out - 1) / (in - 1), widened by one on either side; membership is then decided by recomputing tap(Y), never by
// inverting the fp32 scale.  Fixed summation order and no atomics: both directions repeat bit for bit.  N is free: the module
// upsamples every iteration's flow in one launch (N = iters * B).
#include "common.h"

#include <cstdint>

namespace {

constexpr int kThreads = 256;

struct Tap {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Tap tap(int dst, int in, float scale) {
    Tap t;
    const float src = scale * (float)dst;
    int i0 = (int)src;
    i0 = i0 < in - 1 ? i0 : in - 1;                        // torch's guard_index_and_lambda: never past the last row
    t.i0 = i0;
    t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
    t.l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f);
    t.l0 = 1.0f - t.l1;
    return t;
}

// weight with which high-resolution index `dst` reads low-resolution index `i`
__device__ __forceinline__ float weight_of(int dst, int i, int in, float scale) {
    const Tap t = tap(dst, in, scale);
    return (t.i0 == i ? t.l0 : 0.0f) + (t.i1 == i ? t.l1 : 0.0f);
}

struct Shape {
    int N, h, w, H, W;
    float sy, sx;
    int nchw;           // low-resolution tensor: 1 planar [N][2][h][w], 0 [N][h][w][2]
};

__device__ __forceinline__ size_t low_index(const Shape& s, int n, int c, int y, int x) {
    return s.nchw ? (((size_t)n * 2 + c) * s.h + y) * s.w + x : (((size_t)n * s.h + y) * s.w + x) * 2 + c;
}

__global__ void __launch_bounds__(kThreads) upflow8_fwd_kernel(Shape s, const float* __restrict__ flow, float* __restrict__ out) {
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;           // H * W < 2^31
    if (i >= (unsigned)s.H * (unsigned)s.W) return;
    const int n = blockIdx.y, Y = (int)(i / (unsigned)s.W), X = (int)(i - (unsigned)Y * (unsigned)s.W);
    const Tap ty = tap(Y, s.h, s.sy), tx = tap(X, s.w, s.sx);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float v00 = flow[low_index(s, n, c, ty.i0, tx.i0)], v01 = flow[low_index(s, n, c, ty.i0, tx.i1)];
        const float v10 = flow[low_index(s, n, c, ty.i1, tx.i0)], v11 = flow[low_index(s, n, c, ty.i1, tx.i1)];
        const float v = ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
        out[((size_t)n * 2 + c) * s.H * s.W + i] = 8.0f * v;
    }
}

// candidate high-resolution indices of low-resolution index i: [lo, hi], every dst with i0(dst) or i1(dst) == i lies inside
__device__ __forceinline__ void candidates(int i, int in, int out, int& lo, int& hi) {
    if (in == 1) {
        lo = 0;
        hi = out - 1;
        return;
    }
    const long long r = out - 1, q = in - 1;
    long long a = ((long long)(i - 1) * r) / q - 1;                   // src(dst) > i - 1  <=>  dst > (i - 1) * r / q
    long long b = ((long long)(i + 1) * r + q - 1) / q + 1;           // src(dst) < i + 1  <=>  dst < (i + 1) * r / q
    lo = (int)(a < 0 ? 0 : a);
    hi = (int)(b > out - 1 ? out - 1 : b);
}

__global__ void __launch_bounds__(kThreads) upflow8_bwd_kernel(Shape s, const float* __restrict__ dout, float* __restrict__ dflow) {
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;           // 2 * h * w < 2^31
    const unsigned hw = (unsigned)s.h * (unsigned)s.w;
    if (i >= 2u * hw) return;
    const int n = blockIdx.y, c = (int)(i / hw);
    const unsigned rem = i - (unsigned)c * hw;
    const int y = (int)(rem / (unsigned)s.w), x = (int)(rem - (unsigned)y * (unsigned)s.w);
    int y_lo, y_hi, x_lo, x_hi;
    candidates(y, s.h, s.H, y_lo, y_hi);
    candidates(x, s.w, s.W, x_lo, x_hi);
    const float* g = dout + ((size_t)n * 2 + c) * s.H * s.W;
    float acc = 0.0f;
    for (int Y = y_lo; Y <= y_hi; ++Y) {
        const float wy = weight_of(Y, y, s.h, s.sy);
        if (wy == 0.0f) continue;
        const float* row = g + (size_t)Y * s.W;
        float r = 0.0f;
        for (int X = x_lo; X <= x_hi; ++X) r = fmaf(weight_of(X, x, s.w, s.sx), row[X], r);
        acc = fmaf(wy, r, acc);
    }
    dflow[low_index(s, n, c, y, x)] = 8.0f * acc;
}

int make_shape(const char* who, int N, int h, int w, int nchw, Shape* s) {
    DVS_REQUIRE(N >= 1 && N <= 65535, "%s: N=%d maps must be in 1 .. 65535 (one grid row each)", who, N);
    DVS_REQUIRE(h >= 1 && w >= 1, "%s: h=%d, w=%d must be positive", who, h, w);
    DVS_REQUIRE(h <= (1 << 24) / 8 && w <= (1 << 24) / 8, "%s: h=%d, w=%d: 8h and 8w must stay exact in fp32 (<= 2^24)", who, h, w);
    DVS_REQUIRE((long long)h * w * 64 < (1ll << 31), "%s: 8h * 8w = %lld output pixels per map exceed 2^31 - 1", who, (long long)h * w * 64);
    DVS_REQUIRE(nchw == 0 || nchw == 1, "%s: layout flag %d must be 0 ([N][h][w][2]) or 1 ([N][2][h][w])", who, nchw);
    s->N = N;
    s->h = h;
    s->w = w;
    s->H = 8 * h;
    s->W = 8 * w;
    s->sy = (float)(h - 1) / (float)(s->H - 1);            // H, W >= 8: the out == 1 case of torch's rule cannot occur
    s->sx = (float)(w - 1) / (float)(s->W - 1);
    s->nchw = nchw;
    return DVS_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int dvs_upflow8_fwd(const float* flow, float* out, int N, int h, int w, int flow_nchw, void* stream) {
    DVS_REQUIRE(flow && out, "dvs_upflow8_fwd: null pointer");
    DVS_REQUIRE(aligned16(flow) && aligned16(out), "dvs_upflow8_fwd: misaligned pointer");
    Shape s;
    if (int rc = make_shape("dvs_upflow8_fwd", N, h, w, flow_nchw, &s)) return rc;
    const unsigned items = (unsigned)s.H * (unsigned)s.W;
    hipLaunchKernelGGL(upflow8_fwd_kernel, dim3((items + kThreads - 1) / kThreads, (unsigned)N), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), s, flow, out);
    return dvs::check_launch("dvs_upflow8_fwd");
}

int dvs_upflow8_bwd(const float* dout, float* dflow, int N, int h, int w, int dflow_nchw, void* stream) {
    DVS_REQUIRE(dout && dflow, "dvs_upflow8_bwd: null pointer");
    DVS_REQUIRE(aligned16(dout) && aligned16(dflow), "dvs_upflow8_bwd: misaligned pointer");
    Shape s;
    if (int rc = make_shape("dvs_upflow8_bwd", N, h, w, dflow_nchw, &s)) return rc;
    const unsigned items = 2u * (unsigned)h * (unsigned)w;
    hipLaunchKernelGGL(upflow8_bwd_kernel, dim3((items + kThreads - 1) / kThreads, (unsigned)N), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), s, dout, dflow);
    return dvs::check_launch("dvs_upflow8_bwd");
}

}  // extern "C"
