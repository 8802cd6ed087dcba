// Shift-stack gather and its adjoint: the five taps of a (1,5) / (5,1) convolution laid side by side along the channels.
//
// SepConvGRU (model/raft/core/update.py:33-60) convolves with (1,5) filters, padding (0,2), then with (5,1), padding (2,0).  Over
// NHWC memory such a convolution is a 1x1 convolution of
//     X5[n][y][x][t*C + c] = x[n][y + dy*(t-2)][x + dx*(t-2)][c]   (0 outside the map),   t = 0 .. 4,
// with (dy, dx) = (0, 1) for axis 0 (the W taps of a (1,5) filter) and (1, 0) for axis 1 (the H taps of a (5,1) filter), and the
// filter W[Cout][Cin][1][5] re-laid as [Cout][5*Cin] (raft_update.py).  The contraction then runs on the 1x1 route of the existing
// convolution kernels; this file only moves data.
//
//   forward   one lane owns four consecutive channels of one tap of one pixel: a 16-byte load (or zeros) and a 16-byte store;
//             consecutive lanes write consecutive 16 bytes of X5.
//   adjoint   dx[n][y][x][c] = sum_t dX5[n][y - dy*(t-2)][x - dx*(t-2)][t*C + c] over the in-range sources, in ascending t: one
//             lane owns four channels of one pixel and adds at most five 16-byte loads.
//
// Every output element has one owner and no atomics: two runs agree bit for bit.  Element offsets are 64-bit; the grid covers the
// items 256 per workgroup and strides where that exceeds the 2^31 - 1 workgroups of a launch.  Extents smaller than the window
// (H or W of 1 or 2) need no special case: every tap is tested against the map on its own.
#include "common.h"

#include <cstdint>

namespace {

constexpr int kThreads = 256;
constexpr int kTaps = 5;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

struct Shape {
    size_t pixels;      // N * H * W
    unsigned H, W, C, q;    // q = C / 4
    int dy, dx;
};

// pixel index -> (row, column) inside its image; the image index is not needed: a shift that stays inside [0,H) x [0,W) stays
// inside the image, and moves the pixel index by dy * W + dx
__device__ __forceinline__ void row_col(const Shape& s, size_t p, int& y, int& x) {
    const size_t row = p / s.W;
    x = (int)(p - row * s.W);
    y = (int)(row % s.H);
}

__global__ void __launch_bounds__(kThreads) shift_stack_fwd_kernel(Shape s, const float* __restrict__ in, float* __restrict__ x5) {
    const size_t items = s.pixels * kTaps * s.q, step = (size_t)gridDim.x * kThreads;
    const unsigned per_pixel = kTaps * s.q;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < items; i += step) {
        const size_t p = i / per_pixel;
        const unsigned rem = (unsigned)(i - p * per_pixel);
        const int t = (int)(rem / s.q) - 2;
        const unsigned c = (rem % s.q) * 4u;
        int y, x;
        row_col(s, p, y, x);
        const int ys = y + s.dy * t, xs = x + s.dx * t;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ys >= 0 && ys < (int)s.H && xs >= 0 && xs < (int)s.W) {
            const size_t src = (size_t)((long long)p + (long long)s.dy * t * (long long)s.W + (long long)s.dx * t);
            v = ld4(in + src * s.C + c);
        }
        st4(x5 + i * 4, v);                                 // item i IS float4 number i of X5 [pixels][5][C/4]
    }
}

__global__ void __launch_bounds__(kThreads) shift_stack_bwd_kernel(Shape s, const float* __restrict__ dx5, float* __restrict__ dx) {
    const size_t items = s.pixels * s.q, step = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < items; i += step) {
        const size_t p = i / s.q;
        const unsigned c = (unsigned)(i - p * s.q) * 4u;
        int y, x;
        row_col(s, p, y, x);
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const int t = k - 2;
            const int ys = y - s.dy * t, xs = x - s.dx * t;        // the pixel whose tap k read this one
            if (ys < 0 || ys >= (int)s.H || xs < 0 || xs >= (int)s.W) continue;
            const size_t src = (size_t)((long long)p - (long long)s.dy * t * (long long)s.W - (long long)s.dx * t);
            const float4 g = ld4(dx5 + (src * kTaps + k) * s.C + c);
            acc.x += g.x;
            acc.y += g.y;
            acc.z += g.z;
            acc.w += g.w;
        }
        st4(dx + i * 4, acc);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int make_shape(const char* who, int N, int H, int W, int C, int axis, Shape* s) {
    DVS_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: N=%d, H=%d, W=%d must be positive", who, N, H, W);
    DVS_REQUIRE(C > 0 && C % 4 == 0, "%s: C=%d must be a positive multiple of 4 (16-byte channel groups)", who, C);
    DVS_REQUIRE(axis == 0 || axis == 1, "%s: axis=%d must be 0 (taps along W, a (1,5) filter) or 1 (taps along H, a (5,1) filter)",
                who, axis);
    const size_t pixels = (size_t)N * (size_t)H * (size_t)W;              // < 2^93 cannot happen: three ints
    DVS_REQUIRE(pixels <= (SIZE_MAX / 32) / (size_t)C, "%s: %zu pixels of 5*%d floats overflow a 64-bit byte offset", who, pixels, C);
    s->pixels = pixels;
    s->H = (unsigned)H;
    s->W = (unsigned)W;
    s->C = (unsigned)C;
    s->q = (unsigned)C / 4;
    s->dy = axis == 1 ? 1 : 0;
    s->dx = axis == 0 ? 1 : 0;
    return DVS_OK;
}

unsigned grid_of(size_t items) {
    const size_t blocks = (items + kThreads - 1) / kThreads;
    return (unsigned)(blocks < 0x7fffffffull ? blocks : 0x7fffffffull);    // beyond that the kernels stride
}

}  // namespace

extern "C" {

int dvs_shift_stack_fwd(const float* x, float* x5, int N, int H, int W, int C, int axis, void* stream) {
    DVS_REQUIRE(x && x5, "dvs_shift_stack_fwd: null pointer");
    DVS_REQUIRE(aligned16(x) && aligned16(x5), "dvs_shift_stack_fwd: misaligned pointer");
    Shape s;
    if (int rc = make_shape("dvs_shift_stack_fwd", N, H, W, C, axis, &s)) return rc;
    hipLaunchKernelGGL(shift_stack_fwd_kernel, dim3(grid_of(s.pixels * kTaps * s.q)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), s, x, x5);
    return dvs::check_launch("dvs_shift_stack_fwd");
}

int dvs_shift_stack_bwd(const float* dx5, float* dx, int N, int H, int W, int C, int axis, void* stream) {
    DVS_REQUIRE(dx5 && dx, "dvs_shift_stack_bwd: null pointer");
    DVS_REQUIRE(aligned16(dx5) && aligned16(dx), "dvs_shift_stack_bwd: misaligned pointer");
    Shape s;
    if (int rc = make_shape("dvs_shift_stack_bwd", N, H, W, C, axis, &s)) return rc;
    hipLaunchKernelGGL(shift_stack_bwd_kernel, dim3(grid_of(s.pixels * s.q)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       s, dx5, dx);
    return dvs::check_launch("dvs_shift_stack_bwd");
}

}  // extern "C"
