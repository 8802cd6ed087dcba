// Frame ingest: everything between a video decoder's uint8 frame and the first convolution of a RAFT encoder, in one launch.
//
//   dvs_frame_ingest   load_image's .float() and /= 255.0 (model/raft/raft.py:22-23), InputPadder.pad's replicate padding
//                      (model/raft/core/utils/utils.py:7-21), 2 * image - 1.0 (model/raft/core/raft.py:70-71, 188-190) and the
//                      4-channel NHWC form that raft_encoder hands conv1
//
//   dst[n, y, x, c] = 2 * (float(src[n, clamp(y - top, 0, H - 1), clamp(x - left, 0, W - 1), c']) / 255) - 1   c < 3, c' = bgr ? 2 - c : c
//   dst[n, y, x, 3] = 0
//
// The division is the correctly rounded fp32 quotient (the reference divides on the host), 2 * q is exact and the subtraction is
// rounded on its own: contraction is off for the whole file, as in flowstage.hip.  A streaming kernel at the launch floor: a lane
// owns four consecutive output pixels of a row and stores each as one 16-byte float4 (64 contiguous bytes per lane).  Padding is
// the clamp of the source coordinates; there is no branch on the border.  Two forms: VEC reads the lane's 12 source bytes as
// three dwords (the source pointer, both strides, `left` and W are multiples of 4: the clamped window of four source pixels then
// starts on a dword) and picks each output pixel's source out of the registers; the scalar form reads single bytes.  No LDS, no
// atomics, no workspace.
#include "common.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;                             // output pixels per lane: four float4 stores

struct Frame {
    const unsigned char* src;
    long long image_stride, row_stride;             // bytes
    int H, W, Hp, Wp, left, top;
    int quads;                                      // ceil(Wp / kPix): lanes per output row
    int bgr;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ float4 normalised(unsigned rgb, int bgr) {
    // rgb: byte 0 is the first channel in memory
    const float c0 = 2.0f * ((float)(rgb & 255u) / 255.0f) - 1.0f;
    const float c1 = 2.0f * ((float)(rgb >> 8 & 255u) / 255.0f) - 1.0f;
    const float c2 = 2.0f * ((float)(rgb >> 16 & 255u) / 255.0f) - 1.0f;
    return bgr ? make_float4(c2, c1, c0, 0.0f) : make_float4(c0, c1, c2, 0.0f);
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) frame_ingest_kernel(Frame f, float* __restrict__ dst) {
    const unsigned g = blockIdx.x * kThreads + threadIdx.x;           // host: Hp * quads < 2^31
    const unsigned y = g / (unsigned)f.quads;
    if (y >= (unsigned)f.Hp) return;
    const int x0 = (int)(g - y * (unsigned)f.quads) * kPix;
    const int n = blockIdx.y;
    const unsigned char* row = f.src + (size_t)n * (size_t)f.image_stride + (size_t)clampi((int)y - f.top, f.H - 1) * (size_t)f.row_stride;
    unsigned rgb[kPix];
    if (VEC) {                                                        // W % 4 == 0, left % 4 == 0: s is a multiple of 4 in 0 .. W - 4
        const int s = clampi(x0 - f.left, f.W - kPix);
        const uint3 d = *reinterpret_cast<const uint3*>(row + 3 * (size_t)s);      // source pixels s .. s + 3: 12 * (s / 4) bytes in
        const unsigned p0 = d.x & 0xFFFFFFu, p1 = d.x >> 24 | (d.y & 0xFFFFu) << 8, p2 = d.y >> 16 | (d.z & 0xFFu) << 16, p3 = d.z >> 8;
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const int j = clampi(x0 + k - f.left, f.W - 1) - s;       // 0 .. 3 for every pixel that is stored
            rgb[k] = j <= 0 ? p0 : (j == 1 ? p1 : (j == 2 ? p2 : p3));
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const unsigned char* p = row + 3 * (size_t)clampi(x0 + k - f.left, f.W - 1);
            rgb[k] = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
        }
    }
    float4* o = reinterpret_cast<float4*>(dst) + ((size_t)n * (size_t)f.Hp + y) * (size_t)f.Wp + x0;
#pragma unroll
    for (int k = 0; k < kPix; ++k)
        if (x0 + k < f.Wp) o[k] = normalised(rgb[k], f.bgr);          // the row's tail, not the border
}

using dvs::aligned;

}  // namespace

extern "C" {

int dvs_frame_ingest(const unsigned char* src, long long image_stride, long long row_stride, float* dst, int N, int H, int W,
                     int left, int right, int top, int bottom, int bgr, void* stream) {
    DVS_REQUIRE(src && dst, "dvs_frame_ingest: null pointer");
    DVS_REQUIRE(aligned(dst, 16), "dvs_frame_ingest: misaligned pointer (dst is stored as float4)");
    DVS_REQUIRE(N >= 1 && N <= 65535, "dvs_frame_ingest: N=%d frames must be in 1 .. 65535", N);
    DVS_REQUIRE(H >= 1 && W >= 1, "dvs_frame_ingest: H=%d, W=%d must be positive", H, W);
    DVS_REQUIRE(left >= 0 && left <= 7 && right >= 0 && right <= 7 && top >= 0 && top <= 7 && bottom >= 0 && bottom <= 7,
                "dvs_frame_ingest: pads left=%d, right=%d, top=%d, bottom=%d must be in 0 .. 7", left, right, top, bottom);
    DVS_REQUIRE(bgr == 0 || bgr == 1, "dvs_frame_ingest: bgr=%d must be 0 (RGB) or 1 (BGR)", bgr);
    const long long Hp = (long long)top + H + bottom, Wp = (long long)left + W + right;
    DVS_REQUIRE(Hp * ((Wp + kPix - 1) / kPix) < (1ll << 31) - kThreads && Wp < (1ll << 31),
                "dvs_frame_ingest: Hp * Wp = %lld x %lld pixels per frame exceed 2^31 - 1 lanes of four", Hp, Wp);
    DVS_REQUIRE(row_stride >= 3ll * W, "dvs_frame_ingest: row stride %lld is below 3 * W = %lld bytes", row_stride, 3ll * W);
    DVS_REQUIRE(row_stride < (1ll << 40) && image_stride < (1ll << 40), "dvs_frame_ingest: strides %lld, %lld out of range", image_stride,
                row_stride);
    DVS_REQUIRE(image_stride >= (long long)(H - 1) * row_stride + 3ll * W,
                "dvs_frame_ingest: image stride %lld is below (H - 1) * row stride + 3 * W = %lld bytes", image_stride,
                (long long)(H - 1) * row_stride + 3ll * W);
    Frame f;
    f.src = src;
    f.image_stride = image_stride;
    f.row_stride = row_stride;
    f.H = H, f.W = W, f.Hp = (int)Hp, f.Wp = (int)Wp, f.left = left, f.top = top;
    f.quads = (int)((Wp + kPix - 1) / kPix);
    f.bgr = bgr;
    const bool vec = W % 4 == 0 && left % 4 == 0 && row_stride % 4 == 0 && image_stride % 4 == 0 && aligned(src, 4);
    const unsigned lanes = (unsigned)f.Hp * (unsigned)f.quads;
    const dim3 grid((lanes + kThreads - 1) / kThreads, (unsigned)N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(frame_ingest_kernel<true>, grid, dim3(kThreads), 0, st, f, dst);
    else hipLaunchKernelGGL(frame_ingest_kernel<false>, grid, dim3(kThreads), 0, st, f, dst);
    return dvs::check_launch("dvs_frame_ingest");
}

}  // extern "C"
