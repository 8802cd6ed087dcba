// The stage after a RAFT forward on video: the warm start of the next pair and the flow colouring of the demo.
//
//   dvs_forward_interp  forward_interpolate, model/raft/core/utils/utils.py:26-54 (two scipy griddata(method='nearest') calls)
//   dvs_flow_radmax     the np.max(rad) of flow_to_image, model/raft/core/utils/flow_viz.py:123-128
//   dvs_flow_to_image   the rest of flow_to_image and flow_uv_to_colors, flow_viz.py:70-106 and 129-132
//
// Every expression below is rounded operation by operation, as NumPy rounds it: contraction is off for the whole file.
//
// forward_interp.  Source j = (yj, xj) of image n lands at (xj + dx, yj + dy), in fp64 (int64 grid + fp32 flow); it is valid iff
// 0 < x1 < w and 0 < y1 < h, strictly.  Grid pixel i takes the flow of the valid source with the smallest squared distance, and
// of the LOWEST row-major index among equals (the reference's KD-tree defines no answer at an exact tie; this is the package's).
// No valid source: zeros (the reference has no answer there: NaN from griddata on zero points).  A brute-force search: a workgroup owns kTargets = 64 grid
// pixels, one per lane; its kWaves = 16 waves share every tile of kSources = 1024 staged sources (x1, y1 as fp64 in LDS, NaN for
// an invalid one: a NaN distance never wins a comparison), wave v taking sources 64v .. 64v + 63 of each tile with broadcast LDS
// reads.  Each lane keeps (d2, index); the sixteen partial answers are merged in LDS by the lexicographic rule, so neither the
// split nor the tile sizes can change the result.  At 60x80 that is 75 workgroups of 16 waves.
//
// flow_to_image.  The flow is addressed through element strides (image stride = 2 * plane_stride), so the un-padded view of a
// padded flow is coloured in place.  radmax: a zero-fill launch (a kernel: see radmax_zero_kernel), then per workgroup a shuffle / LDS maximum and one INTEGER
// atomicMax on the bit pattern of the non-negative fp32 radius (ordered like the values; a NaN sorts above +inf and wins, as in
// np.max); a maximum is exact in any order, so the launch geometry cannot change it.  Colouring: a lane owns four consecutive
// pixels of the dense [N][H][W][3] output = 12 bytes = three aligned dwords, stored as one dwordx3; the reads are two float4
// when W, both strides and the pointer allow, scalar otherwise.  fp32 up to fk, fp64 from floor(fk) on, as the reference's dtype
// ladder under NumPy >= 2 runs it; atan2f is the HIP math library's.  The 55 x 3 wheel is rebuilt per workgroup in LDS from the six
// segment lengths, as wheel / 255.0 in fp64.
#include "common.h"

#include <climits>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

// ---- forward_interp ---------------------------------------------------------------------------------------------------------
constexpr int kTargets = 64;                        // grid pixels per workgroup: one per lane
constexpr int kWaves = 16;                          // waves per workgroup: each takes 64 sources of a tile
constexpr int kSources = kTargets * kWaves;         // 1024 sources staged per tile = threads per workgroup
constexpr long long kMaxPoints = 65536;

__global__ void __launch_bounds__(kSources) forward_interp_kernel(const float* __restrict__ flow, float* __restrict__ out, int h,
                                                                  int w) {
    __shared__ double2 src[kSources];
    __shared__ double part_d2[kWaves][kTargets];
    __shared__ int part_idx[kWaves][kTargets];
    const int P = h * w, n = blockIdx.y;
    const float* fx = flow + (size_t)n * 2 * P;
    const float* fy = fx + P;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * kTargets + lane;                       // >= P in the last workgroup's tail: computed, never stored
    const double tx = (double)(i % w), ty = (double)(i / w);
    double best = INFINITY;
    int best_j = INT_MAX;
    for (int sb = 0; sb < P; sb += kSources) {
        const int j = sb + (int)threadIdx.x;
        double2 s = {NAN, NAN};
        if (j < P) {
            const double x1 = (double)(j % w) + (double)fx[j];
            const double y1 = (double)(j / w) + (double)fy[j];
            if (x1 > 0.0 && x1 < (double)w && y1 > 0.0 && y1 < (double)h) s = {x1, y1};
        }
        __syncthreads();                                              // the previous tile has been read by every wave
        src[threadIdx.x] = s;
        __syncthreads();
        const int j0 = sb + wv * kTargets;
        if (j0 < P) {                                                 // wave-uniform
#pragma unroll 8
            for (int k = 0; k < kTargets; ++k) {
                const double2 p = src[wv * kTargets + k];             // one address per wave: a broadcast read
                const double ex = p.x - tx, ey = p.y - ty;
                const double d2 = ex * ex + ey * ey;
                if (d2 < best) {                                      // ascending j inside a lane: strict < keeps the lowest index
                    best = d2;
                    best_j = j0 + k;
                }
            }
        }
    }
    part_d2[wv][lane] = best;
    part_idx[wv][lane] = best_j;
    __syncthreads();
    if (wv != 0 || i >= P) return;
    for (int v = 1; v < kWaves; ++v) {
        const double d2 = part_d2[v][lane];
        const int j = part_idx[v][lane];
        if (d2 < best || (d2 == best && j < best_j)) {
            best = d2;
            best_j = j;
        }
    }
    const bool found = best_j != INT_MAX;
    float* ox = out + (size_t)n * 2 * P;
    ox[i] = found ? fx[best_j] : 0.0f;
    ox[P + i] = found ? fy[best_j] : 0.0f;
}

// ---- flow_to_image ----------------------------------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kPix = 4;                             // pixels per lane: 12 output bytes = three dwords
constexpr int kCols = 55;
constexpr float kPiF = 3.14159274f;                 // np.float32(np.pi)

struct View {
    const float* flow;
    long long plane_stride, row_stride;
    int H, W;
    float clip_flow;                                // < 0: no clipping
};

// Colour wheel entry (k, channel) as an integer 0 .. 255: six segments of lengths 15, 6, 4, 11, 13, 6 (red-yellow, yellow-green,
// green-cyan, cyan-blue, blue-magenta, magenta-red).  An even segment s holds channel s/2 at 255 and ramps the next one up, an
// odd one holds channel (s+1)/2 at 255 and ramps the one before down; the ramp is floor(255 * i / length).
__device__ __forceinline__ int wheel_entry(int k, int ch) {
    const int len[6] = {15, 6, 4, 11, 13, 6};
    int s = 0, i = k;
    while (i >= len[s]) i -= len[s++];
    const int ramp = 255 * i / len[s];
    const int full = ((s + 1) / 2) % 3;
    const int moving = (s & 1) ? (s - 1) / 2 : (s / 2 + 1) % 3;
    if (ch == full) return 255;
    if (ch == moving) return (s & 1) ? 255 - ramp : ramp;
    return 0;
}

__device__ __forceinline__ float clipped(float x, float hi) {
    if (hi < 0.0f) return x;
    x = x < 0.0f ? 0.0f : x;                                          // np.clip(x, 0, hi): a NaN stays a NaN
    return x > hi ? hi : x;
}

__device__ __forceinline__ float radius(float u, float v) { return sqrtf(u * u + v * v); }

// u, v of kPix consecutive pixels of image n, starting at pixel q (row-major in H x W) of that image; the caller keeps q + k < H * W
// for k < count.  VEC: q % 4 == 0 and W % 4 == 0 put the four in one row at a 16-byte aligned address.
template <bool VEC>
__device__ __forceinline__ void load_pixels(const View& s, int n, unsigned q, int count, float* u, float* v) {
    const float* base = s.flow + (size_t)n * 2 * (size_t)s.plane_stride;
    int y = (int)(q / (unsigned)s.W), x = (int)(q - (unsigned)y * (unsigned)s.W);
    if (VEC) {
        const float* p = base + (size_t)y * (size_t)s.row_stride + x;
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + s.plane_stride);
        u[0] = a.x, u[1] = a.y, u[2] = a.z, u[3] = a.w;
        v[0] = b.x, v[1] = b.y, v[2] = b.z, v[3] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            u[k] = v[k] = 0.0f;
            if (k < count) {
                const float* p = base + (size_t)y * (size_t)s.row_stride + x;
                u[k] = p[0];
                v[k] = p[s.plane_stride];
            }
            if (++x == s.W) x = 0, ++y;
        }
    }
#pragma unroll
    for (int k = 0; k < kPix; ++k) u[k] = clipped(u[k], s.clip_flow), v[k] = clipped(v[k], s.clip_flow);
}

// Zero fill of radmax.  A kernel, not hipMemsetAsync: inside a captured HIP graph a memset node is not reliably ordered before
// the kernel node that accumulates into the buffer once a second graph has been captured (conv_fwd.hip: splitk_zero_kernel);
// a replay then takes the maximum over this and an earlier frame.  Kernel -> kernel edges are ordered.
__global__ void __launch_bounds__(kThreads) radmax_zero_kernel(unsigned* __restrict__ radmax, int N) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n < N) radmax[n] = 0u;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) flow_radmax_kernel(View s, unsigned* __restrict__ radmax) {
    __shared__ unsigned wave_max[kThreads / 64];
    const unsigned HW = (unsigned)s.H * (unsigned)s.W;
    const unsigned q = (blockIdx.x * kThreads + threadIdx.x) * kPix;  // host: H * W < 2^31
    const int n = blockIdx.y;
    unsigned m = 0;                                                   // +0.0f: every radius is >= it
    if (q < HW) {
        const int count = HW - q < (unsigned)kPix ? (int)(HW - q) : kPix;
        float u[kPix], v[kPix];
        load_pixels<VEC>(s, n, q, count, u, v);
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            const unsigned r = __float_as_uint(radius(u[k], v[k]));   // pixels past `count` are (0, 0): radius +0
            m = r > m ? r : m;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)m, o, 64);
        m = other > m ? other : m;
    }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kThreads / 64; ++k) m = wave_max[k] > m ? wave_max[k] : m;
        atomicMax(radmax + n, m);
    }
}

__device__ __forceinline__ unsigned shade(float u, float v, float den, const double* wheel, int bgr) {
    u = u / den;
    v = v / den;
    const float rad = radius(u, v);
    const float a = atan2f(-v, -u) / kPiF;
    const float fk = (a + 1.0f) / 2.0f * (float)(kCols - 1);
    const float fl = floorf(fk);
    int k0 = (int)fl;
    k0 = k0 < 0 ? 0 : (k0 > kCols - 1 ? kCols - 1 : k0);             // 0 .. 54 for every finite flow; the clamp is for the others
    const int k1 = k0 + 1 == kCols ? 0 : k0 + 1;
    const double f = (double)fk - (double)fl;
    unsigned rgb = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double col = (1.0 - f) * wheel[k0 * 3 + c] + f * wheel[k1 * 3 + c];
        col = rad <= 1.0f ? 1.0 - (double)rad * (1.0 - col) : col * 0.75;
        int byte = (int)floor(255.0 * col);
        byte = byte < 0 ? 0 : (byte > 255 ? 255 : byte);
        rgb |= (unsigned)byte << (8 * (bgr ? 2 - c : c));
    }
    return rgb;                                                       // byte 0 is the first channel in memory
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) flow_to_image_kernel(View s, const float* __restrict__ radmax,
                                                                 unsigned char* __restrict__ out, unsigned total, int bgr) {
    __shared__ double wheel[kCols * 3];
    if (threadIdx.x < kCols * 3) wheel[threadIdx.x] = (double)wheel_entry(threadIdx.x / 3, threadIdx.x % 3) / 255.0;
    __syncthreads();
    const unsigned HW = (unsigned)s.H * (unsigned)s.W;
    const unsigned g = (blockIdx.x * kThreads + threadIdx.x) * kPix;  // first of this lane's pixels among all N * H * W (< 2^31)
    if (g >= total) return;
    const int count = total - g < (unsigned)kPix ? (int)(total - g) : kPix;
    unsigned rgb[kPix];
    int n = (int)(g / HW);
    unsigned q = g - (unsigned)n * HW;
    if (VEC) {                                                        // H * W % 4 == 0: the four share an image and a row
        float u[kPix], v[kPix];
        load_pixels<true>(s, n, q, kPix, u, v);
        const float den = radmax[n] + 1e-5f;
#pragma unroll
        for (int k = 0; k < kPix; ++k) rgb[k] = shade(u[k], v[k], den, wheel, bgr);
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            rgb[k] = 0;
            if (k < count) {
                float u[kPix], v[kPix];
                load_pixels<false>(s, n, q, 1, u, v);
                rgb[k] = shade(u[0], v[0], radmax[n] + 1e-5f, wheel, bgr);
            }
            if (++q == HW) q = 0, ++n;
        }
    }
    unsigned char* o = out + (size_t)g * 3;                           // 12 * (g / 4): dword aligned
    if (count == kPix) {
        uint3 d;
        d.x = rgb[0] | rgb[1] << 24;
        d.y = rgb[1] >> 8 | rgb[2] << 16;
        d.z = rgb[2] >> 16 | rgb[3] << 8;
        *reinterpret_cast<uint3*>(o) = d;
    } else {
        for (int k = 0; k < count; ++k) {
            o[3 * k] = (unsigned char)(rgb[k] & 255);
            o[3 * k + 1] = (unsigned char)(rgb[k] >> 8 & 255);
            o[3 * k + 2] = (unsigned char)(rgb[k] >> 16);
        }
    }
}

using dvs::aligned;

int make_view(const char* who, const float* flow, long long plane_stride, long long row_stride, int N, int H, int W, float clip_flow,
              View* s, bool* vec) {
    DVS_REQUIRE(flow, "%s: null pointer", who);
    DVS_REQUIRE(aligned(flow, 4), "%s: misaligned pointer", who);
    DVS_REQUIRE(N >= 1 && N <= 65535, "%s: N=%d images must be in 1 .. 65535", who, N);
    DVS_REQUIRE(H >= 1 && W >= 1, "%s: H=%d, W=%d must be positive", who, H, W);
    DVS_REQUIRE((long long)N * H * W < (1ll << 31), "%s: N * H * W = %lld pixels exceed 2^31 - 1", who, (long long)N * H * W);
    DVS_REQUIRE(row_stride >= W, "%s: row stride %lld is below W=%d", who, row_stride, W);
    DVS_REQUIRE(row_stride < (1ll << 40) && plane_stride < (1ll << 40), "%s: strides %lld, %lld out of range", who, plane_stride,
                row_stride);
    DVS_REQUIRE(plane_stride >= (long long)(H - 1) * row_stride + W, "%s: plane stride %lld is below (H - 1) * row stride + W = %lld",
                who, plane_stride, (long long)(H - 1) * row_stride + W);
    DVS_REQUIRE(!(clip_flow != clip_flow), "%s: clip_flow is NaN (negative means no clipping)", who);
    s->flow = flow;
    s->plane_stride = plane_stride;
    s->row_stride = row_stride;
    s->H = H;
    s->W = W;
    s->clip_flow = clip_flow;
    *vec = W % 4 == 0 && row_stride % 4 == 0 && plane_stride % 4 == 0 && aligned(flow, 16);
    return DVS_OK;
}

}  // namespace

extern "C" {

int dvs_forward_interp(const float* flow, float* out, int N, int h, int w, void* stream) {
    DVS_REQUIRE(flow && out, "dvs_forward_interp: null pointer");
    DVS_REQUIRE(aligned(flow, 4) && aligned(out, 4), "dvs_forward_interp: misaligned pointer");
    DVS_REQUIRE(flow != out, "dvs_forward_interp: out must not be flow");
    DVS_REQUIRE(N >= 1 && N <= 65535, "dvs_forward_interp: N=%d images must be in 1 .. 65535 (one grid row each)", N);
    DVS_REQUIRE(h >= 1 && w >= 1, "dvs_forward_interp: h=%d, w=%d: P = h * w must be at least 1", h, w);
    DVS_REQUIRE((long long)h * w <= kMaxPoints, "dvs_forward_interp: P = h * w = %lld exceeds %lld (a brute-force search)",
                (long long)h * w, kMaxPoints);
    const unsigned P = (unsigned)h * (unsigned)w;
    hipLaunchKernelGGL(forward_interp_kernel, dim3((P + kTargets - 1) / kTargets, (unsigned)N), dim3(kSources), 0,
                       static_cast<hipStream_t>(stream), flow, out, h, w);
    return dvs::check_launch("dvs_forward_interp");
}

int dvs_flow_radmax(const float* flow, long long plane_stride, long long row_stride, int N, int H, int W, float clip_flow,
                    float* radmax, void* stream) {
    View s;
    bool vec;
    if (int rc = make_view("dvs_flow_radmax", flow, plane_stride, row_stride, N, H, W, clip_flow, &s, &vec)) return rc;
    DVS_REQUIRE(radmax, "dvs_flow_radmax: null pointer");
    DVS_REQUIRE(aligned(radmax, 4), "dvs_flow_radmax: misaligned pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(radmax_zero_kernel, dim3(((unsigned)N + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                       reinterpret_cast<unsigned*>(radmax), N);
    const unsigned per_block = kThreads * kPix, HW = (unsigned)H * (unsigned)W;
    const dim3 grid((HW + per_block - 1) / per_block, (unsigned)N);
    unsigned* bits = reinterpret_cast<unsigned*>(radmax);
    if (vec) hipLaunchKernelGGL(flow_radmax_kernel<true>, grid, dim3(kThreads), 0, st, s, bits);
    else hipLaunchKernelGGL(flow_radmax_kernel<false>, grid, dim3(kThreads), 0, st, s, bits);
    return dvs::check_launch("dvs_flow_radmax");
}

int dvs_flow_to_image(const float* flow, long long plane_stride, long long row_stride, const float* radmax, unsigned char* out, int N,
                      int H, int W, float clip_flow, int bgr, void* stream) {
    View s;
    bool vec;
    if (int rc = make_view("dvs_flow_to_image", flow, plane_stride, row_stride, N, H, W, clip_flow, &s, &vec)) return rc;
    DVS_REQUIRE(radmax && out, "dvs_flow_to_image: null pointer");
    DVS_REQUIRE(aligned(radmax, 4) && aligned(out, 16), "dvs_flow_to_image: misaligned pointer");
    DVS_REQUIRE(bgr == 0 || bgr == 1, "dvs_flow_to_image: bgr=%d must be 0 (RGB) or 1 (BGR)", bgr);
    const unsigned per_block = kThreads * kPix, total = (unsigned)N * (unsigned)H * (unsigned)W;
    const dim3 grid((total + per_block - 1) / per_block);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(flow_to_image_kernel<true>, grid, dim3(kThreads), 0, st, s, radmax, out, total, bgr);
    else hipLaunchKernelGGL(flow_to_image_kernel<false>, grid, dim3(kThreads), 0, st, s, radmax, out, total, bgr);
    return dvs::check_launch("dvs_flow_to_image");
}

}  // extern "C"
