// Forward-backward consistency of two optical flows: the validity / occlusion mask a consumer needs before it trusts a flow vector.
//
//   dvs_flow_consistency   the criterion of UnFlow (Meister et al. 2018, eq. 2) on a forward and a backward flow, both directions in
//                          one launch; the bilinear gather is bilinear_sampler (model/raft/core/utils/utils.py:57-71) in pixel
//                          coordinates, without its normalise / un-normalise round trip
//
// For pixel (x, y) of image n of direction a (own flow a on image 1's grid, partner flow b on image 2's grid):
//
//   qx = float(x) + a.u(x,y)          qy = float(y) + a.v(x,y)
//   inside = 0 <= qx <= W-1  and  0 <= qy <= H-1                       closed; false for NaN
//   x0 = floor(qx), y0 = floor(qy), wx = qx - x0, wy = qy - y0, x1 = min(x0+1, W-1), y1 = min(y0+1, H-1)
//   s(p) = (p[y0,x0]*(1-wx) + p[y0,x1]*wx)*(1-wy) + (p[y1,x0]*(1-wx) + p[y1,x1]*wx)*wy        p = b.u, b.v  ->  bu, bv
//   sx = a.u + bu, sy = a.v + bv;  d = sx*sx + sy*sy;  m = (a.u*a.u + a.v*a.v) + (bu*bu + bv*bv);  thr = alpha*m + beta
//   excess = d - thr                  +inf where not inside, and where d - thr is NaN (a non-finite sample of b)
//   valid  = inside and excess <= 0
//
// Direction b is the same with the roles swapped.  fp32, every operation rounded on its own: contraction is off for the whole file,
// as in flowstage.hip and ingest.hip.  The border is closed, so a zero flow is valid on the whole image; a clamped tap (x1 = x0 at
// qx = W-1) carries weight 0, and a pixel that is not inside reads nothing of the partner: no address outside the two views is formed.
//
// A streaming kernel at the launch floor: a lane owns four consecutive pixels of a row, the direction rides in blockIdx.z and the
// image in blockIdx.y.  VEC: the lane's own flow is two 16-byte loads, its four mask bytes one dword store and its excess one
// 16-byte store (W, the own flow's strides and every pointer involved are multiples of 4 elements / aligned accordingly); the
// scalar form loads and stores single elements.  The sixteen taps of the partner are scalar gathers in both forms.  No LDS, no
// atomics, no workspace; every output element is written once by the lane that owns it, so the result repeats bit for bit and
// does not depend on the launch geometry.
#include "common.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;                             // pixels per lane: four mask bytes = one dword, four excess values = 16 bytes

struct Field {                                      // one flow, element strides: u of (n, y, x) at p[n * image + y * row + x], v one plane on
    const float* p;
    long long image, plane, row;
};

struct Pair {
    Field flow[2];                                  // [0] = a, [1] = b
    unsigned char* valid[2];                        // dense [N][H][W], may be null
    float* excess[2];                               // dense [N][H][W], may be null
    int H, W;
    int quads;                                      // ceil(W / kPix): lanes per row
    float alpha, beta;
};

// bilinear sample of one plane at (x0 + wx, y0 + wy); every index is inside the view
__device__ __forceinline__ float sample(const float* __restrict__ p, size_t r0, size_t r1, int x0, int x1, float wx, float wy) {
    const float ux = 1.0f - wx, uy = 1.0f - wy;
    const float top = p[r0 + x0] * ux + p[r0 + x1] * wx;
    const float bot = p[r1 + x0] * ux + p[r1 + x1] * wx;
    return top * uy + bot * wy;
}

// excess of the pixel (x, y) whose own flow is (au, av) (valid = excess <= 0); `o` / `other` are the partner's strides / its image n
__device__ __forceinline__ float excess_of(const Field& o, const float* __restrict__ other, int x, int y, int H, int W, float au,
                                           float av, float alpha, float beta) {
    const float qx = (float)x + au, qy = (float)y + av;
    const bool inside = qx >= 0.0f && qx <= (float)(W - 1) && qy >= 0.0f && qy <= (float)(H - 1);
    if (!inside) return INFINITY;
    const float fx = floorf(qx), fy = floorf(qy);
    const int x0 = (int)fx, y0 = (int)fy;                             // 0 .. W - 1, 0 .. H - 1
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    const float wx = qx - fx, wy = qy - fy;
    const size_t r0 = (size_t)y0 * (size_t)o.row, r1 = (size_t)y1 * (size_t)o.row;
    const float bu = sample(other, r0, r1, x0, x1, wx, wy);
    const float bv = sample(other + o.plane, r0, r1, x0, x1, wx, wy);
    const float sx = au + bu, sy = av + bv;
    const float d = sx * sx + sy * sy;
    const float m = (au * au + av * av) + (bu * bu + bv * bv);
    const float thr = alpha * m + beta;
    const float e = d - thr;
    return e != e ? INFINITY : e;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) flow_consistency_kernel(Pair s) {
    const unsigned g = blockIdx.x * kThreads + threadIdx.x;           // host: H * quads < 2^31 - kThreads
    const unsigned y = g / (unsigned)s.quads;
    if (y >= (unsigned)s.H) return;
    const int x = (int)(g - y * (unsigned)s.quads) * kPix;
    const int n = blockIdx.y, dir = blockIdx.z;
    const Field own = s.flow[dir], oth = s.flow[dir ^ 1];
    unsigned char* __restrict__ valid = s.valid[dir];
    float* __restrict__ excess = s.excess[dir];
    const float* mine = own.p + (size_t)n * (size_t)own.image + (size_t)y * (size_t)own.row + x;
    const float* other = oth.p + (size_t)n * (size_t)oth.image;
    float u[kPix], v[kPix];
    if (VEC) {                                                        // W % 4 == 0: the four are in the row, 16-byte aligned
        const float4 a = *reinterpret_cast<const float4*>(mine), b = *reinterpret_cast<const float4*>(mine + own.plane);
        u[0] = a.x, u[1] = a.y, u[2] = a.z, u[3] = a.w;
        v[0] = b.x, v[1] = b.y, v[2] = b.z, v[3] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            u[k] = v[k] = NAN;                                        // past the row: not inside, nothing is read for it
            if (x + k < s.W) u[k] = mine[k], v[k] = mine[own.plane + k];
        }
    }
    float e[kPix];
#pragma unroll
    for (int k = 0; k < kPix; ++k) e[k] = excess_of(oth, other, x + k, (int)y, s.H, s.W, u[k], v[k], s.alpha, s.beta);
    const size_t o = ((size_t)n * (size_t)s.H + y) * (size_t)s.W + x;
    if (VEC) {
        if (valid) {
            unsigned m = 0;
#pragma unroll
            for (int k = 0; k < kPix; ++k) m |= (e[k] <= 0.0f ? 1u : 0u) << (8 * k);
            *reinterpret_cast<unsigned*>(valid + o) = m;
        }
        if (excess) *reinterpret_cast<float4*>(excess + o) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            if (x + k < s.W) {                                        // the row's tail
                if (valid) valid[o + k] = e[k] <= 0.0f ? 1 : 0;
                if (excess) excess[o + k] = e[k];
            }
        }
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int make_field(const char* name, const float* p, long long image, long long plane, long long row, int H, int W, Field* f) {
    DVS_REQUIRE(p, "dvs_flow_consistency: null pointer (%s)", name);
    DVS_REQUIRE(aligned(p, 4), "dvs_flow_consistency: misaligned pointer (%s)", name);
    DVS_REQUIRE(row >= W, "dvs_flow_consistency: %s row stride %lld is below W=%d", name, row, W);
    DVS_REQUIRE(row < (1ll << 40) && plane < (1ll << 40) && image < (1ll << 40), "dvs_flow_consistency: %s strides %lld, %lld, %lld out of range",
                name, image, plane, row);
    const long long extent = (long long)(H - 1) * row + W;
    DVS_REQUIRE(plane >= extent, "dvs_flow_consistency: %s plane stride %lld is below (H - 1) * row stride + W = %lld", name, plane, extent);
    DVS_REQUIRE(image >= plane + extent, "dvs_flow_consistency: %s image stride %lld is below plane stride + (H - 1) * row stride + W = %lld",
                name, image, plane + extent);
    f->p = p;
    f->image = image;
    f->plane = plane;
    f->row = row;
    return DVS_OK;
}

bool vec_field(const Field& f) { return f.row % 4 == 0 && f.plane % 4 == 0 && f.image % 4 == 0 && aligned(f.p, 16); }

}  // namespace

extern "C" {

int dvs_flow_consistency(const float* a, long long a_image_stride, long long a_plane_stride, long long a_row_stride, const float* b,
                         long long b_image_stride, long long b_plane_stride, long long b_row_stride, unsigned char* valid_a,
                         unsigned char* valid_b, float* excess_a, float* excess_b, int N, int H, int W, float alpha, float beta,
                         void* stream) {
    DVS_REQUIRE(N >= 1 && N <= 65535, "dvs_flow_consistency: N=%d images must be in 1 .. 65535", N);
    DVS_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24),
                "dvs_flow_consistency: H=%d, W=%d must be in 1 .. 2^24 (pixel coordinates are exact in fp32)", H, W);
    const long long quads = ((long long)W + kPix - 1) / kPix;
    DVS_REQUIRE((long long)H * quads < (1ll << 31) - kThreads, "dvs_flow_consistency: H * W = %d x %d pixels per image exceed 2^31 - 1 lanes of four",
                H, W);
    Pair s;
    if (int rc = make_field("a", a, a_image_stride, a_plane_stride, a_row_stride, H, W, &s.flow[0])) return rc;
    if (int rc = make_field("b", b, b_image_stride, b_plane_stride, b_row_stride, H, W, &s.flow[1])) return rc;
    DVS_REQUIRE(alpha >= 0.0f && beta >= 0.0f && alpha < INFINITY && beta < INFINITY,
                "dvs_flow_consistency: alpha=%g, beta=%g must be finite and not negative", (double)alpha, (double)beta);
    DVS_REQUIRE(aligned(excess_a, 4) && aligned(excess_b, 4), "dvs_flow_consistency: misaligned pointer (excess)");
    s.valid[0] = valid_a, s.valid[1] = valid_b;
    s.excess[0] = excess_a, s.excess[1] = excess_b;
    s.H = H, s.W = W, s.quads = (int)quads;
    s.alpha = alpha, s.beta = beta;
    if (!valid_a && !valid_b && !excess_a && !excess_b) return DVS_OK;            // nothing to write: no launch
    const bool vec = W % 4 == 0 && vec_field(s.flow[0]) && vec_field(s.flow[1]) && aligned(valid_a, 4) && aligned(valid_b, 4) &&
                     aligned(excess_a, 16) && aligned(excess_b, 16);
    const unsigned lanes = (unsigned)H * (unsigned)quads;
    const dim3 grid((lanes + kThreads - 1) / kThreads, (unsigned)N, 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(flow_consistency_kernel<true>, grid, dim3(kThreads), 0, st, s);
    else hipLaunchKernelGGL(flow_consistency_kernel<false>, grid, dim3(kThreads), 0, st, s);
    return dvs::check_launch("dvs_flow_consistency");
}

}  // extern "C"
