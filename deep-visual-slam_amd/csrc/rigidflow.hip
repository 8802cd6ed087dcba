// Rigid flow from depth and pose, and the residual of a measured flow against it: the flow a STATIC scene would show under this
// depth and this camera motion, and the pixels where a measured flow disagrees with it (moving objects, or wrong depth).
//
//   dvs_rigid_flow   the reference's view synthesis, BackprojectDepth and Project3D (vo/learner_func.py:106-159), in pixel
//                    coordinates without the normalise round trip, and the residual test of GeoNet (Yin and Shi 2018) with the
//                    threshold form of dvs_flow_consistency
//
// Per image n, P = (K T)[:3, :], every lane from uniform loads:
//
//   P[i][j] = ((K[i][0]*T[0][j] + K[i][1]*T[1][j]) + K[i][2]*T[2][j]) + K[i][3]*T[3][j]          i < 3
//
// For pixel (x, y) with d = depth(x, y), iK = inv_K:
//
//   rx = (iK[0][0]*x + iK[0][1]*y) + iK[0][2]                ry, rz: rows 1, 2
//   X = d*rx, Y = d*ry, Z = d*rz
//   cx = ((P[0][0]*X + P[0][1]*Y) + P[0][2]*Z) + P[0][3]     cy, cz: rows 1, 2
//   den = cz + eps;  px = cx / den, py = cy / den            the correctly rounded quotient
//   ru = px - x, rv = py - y                                 rigid; a non-finite component is stored as 0x7FC00000
//   inside = cz > 0 and 0 <= px <= W-1 and 0 <= py <= H-1    closed; false for NaN
//
// and with a measured flow (fu, fv):
//
//   ex = fu - ru, ey = fv - rv;  e2 = ex*ex + ey*ey;  m = (fu*fu + fv*fv) + (ru*ru + rv*rv);  thr = alpha*m + beta
//   excess = e2 - thr                 +inf where not inside, where valid is given and 0, and where e2 - thr is NaN
//   label  = 0 (not judged) where excess is +inf by that rule, 1 (static) where excess <= 0, 2 (moving) otherwise
//
// fp32, every operation rounded on its own: contraction is off for the whole file, as in flowcons.hip.
//
// A streaming kernel in the shape of flowcons.hip: a lane owns four consecutive pixels of a row, the image rides in blockIdx.y.
// VEC: depth and the two flow planes are 16-byte loads, the four valid bytes one dword load, rigid and excess 16-byte stores and
// the four labels one dword store (W, every stride and every pointer involved are multiples of 4 elements / aligned accordingly);
// the scalar form loads and stores single elements.  No LDS, no atomics, no workspace; every output element is written once by
// the lane that owns it, so the result repeats bit for bit and does not depend on the launch geometry or on the batch.
#include "common.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPix = 4;                             // pixels per lane: four label bytes = one dword, four floats = 16 bytes

struct Args {
    const float* depth;                             // d of (n, y, x) at depth[n * d_image + y * d_row + x]
    long long d_image, d_row;
    const float *K, *iK, *T;                        // dense [N][4][4]
    const float* flow;                              // u of (n, y, x) at flow[n * f_image + y * f_row + x], v one plane on; may be null
    long long f_image, f_plane, f_row;
    const unsigned char* valid;                     // dense [N][H][W], may be null
    float* rigid;                                   // dense [N][2][H][W], may be null
    float* excess;                                  // dense [N][H][W], may be null
    unsigned char* label;                           // dense [N][H][W], may be null
    int H, W;
    int quads;                                      // ceil(W / kPix): lanes per row
    float alpha, beta, eps;
};

struct Camera {                                     // one image's P = (K T)[:3, :] and the three rows of inv_K that count
    float P[3][4];
    float iK[3][3];
};

__device__ __forceinline__ Camera camera_of(const Args& s, int n) {
    const float* __restrict__ K = s.K + (size_t)n * 16;
    const float* __restrict__ T = s.T + (size_t)n * 16;
    const float* __restrict__ iK = s.iK + (size_t)n * 16;
    Camera c;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c.P[i][j] = ((K[4 * i] * T[j] + K[4 * i + 1] * T[4 + j]) + K[4 * i + 2] * T[8 + j]) + K[4 * i + 3] * T[12 + j];
#pragma unroll
        for (int j = 0; j < 3; ++j) c.iK[i][j] = iK[4 * i + j];
    }
    return c;
}

// (ru, rv) of the pixel (x, y) at depth d; returns inside
__device__ __forceinline__ bool project(const Camera& c, int xi, int yi, float d, int H, int W, float eps, float* ru, float* rv) {
    const float x = (float)xi, y = (float)yi;
    const float rx = (c.iK[0][0] * x + c.iK[0][1] * y) + c.iK[0][2];
    const float ry = (c.iK[1][0] * x + c.iK[1][1] * y) + c.iK[1][2];
    const float rz = (c.iK[2][0] * x + c.iK[2][1] * y) + c.iK[2][2];
    const float X = d * rx, Y = d * ry, Z = d * rz;
    const float cx = ((c.P[0][0] * X + c.P[0][1] * Y) + c.P[0][2] * Z) + c.P[0][3];
    const float cy = ((c.P[1][0] * X + c.P[1][1] * Y) + c.P[1][2] * Z) + c.P[1][3];
    const float cz = ((c.P[2][0] * X + c.P[2][1] * Y) + c.P[2][2] * Z) + c.P[2][3];
    const float den = cz + eps;
    const float px = cx / den, py = cy / den;
    const float u = px - x, v = py - y;
    const float qnan = __uint_as_float(0x7FC00000u);                  // one bit pattern for every non-finite component
    *ru = __builtin_isfinite(u) ? u : qnan;
    *rv = __builtin_isfinite(v) ? v : qnan;
    return cz > 0.0f && px >= 0.0f && px <= (float)(W - 1) && py >= 0.0f && py <= (float)(H - 1);
}

// excess of a judged pixel (NaN where the flow is not finite: the caller turns it into "not judged")
__device__ __forceinline__ float residual(float fu, float fv, float ru, float rv, float alpha, float beta) {
    const float ex = fu - ru, ey = fv - rv;
    const float e2 = ex * ex + ey * ey;
    const float m = (fu * fu + fv * fv) + (ru * ru + rv * rv);
    const float thr = alpha * m + beta;
    return e2 - thr;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) rigid_flow_kernel(Args s) {
    const unsigned g = blockIdx.x * kThreads + threadIdx.x;           // host: H * quads < 2^31 - kThreads
    const unsigned y = g / (unsigned)s.quads;
    if (y >= (unsigned)s.H) return;
    const int x = (int)(g - y * (unsigned)s.quads) * kPix;
    const int n = blockIdx.y;
    const Camera cam = camera_of(s, n);
    const float* dp = s.depth + (size_t)n * (size_t)s.d_image + (size_t)y * (size_t)s.d_row + x;
    const float* fp = s.flow ? s.flow + (size_t)n * (size_t)s.f_image + (size_t)y * (size_t)s.f_row + x : nullptr;
    const size_t o = ((size_t)n * (size_t)s.H + y) * (size_t)s.W + x;                 // of the dense [N][H][W] fields
    const size_t plane = (size_t)s.H * (size_t)s.W;
    const size_t r = o + (size_t)n * plane;                                           // of rigid [N][2][H][W]: u; v one plane on
    float d[kPix], fu[kPix], fv[kPix];
    unsigned ok = 0x01010101u;                                        // the four valid bytes; all judged without a mask
    if (VEC) {                                                        // W % 4 == 0: the four are in the row, 16-byte aligned
        const float4 a = *reinterpret_cast<const float4*>(dp);
        d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w;
        if (fp) {
            const float4 b = *reinterpret_cast<const float4*>(fp), c = *reinterpret_cast<const float4*>(fp + s.f_plane);
            fu[0] = b.x, fu[1] = b.y, fu[2] = b.z, fu[3] = b.w;
            fv[0] = c.x, fv[1] = c.y, fv[2] = c.z, fv[3] = c.w;
            if (s.valid) ok = *reinterpret_cast<const unsigned*>(s.valid + o);
        }
    } else {
        ok = 0;
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            d[k] = fu[k] = fv[k] = NAN;                               // past the row: nothing is read or stored for it
            if (x + k < s.W) {
                d[k] = dp[k];
                if (fp) fu[k] = fp[k], fv[k] = fp[s.f_plane + k];
                ok |= (fp && s.valid ? (s.valid[o + k] ? 1u : 0u) : 1u) << (8 * k);
            }
        }
    }
    float ru[kPix], rv[kPix], e[kPix];
    unsigned lab = 0;
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        const bool inside = project(cam, x + k, (int)y, d[k], s.H, s.W, s.eps, &ru[k], &rv[k]);
        e[k] = INFINITY;
        if (fp) {
            const float t = residual(fu[k], fv[k], ru[k], rv[k], s.alpha, s.beta);
            const bool judged = inside && (ok >> (8 * k) & 255u) != 0 && t == t;
            if (judged) e[k] = t, lab |= (t <= 0.0f ? 1u : 2u) << (8 * k);
        }
    }
    if (VEC) {
        if (s.rigid) {
            *reinterpret_cast<float4*>(s.rigid + r) = make_float4(ru[0], ru[1], ru[2], ru[3]);
            *reinterpret_cast<float4*>(s.rigid + r + plane) = make_float4(rv[0], rv[1], rv[2], rv[3]);
        }
        if (s.excess) *reinterpret_cast<float4*>(s.excess + o) = make_float4(e[0], e[1], e[2], e[3]);
        if (s.label) *reinterpret_cast<unsigned*>(s.label + o) = lab;
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) {
            if (x + k < s.W) {                                        // the row's tail
                if (s.rigid) s.rigid[r + k] = ru[k], s.rigid[r + plane + k] = rv[k];
                if (s.excess) s.excess[o + k] = e[k];
                if (s.label) s.label[o + k] = (unsigned char)(lab >> (8 * k) & 255u);
            }
        }
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

struct Span {                                       // the bytes [lo, hi) an argument covers; empty for a null pointer
    const char* name;
    uintptr_t lo, hi;
};

Span span(const char* name, const void* p, long long bytes) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return Span{name, lo, p ? lo + (uintptr_t)bytes : lo};
}

bool finite_nonneg(float v) { return v >= 0.0f && v < INFINITY; }

}  // namespace

extern "C" {

int dvs_rigid_flow(const float* depth, long long depth_image_stride, long long depth_row_stride, const float* K, const float* inv_K,
                   const float* T, const float* flow, long long flow_image_stride, long long flow_plane_stride, long long flow_row_stride,
                   const unsigned char* valid, float* rigid, float* excess, unsigned char* label, int N, int H, int W, float alpha,
                   float beta, float eps, void* stream) {
    DVS_REQUIRE(N >= 1 && N <= 65535, "dvs_rigid_flow: N=%d images must be in 1 .. 65535", N);
    DVS_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24),
                "dvs_rigid_flow: H=%d, W=%d must be in 1 .. 2^24 (pixel coordinates are exact in fp32)", H, W);
    const long long quads = ((long long)W + kPix - 1) / kPix;
    DVS_REQUIRE((long long)H * quads < (1ll << 31) - kThreads, "dvs_rigid_flow: H * W = %d x %d pixels per image exceed 2^31 - 1 lanes of four", H,
                W);
    DVS_REQUIRE(depth && K && inv_K && T, "dvs_rigid_flow: null pointer (depth, K, inv_K or T)");
    DVS_REQUIRE(aligned(depth, 4) && aligned(K, 4) && aligned(inv_K, 4) && aligned(T, 4), "dvs_rigid_flow: misaligned pointer (depth, K, inv_K or T)");
    const long long extent = (long long)(H - 1) * depth_row_stride + W;
    DVS_REQUIRE(depth_row_stride >= W, "dvs_rigid_flow: depth row stride %lld is below W=%d", depth_row_stride, W);
    DVS_REQUIRE(depth_row_stride < (1ll << 40) && depth_image_stride < (1ll << 40), "dvs_rigid_flow: depth strides %lld, %lld out of range",
                depth_image_stride, depth_row_stride);
    DVS_REQUIRE(depth_image_stride >= extent, "dvs_rigid_flow: depth image stride %lld is below (H - 1) * row stride + W = %lld",
                depth_image_stride, extent);
    long long f_extent = 0;
    if (flow) {
        DVS_REQUIRE(aligned(flow, 4), "dvs_rigid_flow: misaligned pointer (flow)");
        DVS_REQUIRE(flow_row_stride >= W, "dvs_rigid_flow: flow row stride %lld is below W=%d", flow_row_stride, W);
        DVS_REQUIRE(flow_row_stride < (1ll << 40) && flow_plane_stride < (1ll << 40) && flow_image_stride < (1ll << 40),
                    "dvs_rigid_flow: flow strides %lld, %lld, %lld out of range", flow_image_stride, flow_plane_stride, flow_row_stride);
        f_extent = (long long)(H - 1) * flow_row_stride + W;
        DVS_REQUIRE(flow_plane_stride >= f_extent, "dvs_rigid_flow: flow plane stride %lld is below (H - 1) * row stride + W = %lld",
                    flow_plane_stride, f_extent);
        DVS_REQUIRE(flow_image_stride >= flow_plane_stride + f_extent,
                    "dvs_rigid_flow: flow image stride %lld is below plane stride + (H - 1) * row stride + W = %lld", flow_image_stride,
                    flow_plane_stride + f_extent);
    } else {
        DVS_REQUIRE(!excess && !label, "dvs_rigid_flow: excess and label need a flow");     // valid is read with a flow only
    }
    DVS_REQUIRE(finite_nonneg(alpha) && finite_nonneg(beta) && finite_nonneg(eps),
                "dvs_rigid_flow: alpha=%g, beta=%g, eps=%g must be finite and not negative", (double)alpha, (double)beta, (double)eps);
    DVS_REQUIRE(aligned(rigid, 4) && aligned(excess, 4), "dvs_rigid_flow: misaligned pointer (rigid or excess)");
    const long long pixels = (long long)N * H * W;
    const Span ins[] = {span("depth", depth, 4 * ((long long)(N - 1) * depth_image_stride + extent)),
                        span("K", K, 64ll * N),
                        span("inv_K", inv_K, 64ll * N),
                        span("T", T, 64ll * N),
                        span("flow", flow, 4 * ((long long)(N - 1) * flow_image_stride + flow_plane_stride + f_extent)),
                        span("valid", valid, pixels)};
    const Span outs[] = {span("rigid", rigid, 8 * pixels), span("excess", excess, 4 * pixels), span("label", label, pixels)};
    for (const Span& o : outs)
        for (const Span& i : ins)
            DVS_REQUIRE(!(o.lo < i.hi && i.lo < o.hi), "dvs_rigid_flow: output %s overlaps input %s", o.name, i.name);
    if (!rigid && !excess && !label) return DVS_OK;                   // nothing to write: no launch
    Args s;
    s.depth = depth, s.d_image = depth_image_stride, s.d_row = depth_row_stride;
    s.K = K, s.iK = inv_K, s.T = T;
    s.flow = flow, s.f_image = flow_image_stride, s.f_plane = flow_plane_stride, s.f_row = flow_row_stride;
    s.valid = valid, s.rigid = rigid, s.excess = excess, s.label = label;
    s.H = H, s.W = W, s.quads = (int)quads;
    s.alpha = alpha, s.beta = beta, s.eps = eps;
    const bool vec = W % 4 == 0 && depth_row_stride % 4 == 0 && depth_image_stride % 4 == 0 && aligned(depth, 16) &&
                     (!flow || (flow_row_stride % 4 == 0 && flow_plane_stride % 4 == 0 && flow_image_stride % 4 == 0 && aligned(flow, 16))) &&
                     aligned(valid, 4) && aligned(rigid, 16) && aligned(excess, 16) && aligned(label, 4);
    const unsigned lanes = (unsigned)H * (unsigned)quads;
    const dim3 grid((lanes + kThreads - 1) / kThreads, (unsigned)N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(rigid_flow_kernel<true>, grid, dim3(kThreads), 0, st, s);
    else hipLaunchKernelGGL(rigid_flow_kernel<false>, grid, dim3(kThreads), 0, st, s);
    return dvs::check_launch("dvs_rigid_flow");
}

}  // extern "C"
