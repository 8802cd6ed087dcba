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
//   (X, Y, Z) = d * (rx, ry, rz)                             the ray of pixelfield.h
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
// A streaming kernel in the lane geometry of pixelfield.h: a lane owns four consecutive pixels of a row, the image rides in
// blockIdx.y.  Depth, the two flow planes, the valid bytes, rigid, excess and the labels go through pixelfield.h's vector or scalar
// loads and stores.  No LDS, no atomics, no workspace; every output element is written once by the lane that owns it, so the
// result repeats bit for bit and does not depend on the launch geometry or on the batch.
#include "pixelfield.h"

#pragma clang fp contract(off)

namespace {

using namespace dvs;
constexpr int kThreads = kPixThreads;

struct Args {
    Plane depth;
    const float *K, *iK, *T;                        // dense [N][4][4]
    Field flow;                                     // p may be null
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
    Camera c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c.P[i][j] = ((K[4 * i] * T[j] + K[4 * i + 1] * T[4 + j]) + K[4 * i + 2] * T[8 + j]) + K[4 * i + 3] * T[12 + j];
    load_inv_K(s.iK + (size_t)n * 16, c.iK);
    return c;
}

// (ru, rv) of the pixel (x, y) at depth d; returns inside
__device__ __forceinline__ bool project(const Camera& c, int xi, int yi, float d, int H, int W, float eps, float* ru, float* rv) {
    const float x = (float)xi, y = (float)yi;
    float X, Y, Z;
    back_project(c.iK, x, y, d, &X, &Y, &Z);
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
    unsigned y;
    int x;
    lane_pixels(blockIdx.x * kThreads + threadIdx.x, s.quads, &y, &x);
    if (y >= (unsigned)s.H) return;
    const int n = blockIdx.y, count = s.W - x;
    const Camera cam = camera_of(s, n);
    const bool measured = s.flow.p != nullptr;
    const size_t o = ((size_t)n * (size_t)s.H + y) * (size_t)s.W + x;                 // of the dense [N][H][W] fields
    const size_t plane = (size_t)s.H * (size_t)s.W;
    const size_t r = o + (size_t)n * plane;                                           // of rigid [N][2][H][W]: u; v one plane on
    float d[kPix], fu[kPix], fv[kPix];
    unsigned ok = 0;
    load_quad<VEC>(at(s.depth, n, y, x), count, d);
    if (measured) {
        const float* fp = at(s.flow, n, y, x);
        load_quad<VEC>(fp, count, fu);
        load_quad<VEC>(fp + s.flow.plane, count, fv);
        ok = load_mask<VEC>(s.valid ? s.valid + o : nullptr, count);                  // valid is read with a flow only
    }
    float ru[kPix], rv[kPix], e[kPix];
    unsigned lab = 0;
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        const bool inside = project(cam, x + k, (int)y, d[k], s.H, s.W, s.eps, &ru[k], &rv[k]);
        e[k] = INFINITY;
        if (measured) {
            const float t = residual(fu[k], fv[k], ru[k], rv[k], s.alpha, s.beta);
            const bool judged = inside && (ok >> (8 * k) & 255u) != 0 && t == t;
            if (judged) e[k] = t, lab |= (t <= 0.0f ? 1u : 2u) << (8 * k);
        }
    }
    if (s.rigid) {
        store_quad<VEC>(s.rigid + r, count, ru);
        store_quad<VEC>(s.rigid + r + plane, count, rv);
    }
    if (s.excess) store_quad<VEC>(s.excess + o, count, e);
    if (s.label) store_mask<VEC>(s.label + o, count, lab);
}

}  // namespace

extern "C" {

int dvs_rigid_flow(const float* depth, long long depth_image_stride, long long depth_row_stride, const float* K, const float* inv_K,
                   const float* T, const float* flow, long long flow_image_stride, long long flow_plane_stride, long long flow_row_stride,
                   const unsigned char* valid, float* rigid, float* excess, unsigned char* label, int N, int H, int W, float alpha,
                   float beta, float eps, void* stream) {
    const char* who = "dvs_rigid_flow";
    Args s;
    if (int rc = check_shape(who, N, H, W, &s.quads)) return rc;
    s.depth = Plane{depth, depth_image_stride, depth_row_stride};
    s.flow = flow ? Field{flow, flow_image_stride, flow_plane_stride, flow_row_stride} : Field{nullptr, 0, 0, 0};
    if (int rc = check_plane(who, "depth", s.depth, H, W)) return rc;
    if (int rc = check_floats(who, "K", K)) return rc;
    if (int rc = check_floats(who, "inv_K", inv_K)) return rc;
    if (int rc = check_floats(who, "T", T)) return rc;
    if (flow) {
        if (int rc = check_field(who, "flow", s.flow, H, W)) return rc;
    } else {
        DVS_REQUIRE(!excess && !label, "dvs_rigid_flow: excess and label need a flow");     // valid is read with a flow only
    }
    DVS_REQUIRE(finite_nonneg(alpha) && finite_nonneg(beta) && finite_nonneg(eps),
                "dvs_rigid_flow: alpha=%g, beta=%g, eps=%g must be finite and not negative", (double)alpha, (double)beta, (double)eps);
    DVS_REQUIRE(aligned(rigid, 4) && aligned(excess, 4), "dvs_rigid_flow: misaligned pointer (rigid or excess)");
    const long long pixels = (long long)N * H * W;
    const Span ins[] = {span("depth", s.depth, N, H, W), span("K", K, 64ll * N), span("inv_K", inv_K, 64ll * N),
                        span("T", T, 64ll * N), span("flow", s.flow, N, H, W), span("valid", valid, pixels)};
    const Span outs[] = {span("rigid", rigid, 8 * pixels), span("excess", excess, 4 * pixels), span("label", label, pixels)};
    if (int rc = check_overlap(who, outs, ins, "input")) return rc;
    if (!rigid && !excess && !label) return DVS_OK;                   // nothing to write: no launch
    s.K = K, s.iK = inv_K, s.T = T;
    s.valid = valid, s.rigid = rigid, s.excess = excess, s.label = label;
    s.H = H, s.W = W;
    s.alpha = alpha, s.beta = beta, s.eps = eps;
    const bool vector = W % 4 == 0 && vec(s.depth) && vec(s.flow) && aligned(valid, 4) && aligned(rigid, 16) && aligned(excess, 16) &&
                        aligned(label, 4);
    const unsigned lanes = (unsigned)H * (unsigned)s.quads;
    const dim3 grid((lanes + kThreads - 1) / kThreads, (unsigned)N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vector) hipLaunchKernelGGL(rigid_flow_kernel<true>, grid, dim3(kThreads), 0, st, s);
    else hipLaunchKernelGGL(rigid_flow_kernel<false>, grid, dim3(kThreads), 0, st, s);
    return check_launch(who);
}

}  // extern "C"
