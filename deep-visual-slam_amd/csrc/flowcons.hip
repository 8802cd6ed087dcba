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
// A streaming kernel at the launch floor, in the lane geometry of pixelfield.h (a lane owns four consecutive pixels of a row), the
// direction in blockIdx.z and the image in blockIdx.y.  The lane's own flow, its mask bytes and its excess go through pixelfield.h's
// vector or scalar loads and stores; the sixteen taps of the partner are scalar gathers in both forms.  No LDS, no atomics, no
// workspace; every output element is written once by the lane that owns it, so the result repeats bit for bit and does not
// depend on the launch geometry.
#include "pixelfield.h"

#pragma clang fp contract(off)

namespace {

using namespace dvs;
constexpr int kThreads = kPixThreads;

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
    if (!inside) return INFINITY;                                     // NaN included: a pixel past the row's tail reads nothing
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
    unsigned y;
    int x;
    lane_pixels(blockIdx.x * kThreads + threadIdx.x, s.quads, &y, &x);
    if (y >= (unsigned)s.H) return;
    const int n = blockIdx.y, dir = blockIdx.z, count = s.W - x;
    const Field own = s.flow[dir], oth = s.flow[dir ^ 1];
    const float* mine = at(own, n, y, x);
    const float* other = at(oth, n, 0, 0);
    float u[kPix], v[kPix], e[kPix];
    load_quad<VEC>(mine, count, u);
    load_quad<VEC>(mine + own.plane, count, v);
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
        e[k] = excess_of(oth, other, x + k, (int)y, s.H, s.W, u[k], v[k], s.alpha, s.beta);
        m |= (e[k] <= 0.0f ? 1u : 0u) << (8 * k);
    }
    const size_t o = ((size_t)n * (size_t)s.H + y) * (size_t)s.W + x;
    if (s.valid[dir]) store_mask<VEC>(s.valid[dir] + o, count, m);
    if (s.excess[dir]) store_quad<VEC>(s.excess[dir] + o, count, e);
}

}  // namespace

extern "C" {

int dvs_flow_consistency(const float* a, long long a_image_stride, long long a_plane_stride, long long a_row_stride, const float* b,
                         long long b_image_stride, long long b_plane_stride, long long b_row_stride, unsigned char* valid_a,
                         unsigned char* valid_b, float* excess_a, float* excess_b, int N, int H, int W, float alpha, float beta,
                         void* stream) {
    const char* who = "dvs_flow_consistency";
    Pair s;
    if (int rc = check_shape(who, N, H, W, &s.quads)) return rc;
    s.flow[0] = Field{a, a_image_stride, a_plane_stride, a_row_stride};
    s.flow[1] = Field{b, b_image_stride, b_plane_stride, b_row_stride};
    if (int rc = check_field(who, "a", s.flow[0], H, W)) return rc;
    if (int rc = check_field(who, "b", s.flow[1], H, W)) return rc;
    DVS_REQUIRE(finite_nonneg(alpha) && finite_nonneg(beta), "dvs_flow_consistency: alpha=%g, beta=%g must be finite and not negative",
                (double)alpha, (double)beta);
    DVS_REQUIRE(aligned(excess_a, 4) && aligned(excess_b, 4), "dvs_flow_consistency: misaligned pointer (excess)");
    s.valid[0] = valid_a, s.valid[1] = valid_b;
    s.excess[0] = excess_a, s.excess[1] = excess_b;
    s.H = H, s.W = W;
    s.alpha = alpha, s.beta = beta;
    if (!valid_a && !valid_b && !excess_a && !excess_b) return DVS_OK;            // nothing to write: no launch
    const bool vector = W % 4 == 0 && vec(s.flow[0]) && vec(s.flow[1]) && aligned(valid_a, 4) && aligned(valid_b, 4) &&
                        aligned(excess_a, 16) && aligned(excess_b, 16);
    const unsigned lanes = (unsigned)H * (unsigned)s.quads;
    const dim3 grid((lanes + kThreads - 1) / kThreads, (unsigned)N, 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vector) hipLaunchKernelGGL(flow_consistency_kernel<true>, grid, dim3(kThreads), 0, st, s);
    else hipLaunchKernelGGL(flow_consistency_kernel<false>, grid, dim3(kThreads), 0, st, s);
    return check_launch(who);
}

}  // extern "C"
