// Gate arithmetic of RAFT's ConvGRU (model/raft/core/update.py:23-31) around the three convolutions that stay per iteration.
//
// The reference forms z, r and q from ONE 242-channel concatenation cat[h, inp, motion, flow].  A convolution is linear in its
// input channels, so the pre-activations are sums of convolutions of the parts (raft_update.py):
//     a_h [P][2hd]  conv(h)        z and r columns
//     a_x [P][3hd]  conv(motion)   z, r and q columns
//     c   [P][3hd]  conv(inp) + biases, the same in every iteration of a forward pass
//     a_q [P][hd]   conv(r * h)
//
//   gates fwd   z = sigmoid(a_h + a_x + c), r = sigmoid(a_h + a_x + c), rh = r * h
//   blend fwd   q = tanh(a_q + a_x + c), h' = (1 - z) * h + z * q
//   blend bwd   dpre_q = g * z * (1 - q^2), dpre_z = g * (q - h) * z * (1 - z), dh_a = g * (1 - z)
//   gates bwd   dpre_r = d_rh * h * r * (1 - r), dh = dh_a + d_rh * r
//
// dpre [P][3hd] = (dpre_z, dpre_r, dpre_q) is the gradient of a_x and of c at once.  The gradients of a_h (its first 2hd columns)
// and of a_q (its last hd) are ALSO written as contiguous matrices dah [P][2hd] and dq [P][hd]: the convolution backward reads
// dense NHWC rows, and a strided copy would read and write those 12 * hd bytes per pixel again in a launch of its own.
//
// Layout: P = B*H*W pixel rows of a channels_last tensor.  One thread owns four consecutive channels of one pixel (16-byte loads
// and stores), every output element has one owner and no atomics: two runs agree bit for bit.  Element offsets are 64-bit; the
// grid covers P * hd / 4 items, 256 per workgroup, and strides where that exceeds the 2^31 - 1 workgroups of a launch.
// Memory-bound by a wide margin (one expf or tanhf per 28 .. 40 bytes), so the math library's functions are used, not the fast
// intrinsics.  sigmoid is evaluated on e = exp(-|x|) <= 1, which cannot overflow: 1 / (1 + e) or e / (1 + e).
#include "common.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

__device__ __forceinline__ float sigmoidf(float x) {
    const float e = expf(-fabsf(x));
    const float d = 1.0f + e;
    return (x >= 0.0f ? 1.0f : e) / d;
}

#define DVS_GRU_MAP4(out, expr)                          \
    do {                                                 \
        { const int k = 0; (out).x = (expr); }           \
        { const int k = 1; (out).y = (expr); }           \
        { const int k = 2; (out).z = (expr); }           \
        { const int k = 3; (out).w = (expr); }           \
    } while (0)

__device__ __forceinline__ float at(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// item -> (pixel, first channel): a 32-bit division whenever the item count allows it
__device__ __forceinline__ void split(size_t item, unsigned q, bool narrow, size_t& p, unsigned& ch) {
    if (narrow) {
        const unsigned pi = (unsigned)item / q;
        p = pi;
        ch = ((unsigned)item - pi * q) * 4u;
    } else {
        p = item / q;
        ch = (unsigned)(item - p * q) * 4u;
    }
}

struct Shape {
    size_t items;       // P * hd / 4
    unsigned hd, q;     // hidden channels, hd / 4
    bool narrow;        // items < 2^32
};

__global__ void __launch_bounds__(kThreads)
gru_gates_fwd_kernel(Shape s, const float* __restrict__ a_h, const float* __restrict__ a_x, const float* __restrict__ c,
                     const float* __restrict__ h, float* __restrict__ z, float* __restrict__ r, float* __restrict__ rh) {
    const size_t step = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < s.items; i += step) {
        size_t p;
        unsigned ch;
        split(i, s.q, s.narrow, p, ch);
        const size_t o1 = i * 4, o2 = p * 2 * s.hd + ch, o3 = p * 3 * s.hd + ch;
        const float4 hz = ld4(a_h + o2), hr = ld4(a_h + o2 + s.hd);
        const float4 xz = ld4(a_x + o3), xr = ld4(a_x + o3 + s.hd);
        const float4 cz = ld4(c + o3), cr = ld4(c + o3 + s.hd);
        const float4 hv = ld4(h + o1);
        float4 zv, rv, rhv;
        DVS_GRU_MAP4(zv, sigmoidf((at(hz, k) + at(xz, k)) + at(cz, k)));
        DVS_GRU_MAP4(rv, sigmoidf((at(hr, k) + at(xr, k)) + at(cr, k)));
        DVS_GRU_MAP4(rhv, at(rv, k) * at(hv, k));
        st4(z + o1, zv);
        st4(r + o1, rv);
        st4(rh + o1, rhv);
    }
}

__global__ void __launch_bounds__(kThreads)
gru_blend_fwd_kernel(Shape s, const float* __restrict__ a_q, const float* __restrict__ a_x, const float* __restrict__ c,
                     const float* __restrict__ z, const float* __restrict__ h, float* __restrict__ q, float* __restrict__ h_new) {
    const size_t step = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < s.items; i += step) {
        size_t p;
        unsigned ch;
        split(i, s.q, s.narrow, p, ch);
        const size_t o1 = i * 4, o3 = p * 3 * s.hd + 2 * s.hd + ch;
        const float4 aq = ld4(a_q + o1), xq = ld4(a_x + o3), cq = ld4(c + o3);
        const float4 zv = ld4(z + o1), hv = ld4(h + o1);
        float4 qv, hn;
        DVS_GRU_MAP4(qv, tanhf((at(aq, k) + at(xq, k)) + at(cq, k)));
        DVS_GRU_MAP4(hn, (1.0f - at(zv, k)) * at(hv, k) + at(zv, k) * at(qv, k));
        st4(q + o1, qv);
        st4(h_new + o1, hn);
    }
}

__global__ void __launch_bounds__(kThreads)
gru_blend_bwd_kernel(Shape s, const float* __restrict__ g, const float* __restrict__ z, const float* __restrict__ q,
                     const float* __restrict__ h, float* __restrict__ dpre, float* __restrict__ dah, float* __restrict__ dq,
                     float* __restrict__ dh_a) {
    const size_t step = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < s.items; i += step) {
        size_t p;
        unsigned ch;
        split(i, s.q, s.narrow, p, ch);
        const size_t o1 = i * 4, o2 = p * 2 * s.hd + ch, o3 = p * 3 * s.hd + ch;
        const float4 gv = ld4(g + o1), zv = ld4(z + o1), qv = ld4(q + o1), hv = ld4(h + o1);
        float4 dqv, dzv, dhv;
        DVS_GRU_MAP4(dqv, at(gv, k) * at(zv, k) * (1.0f - at(qv, k) * at(qv, k)));
        DVS_GRU_MAP4(dzv, at(gv, k) * (at(qv, k) - at(hv, k)) * at(zv, k) * (1.0f - at(zv, k)));
        DVS_GRU_MAP4(dhv, at(gv, k) * (1.0f - at(zv, k)));
        st4(dpre + o3, dzv);
        st4(dpre + o3 + 2 * s.hd, dqv);
        st4(dah + o2, dzv);
        st4(dq + o1, dqv);
        st4(dh_a + o1, dhv);
    }
}

__global__ void __launch_bounds__(kThreads)
gru_gates_bwd_kernel(Shape s, const float* __restrict__ d_rh, const float* __restrict__ h, const float* __restrict__ r,
                     const float* __restrict__ dh_a, float* __restrict__ dpre, float* __restrict__ dah, float* __restrict__ dh) {
    const size_t step = (size_t)gridDim.x * kThreads;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < s.items; i += step) {
        size_t p;
        unsigned ch;
        split(i, s.q, s.narrow, p, ch);
        const size_t o1 = i * 4, o2 = p * 2 * s.hd + s.hd + ch, o3 = p * 3 * s.hd + s.hd + ch;
        const float4 dv = ld4(d_rh + o1), hv = ld4(h + o1), rv = ld4(r + o1), av = ld4(dh_a + o1);
        float4 drv, dhv;
        DVS_GRU_MAP4(drv, at(dv, k) * at(hv, k) * at(rv, k) * (1.0f - at(rv, k)));
        DVS_GRU_MAP4(dhv, at(av, k) + at(dv, k) * at(rv, k));
        st4(dpre + o3, drv);
        st4(dah + o2, drv);
        st4(dh + o1, dhv);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int make_shape(const char* who, size_t P, int hidden, Shape* s, unsigned* grid) {
    DVS_REQUIRE(hidden > 0, "%s: hidden=%d must be positive", who, hidden);
    DVS_REQUIRE(hidden % 4 == 0, "%s: hidden=%d must be a multiple of 4 (16-byte channel groups)", who, hidden);
    DVS_REQUIRE(P > 0, "%s: P=0 pixel rows", who);
    DVS_REQUIRE(P <= (SIZE_MAX / 16) / (size_t)hidden, "%s: P=%zu rows of 3*%d floats overflow a 64-bit byte offset", who, P, hidden);
    s->hd = (unsigned)hidden;
    s->q = (unsigned)hidden / 4;
    s->items = P * s->q;
    s->narrow = s->items < (1ull << 32);
    const size_t blocks = (s->items + kThreads - 1) / kThreads;
    *grid = (unsigned)(blocks < 0x7fffffffull ? blocks : 0x7fffffffull);       // beyond that the kernels stride
    return DVS_OK;
}

}  // namespace

extern "C" {

int dvs_gru_gates_fwd(const float* a_h, const float* a_x, const float* c, const float* h, float* z, float* r, float* rh, size_t P,
                      int hidden, void* stream) {
    DVS_REQUIRE(a_h && a_x && c && h && z && r && rh, "dvs_gru_gates_fwd: null pointer");
    DVS_REQUIRE(aligned16(a_h) && aligned16(a_x) && aligned16(c) && aligned16(h) && aligned16(z) && aligned16(r) && aligned16(rh),
                "dvs_gru_gates_fwd: misaligned pointer");
    Shape s;
    unsigned grid;
    if (int rc = make_shape("dvs_gru_gates_fwd", P, hidden, &s, &grid)) return rc;
    hipLaunchKernelGGL(gru_gates_fwd_kernel, dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), s, a_h, a_x, c, h, z, r, rh);
    return dvs::check_launch("dvs_gru_gates_fwd");
}

int dvs_gru_blend_fwd(const float* a_q, const float* a_x, const float* c, const float* z, const float* h, float* q, float* h_new,
                      size_t P, int hidden, void* stream) {
    DVS_REQUIRE(a_q && a_x && c && z && h && q && h_new, "dvs_gru_blend_fwd: null pointer");
    DVS_REQUIRE(aligned16(a_q) && aligned16(a_x) && aligned16(c) && aligned16(z) && aligned16(h) && aligned16(q) && aligned16(h_new),
                "dvs_gru_blend_fwd: misaligned pointer");
    Shape s;
    unsigned grid;
    if (int rc = make_shape("dvs_gru_blend_fwd", P, hidden, &s, &grid)) return rc;
    hipLaunchKernelGGL(gru_blend_fwd_kernel, dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), s, a_q, a_x, c, z, h, q,
                       h_new);
    return dvs::check_launch("dvs_gru_blend_fwd");
}

int dvs_gru_blend_bwd(const float* g, const float* z, const float* q, const float* h, float* dpre, float* dah, float* dq, float* dh_a,
                      size_t P, int hidden, void* stream) {
    DVS_REQUIRE(g && z && q && h && dpre && dah && dq && dh_a, "dvs_gru_blend_bwd: null pointer");
    DVS_REQUIRE(aligned16(g) && aligned16(z) && aligned16(q) && aligned16(h) && aligned16(dpre) && aligned16(dah) && aligned16(dq) &&
                    aligned16(dh_a), "dvs_gru_blend_bwd: misaligned pointer");
    Shape s;
    unsigned grid;
    if (int rc = make_shape("dvs_gru_blend_bwd", P, hidden, &s, &grid)) return rc;
    hipLaunchKernelGGL(gru_blend_bwd_kernel, dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), s, g, z, q, h, dpre, dah,
                       dq, dh_a);
    return dvs::check_launch("dvs_gru_blend_bwd");
}

int dvs_gru_gates_bwd(const float* d_rh, const float* h, const float* r, const float* dh_a, float* dpre, float* dah, float* dh,
                      size_t P, int hidden, void* stream) {
    DVS_REQUIRE(d_rh && h && r && dh_a && dpre && dah && dh, "dvs_gru_gates_bwd: null pointer");
    DVS_REQUIRE(aligned16(d_rh) && aligned16(h) && aligned16(r) && aligned16(dh_a) && aligned16(dpre) && aligned16(dah) && aligned16(dh),
                "dvs_gru_gates_bwd: misaligned pointer");
    Shape s;
    unsigned grid;
    if (int rc = make_shape("dvs_gru_gates_bwd", P, hidden, &s, &grid)) return rc;
    hipLaunchKernelGGL(gru_gates_bwd_kernel, dim3(grid), dim3(kThreads), 0, static_cast<hipStream_t>(stream), s, d_rh, h, r, dh_a, dpre,
                       dah, dh);
    return dvs::check_launch("dvs_gru_gates_bwd");
}

}  // extern "C"
