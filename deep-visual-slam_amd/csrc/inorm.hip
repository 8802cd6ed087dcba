// InstanceNorm2d with the Bottleneck tail fused (model/raft/core/extractor.py:60-116, norm_fn = 'instance' and 'none').
//
//   forward    z   = norm ? (y - mean[n,c]) * invstd[n,c] : y                 nn.InstanceNorm2d(C): no affine, no running
//              z   = relu ? max(z, 0) : z                                     statistics, biased variance, eps = 1e-5, the
//              out = residual ? max(residual + z, 0) : z                      input's own statistics in train and eval mode
//   backward   g   = residual ? dout * [out > 0] : dout                       (also written as d residual)
//              du  = relu ? g * [z > 0] : g
//              dy  = norm ? invstd * (du - mean_hw(du) - xhat * mean_hw(du * xhat)) : du
//
// Layout: fp32 NHWC [N][HW][C], C % 4 == 0.  A lane owns 4 consecutive channels of a pixel (16-byte loads and stores).  A
// workgroup of 256 threads is cut into R = 256 / (C/4) pixel rows of C/4 lanes; the 256 - R * (C/4) lanes left over when C/4
// does not divide 256 (C = 24: 4 of them, C = 96: 16) only take part in the barriers.
//
// Slices.  An image is cut into slices of kSlice = 1024 pixels (the last one ragged); workgroup (s, n) handles slice s of image
// n, in every kernel.  The statistics kernel makes one (mean, M2) pair per slice and channel -- the slice's mean first, then the
// sum of squared deviations around it in a second pass over the same 1024 * C floats (L2 hits), with the first-order term that
// corrects the first pass's rounding -- and writes it to the workspace [N][S][2][C].  The applying kernel's workgroups each merge
// the S pairs of their image at their head with Chan's formula: lane (row, cg) folds slices row, row + R, .. in ascending order
// (independent loads, one L2 round trip deep instead of S), then the rows are folded by a fixed tree.  Every workgroup of an
// image performs the same operations in the same order and arrives at the same bits.  sum(x^2) / n - mean^2 appears nowhere.
// The backward's two sums per channel (du and du * xhat) take the same route with plain additions.
//
// No atomics anywhere and a fixed reduction order: two runs agree bit for bit, and an image's result does not depend on its
// neighbours in the batch.  The sign test [z > 0] of the backward recomputes z from y, mean and invstd through inorm_z(), the one
// function the forward uses, so both sites round alike.
#include "common.h"

#include <cstdint>

namespace {

constexpr int kThreads = 256;
constexpr int kSlice = 1024;            // pixels per slice: T of the tests and of DESIGN.md
constexpr float kEps = 1e-5f;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// (y - mean) * invstd: one subtraction and one fmaf with a zero addend.  Neither can be contracted with a neighbouring operation,
// so the forward's value and the backward's recomputed one are the same bits.
__device__ __forceinline__ float inorm_z(float y, float mean, float invstd) { return fmaf(__fsub_rn(y, mean), invstd, 0.0f); }

struct Geo {
    size_t HW;          // pixels per image
    int C, Q, R;        // channels, C / 4, pixel rows per workgroup
    int S;              // slices per image
};

struct Lane {
    bool on;
    int row, cg;
    size_t p0, p1;      // this workgroup's pixels [p0, p1) of image n
    size_t base;        // float offset of pixel 0 of image n, plus 4 * cg
};

__device__ __forceinline__ Lane lane_of(const Geo& g) {
    Lane l;
    const int t = threadIdx.x;
    l.on = t < g.R * g.Q;
    l.row = t / g.Q;
    l.cg = t - l.row * g.Q;
    l.p0 = (size_t)blockIdx.x * kSlice;
    l.p1 = l.p0 + kSlice < g.HW ? l.p0 + kSlice : g.HW;
    l.base = (size_t)blockIdx.y * g.HW * g.C + 4 * l.cg;
    return l;
}

// Sum over the rows of the workgroup by a fixed tree; every lane gets the total of its channel group.
__device__ __forceinline__ f32x4 rows_sum(f32x4 v, const Lane& l, const Geo& g, f32x4* sm) {
    __syncthreads();
    if (l.on) sm[threadIdx.x] = v;
    int top = 1;
    while (top < g.R) top <<= 1;
    for (int step = top >> 1; step >= 1; step >>= 1) {
        __syncthreads();
        if (l.on && l.row < step && l.row + step < g.R) sm[threadIdx.x] += sm[threadIdx.x + step * g.Q];
    }
    __syncthreads();
    return sm[l.on ? l.cg : 0];
}

// ---- forward statistics: (mean, M2) of one slice ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) inorm_stats_kernel(Geo g, const float* __restrict__ y, float* __restrict__ ws) {
    __shared__ f32x4 sm[kThreads];
    const Lane l = lane_of(g);
    const float cnt = (float)(l.p1 - l.p0);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (l.on)
        for (size_t p = l.p0 + l.row; p < l.p1; p += g.R) s += ld4(y + l.base + p * g.C);
    const f32x4 m0 = rows_sum(s, l, g, sm) / cnt;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (l.on)
        for (size_t p = l.p0 + l.row; p < l.p1; p += g.R) {
            const f32x4 d = ld4(y + l.base + p * g.C) - m0;
            s1 += d;
#pragma unroll
            for (int j = 0; j < 4; ++j) s2[j] = fmaf(d[j], d[j], s2[j]);
        }
    s1 = rows_sum(s1, l, g, sm);
    s2 = rows_sum(s2, l, g, sm);
    if (l.on && l.row == 0) {
        // s1 is what the first pass's rounding left of the mean; a constant channel gets its value back exactly and M2 = 0
        f32x4 mean, m2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float corr = s1[j] / cnt;
            mean[j] = m0[j] + corr;
            m2[j] = fmaxf(s2[j] - s1[j] * corr, 0.0f);
        }
        float* out = ws + ((size_t)blockIdx.y * g.S + blockIdx.x) * 2 * g.C + 4 * l.cg;
        st4(out, mean);
        st4(out + g.C, m2);
    }
}

struct Moments {
    float n;
    f32x4 mean, m2;
};

// Chan, Golub, LeVeque: b folded into a.  An empty side is the identity.
__device__ __forceinline__ void chan(Moments& a, const Moments& b) {
    if (b.n == 0.0f) return;
    if (a.n == 0.0f) {
        a = b;
        return;
    }
    const float n = a.n + b.n, fb = b.n / n, fab = a.n * fb;
    const f32x4 d = b.mean - a.mean;
    a.mean += d * fb;
    a.m2 += b.m2 + d * d * fab;
    a.n = n;
}

// mean and invstd of image blockIdx.y for every lane's channel group, from the S slice pairs.
__device__ __forceinline__ void image_stats(const Geo& g, const Lane& l, const float* __restrict__ ws, f32x4* sm_mean, f32x4* sm_m2,
                                            float* sm_n, f32x4& mean, f32x4& invstd) {
    Moments a;
    a.n = 0.0f;
    a.mean = a.m2 = f32x4{0.f, 0.f, 0.f, 0.f};
    if (l.on) {
        const float* img = ws + (size_t)blockIdx.y * g.S * 2 * g.C + 4 * l.cg;
        for (int s = l.row; s < g.S; s += g.R) {
            Moments b;
            const size_t q0 = (size_t)s * kSlice;
            b.n = (float)((q0 + kSlice < g.HW ? q0 + kSlice : g.HW) - q0);
            b.mean = ld4(img + (size_t)s * 2 * g.C);
            b.m2 = ld4(img + (size_t)s * 2 * g.C + g.C);
            chan(a, b);
        }
        sm_mean[threadIdx.x] = a.mean;
        sm_m2[threadIdx.x] = a.m2;
        sm_n[threadIdx.x] = a.n;
    }
    int top = 1;
    while (top < g.R) top <<= 1;
    for (int step = top >> 1; step >= 1; step >>= 1) {
        __syncthreads();
        if (l.on && l.row < step && l.row + step < g.R) {
            const int o = threadIdx.x + step * g.Q;
            Moments b;
            b.n = sm_n[o];
            b.mean = sm_mean[o];
            b.m2 = sm_m2[o];
            chan(a, b);
            sm_mean[threadIdx.x] = a.mean;
            sm_m2[threadIdx.x] = a.m2;
            sm_n[threadIdx.x] = a.n;
        }
    }
    __syncthreads();
    const int src = l.on ? l.cg : 0;
    mean = sm_mean[src];
    const f32x4 m2 = sm_m2[src];
    const float hw = (float)g.HW;
#pragma unroll
    for (int j = 0; j < 4; ++j) invstd[j] = 1.0f / sqrtf(m2[j] / hw + kEps);
}

// ---- forward apply ------------------------------------------------------------------------------------------------------------
template <bool NORM>
__global__ void __launch_bounds__(kThreads)
inorm_apply_kernel(Geo g, const float* __restrict__ y, const float* __restrict__ res, const float* __restrict__ ws,
                   float* __restrict__ out, float* __restrict__ table, int relu) {
    const Lane l = lane_of(g);
    f32x4 mean = {0.f, 0.f, 0.f, 0.f}, invstd = {1.f, 1.f, 1.f, 1.f};
    if (NORM) {
        __shared__ f32x4 sm_mean[kThreads], sm_m2[kThreads];
        __shared__ float sm_n[kThreads];
        image_stats(g, l, ws, sm_mean, sm_m2, sm_n, mean, invstd);
        if (blockIdx.x == 0 && l.on && l.row == 0) {
            float* t = table + (size_t)blockIdx.y * 2 * g.C + 4 * l.cg;
            st4(t, mean);
            st4(t + g.C, invstd);
        }
    }
    if (!l.on) return;
    for (size_t p = l.p0 + l.row; p < l.p1; p += g.R) {
        const size_t o = l.base + p * g.C;
        f32x4 v = ld4(y + o);
        if (NORM) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = inorm_z(v[j], mean[j], invstd[j]);
        }
        if (relu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.0f);
        }
        if (res) {
            const f32x4 r = ld4(res + o);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(r[j] + v[j], 0.0f);
        }
        st4(out + o, v);
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// du and xhat of one 4-channel item; g (the gradient behind the residual's ReLU) on the way
__device__ __forceinline__ void bwd_item(const float* __restrict__ dout, const float* __restrict__ y, const float* __restrict__ out,
                                         size_t o, const f32x4& mean, const f32x4& invstd, bool norm, int relu, f32x4& gv, f32x4& du,
                                         f32x4& xh) {
    gv = ld4(dout + o);
    if (out) {
        const f32x4 ov = ld4(out + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[j] = ov[j] > 0.0f ? gv[j] : 0.0f;
    }
    xh = ld4(y + o);
    if (norm) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xh[j] = inorm_z(xh[j], mean[j], invstd[j]);
    }
    du = gv;
    if (relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) du[j] = xh[j] > 0.0f ? gv[j] : 0.0f;
    }
}

// per slice and channel: sum du, sum du * xhat -> ws [N][S][2][C]
__global__ void __launch_bounds__(kThreads)
inorm_bwd_reduce_kernel(Geo g, const float* __restrict__ dout, const float* __restrict__ y, const float* __restrict__ out,
                        const float* __restrict__ table, float* __restrict__ ws, int relu) {
    __shared__ f32x4 sm[kThreads];
    const Lane l = lane_of(g);
    f32x4 mean = {0.f, 0.f, 0.f, 0.f}, invstd = {1.f, 1.f, 1.f, 1.f};
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (l.on) {
        const float* t = table + (size_t)blockIdx.y * 2 * g.C + 4 * l.cg;
        mean = ld4(t);
        invstd = ld4(t + g.C);
        for (size_t p = l.p0 + l.row; p < l.p1; p += g.R) {
            f32x4 gv, du, xh;
            bwd_item(dout, y, out, l.base + p * g.C, mean, invstd, true, relu, gv, du, xh);
            a += du;
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = fmaf(du[j], xh[j], b[j]);
        }
    }
    a = rows_sum(a, l, g, sm);
    b = rows_sum(b, l, g, sm);
    if (l.on && l.row == 0) {
        float* o = ws + ((size_t)blockIdx.y * g.S + blockIdx.x) * 2 * g.C + 4 * l.cg;
        st4(o, a);
        st4(o + g.C, b);
    }
}

template <bool NORM>
__global__ void __launch_bounds__(kThreads)
inorm_bwd_apply_kernel(Geo g, const float* __restrict__ dout, const float* __restrict__ y, const float* __restrict__ out,
                       const float* __restrict__ table, const float* __restrict__ ws, float* __restrict__ dy,
                       float* __restrict__ dres, int relu) {
    const Lane l = lane_of(g);
    f32x4 mean = {0.f, 0.f, 0.f, 0.f}, invstd = {1.f, 1.f, 1.f, 1.f};
    f32x4 m_du = {0.f, 0.f, 0.f, 0.f}, m_dux = {0.f, 0.f, 0.f, 0.f};
    if (NORM) {
        // the image's two sums from the S slice sums: lane (row, cg) adds slices row, row + R, .. in ascending order, then the tree
        __shared__ f32x4 sm[kThreads];
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (l.on) {
            const float* img = ws + (size_t)blockIdx.y * g.S * 2 * g.C + 4 * l.cg;
            for (int s = l.row; s < g.S; s += g.R) {
                a += ld4(img + (size_t)s * 2 * g.C);
                b += ld4(img + (size_t)s * 2 * g.C + g.C);
            }
            const float* t = table + (size_t)blockIdx.y * 2 * g.C + 4 * l.cg;
            mean = ld4(t);
            invstd = ld4(t + g.C);
        }
        const float hw = (float)g.HW;
        m_du = rows_sum(a, l, g, sm) / hw;
        m_dux = rows_sum(b, l, g, sm) / hw;
    }
    if (!l.on) return;
    for (size_t p = l.p0 + l.row; p < l.p1; p += g.R) {
        const size_t o = l.base + p * g.C;
        f32x4 gv, du, xh;
        bwd_item(dout, y, out, o, mean, invstd, NORM, relu, gv, du, xh);
        if (NORM) {
#pragma unroll
            for (int j = 0; j < 4; ++j) du[j] = invstd[j] * ((du[j] - m_du[j]) - xh[j] * m_dux[j]);
        }
        st4(dy + o, du);
        if (dres) st4(dres + o, gv);
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int make_geo(const char* who, int N, size_t HW, int C, Geo* g) {
    DVS_REQUIRE(C >= 4 && C <= 1024 && C % 4 == 0, "%s: C=%d must be a multiple of 4 in 4 .. 1024 (16-byte channel groups)", who, C);
    DVS_REQUIRE(N >= 1 && N <= 65535, "%s: N=%d images must be in 1 .. 65535 (one grid row each)", who, N);
    DVS_REQUIRE(HW >= 2, "%s: HW=%zu: instance norm needs more than one spatial element per image", who, HW);
    DVS_REQUIRE(HW <= 0x7fffffffull, "%s: HW=%zu pixels per image exceed 2^31 - 1", who, HW);
    DVS_REQUIRE((size_t)N * HW <= (SIZE_MAX / 16) / (size_t)C, "%s: N*HW*C = %d*%zu*%d floats overflow a 64-bit byte offset", who, N, HW, C);
    g->HW = HW;
    g->C = C;
    g->Q = C / 4;
    g->R = kThreads / g->Q;
    g->S = (int)((HW + kSlice - 1) / kSlice);
    return DVS_OK;
}

size_t ws_bytes_of(int N, const Geo& g) { return (size_t)N * g.S * 2 * g.C * sizeof(float); }

}  // namespace

extern "C" {

int dvs_inorm_slice_pixels(void) { return kSlice; }

size_t dvs_inorm_workspace(int N, size_t HW, int C) {
    Geo g;
    if (make_geo("dvs_inorm_workspace", N, HW, C, &g)) return 0;
    return ws_bytes_of(N, g);
}

int dvs_inorm_fwd(const float* y, const float* residual, float* out, float* table, void* workspace, size_t workspace_bytes, int N,
                  size_t HW, int C, int norm, int relu, void* stream) {
    DVS_REQUIRE(y && out, "dvs_inorm_fwd: null pointer (y, out)");
    DVS_REQUIRE(aligned16(y) && aligned16(residual) && aligned16(out) && aligned16(table) && aligned16(workspace),
                "dvs_inorm_fwd: misaligned pointer");
    Geo g;
    if (int rc = make_geo("dvs_inorm_fwd", N, HW, C, &g)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)g.S, (unsigned)N);
    if (norm) {
        DVS_REQUIRE(table && workspace, "dvs_inorm_fwd: null pointer (table and workspace are required with norm = 1)");
        DVS_REQUIRE(workspace_bytes >= ws_bytes_of(N, g), "dvs_inorm_fwd: workspace of %zu bytes, dvs_inorm_workspace asks for %zu",
                    workspace_bytes, ws_bytes_of(N, g));
        float* ws = static_cast<float*>(workspace);
        hipLaunchKernelGGL(inorm_stats_kernel, grid, dim3(kThreads), 0, st, g, y, ws);
        hipLaunchKernelGGL(inorm_apply_kernel<true>, grid, dim3(kThreads), 0, st, g, y, residual, ws, out, table, relu);
    } else {
        hipLaunchKernelGGL(inorm_apply_kernel<false>, grid, dim3(kThreads), 0, st, g, y, residual, nullptr, out, nullptr, relu);
    }
    return dvs::check_launch("dvs_inorm_fwd");
}

int dvs_inorm_bwd(const float* dout, const float* y, const float* out, const float* table, float* dy, float* dresidual,
                  void* workspace, size_t workspace_bytes, int N, size_t HW, int C, int norm, int relu, void* stream) {
    DVS_REQUIRE(dout && y && dy, "dvs_inorm_bwd: null pointer (dout, y, dy)");
    DVS_REQUIRE((out == nullptr) == (dresidual == nullptr),
                "dvs_inorm_bwd: out and dresidual go together (both with a residual, neither without)");
    DVS_REQUIRE(aligned16(dout) && aligned16(y) && aligned16(out) && aligned16(table) && aligned16(dy) && aligned16(dresidual) &&
                    aligned16(workspace), "dvs_inorm_bwd: misaligned pointer");
    Geo g;
    if (int rc = make_geo("dvs_inorm_bwd", N, HW, C, &g)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)g.S, (unsigned)N);
    if (norm) {
        DVS_REQUIRE(table && workspace, "dvs_inorm_bwd: null pointer (table and workspace are required with norm = 1)");
        DVS_REQUIRE(workspace_bytes >= ws_bytes_of(N, g), "dvs_inorm_bwd: workspace of %zu bytes, dvs_inorm_workspace asks for %zu",
                    workspace_bytes, ws_bytes_of(N, g));
        float* ws = static_cast<float*>(workspace);
        hipLaunchKernelGGL(inorm_bwd_reduce_kernel, grid, dim3(kThreads), 0, st, g, dout, y, out, table, ws, relu);
        hipLaunchKernelGGL(inorm_bwd_apply_kernel<true>, grid, dim3(kThreads), 0, st, g, dout, y, out, table, ws, dy, dresidual, relu);
    } else {
        hipLaunchKernelGGL(inorm_bwd_apply_kernel<false>, grid, dim3(kThreads), 0, st, g, dout, y, out, nullptr, nullptr, dy, dresidual,
                           relu);
    }
    return dvs::check_launch("dvs_inorm_bwd");
}

}  // extern "C"
