// FlowPoseNet's tail (model/posenet_single.py:115-118, 137-142): ReLU, global average pooling, Linear and the pose scale, with
// its backward.
//
//   forward    a(v)       = relu ? max(v, 0) : v
//              mean[n][c] = (1/P) sum_p a(y[n][p][c])
//              out[n][j]  = scale * (b[j] + sum_c W[j][c] * mean[n][c])
//   backward   g[n][c]    = (scale/P) sum_j dout[n][j] * W[j][c]
//              dy[n][p][c] = relu ? (y > 0 ? g : 0) : g
//              dW[j][c]   = scale * sum_n dout[n][j] * mean[n][c]              written, not accumulated
//              db[j]      = scale * sum_n dout[n][j]
//
// Layout: fp32 NHWC [N][P][C], C % 4 == 0.  As in inorm.hip a lane owns 4 consecutive channels of a pixel (16-byte loads and
// stores) and a workgroup of 256 threads is cut into R = 256 / (C/4) pixel rows of C/4 lanes; the lanes left over when C/4 does not
// divide 256 only take part in the barriers.
//
// Slices.  An image is cut into slices of kSlice = 256 pixels (the last one ragged); workgroup (s, n) handles slice s of image n.
// The pooling kernel writes one mean per slice and channel to the workspace [N][S][C]: the rows' sums in pixel order, the rows
// folded by a fixed tree, divided by the slice's count -- and then a second pass over the same pixels (L2 hits) that adds what the
// first pass's rounding left, sum(a - m0) / count, so a constant channel gets its value back.  The second launch, one workgroup per
// image, folds the slice means in ascending order around the first one, mean = m_0 + sum_s (count_s / P) * (m_s - m_0), writes
// mean[n][:] and computes the J dot products: every thread multiplies its channels in ascending order, a wave adds its 64 lanes by
// the xor butterfly, thread j adds the four waves in order.
//
// No atomics anywhere and a fixed order everywhere: two runs agree bit for bit, and a sample's out, mean and dy do not depend on
// the other samples of the batch.  dW and db add the samples in ascending order, one thread per 4 channels of a row of W.
#include "common.h"

#include <cstdint>

namespace {

constexpr int kThreads = 256;
constexpr int kSlice = 256;             // pixels per slice: T of the tests and of DESIGN.md
constexpr int kMaxC = 1024;
constexpr int kMaxJ = 16;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

struct Geo {
    size_t P;           // pixels per image
    int C, Q, R;        // channels, C / 4, pixel rows per workgroup
    int S;              // slices per image
    int J;
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
    l.p1 = l.p0 + kSlice < g.P ? l.p0 + kSlice : g.P;
    l.base = (size_t)blockIdx.y * g.P * g.C + 4 * l.cg;
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

__device__ __forceinline__ f32x4 act(f32x4 v, int relu) {
    if (relu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.0f);
    }
    return v;
}

// ---- forward 1: the mean of a(y) over one slice -> ws [N][S][C] --------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) pool_slice_kernel(Geo g, const float* __restrict__ y, float* __restrict__ ws, int relu) {
    __shared__ f32x4 sm[kThreads];
    const Lane l = lane_of(g);
    const float cnt = (float)(l.p1 - l.p0);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (l.on)
        for (size_t p = l.p0 + l.row; p < l.p1; p += g.R) s += act(ld4(y + l.base + p * g.C), relu);
    const f32x4 m0 = rows_sum(s, l, g, sm) / cnt;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f};
    if (l.on)
        for (size_t p = l.p0 + l.row; p < l.p1; p += g.R) s1 += act(ld4(y + l.base + p * g.C), relu) - m0;
    s1 = rows_sum(s1, l, g, sm);
    if (l.on && l.row == 0) st4(ws + ((size_t)blockIdx.y * g.S + blockIdx.x) * g.C + 4 * l.cg, m0 + s1 / cnt);
}

// ---- forward 2: the image's mean from its slice means, then the J dot products ---------------------------------------------------
__global__ void __launch_bounds__(kThreads)
pool_fc_kernel(Geo g, const float* __restrict__ ws, const float* __restrict__ W, const float* __restrict__ b, float* __restrict__ out,
               float* __restrict__ mean, float scale) {
    __shared__ float sm_mean[kMaxC];
    __shared__ float sm_dot[kMaxJ][kThreads / dvs::kWave];
    const int t = threadIdx.x, n = blockIdx.x;
    if (t < g.Q) {
        const float* img = ws + (size_t)n * g.S * g.C + 4 * t;
        const float total = (float)g.P;
        const f32x4 m0 = ld4(img);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s = 1; s < g.S; ++s) {
            const size_t q0 = (size_t)s * kSlice;
            const float w = (float)((q0 + kSlice < g.P ? q0 + kSlice : g.P) - q0) / total;
            acc += (ld4(img + (size_t)s * g.C) - m0) * w;
        }
        const f32x4 m = m0 + acc;
        st4(mean + (size_t)n * g.C + 4 * t, m);
#pragma unroll
        for (int k = 0; k < 4; ++k) sm_mean[4 * t + k] = m[k];
    }
    __syncthreads();
    for (int j = 0; j < g.J; ++j) {
        float d = 0.0f;
        for (int c = t; c < g.C; c += kThreads) d = fmaf(W[(size_t)j * g.C + c], sm_mean[c], d);
        d = dvs::wave_sum(d);
        if ((t & (dvs::kWave - 1)) == 0) sm_dot[j][t / dvs::kWave] = d;
    }
    __syncthreads();
    if (t < g.J) {
        float d = sm_dot[t][0];
#pragma unroll
        for (int w = 1; w < kThreads / dvs::kWave; ++w) d += sm_dot[t][w];
        out[(size_t)n * g.J + t] = scale * ((b ? b[t] : 0.0f) + d);
    }
}

// ---- backward 1: dy ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
pool_fc_dy_kernel(Geo g, const float* __restrict__ dout, const float* __restrict__ y, const float* __restrict__ W,
                  float* __restrict__ dy, int relu, float scale) {
    const Lane l = lane_of(g);
    if (!l.on) return;
    f32x4 gv = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < g.J; ++j) gv += ld4(W + (size_t)j * g.C + 4 * l.cg) * dout[(size_t)blockIdx.y * g.J + j];
    gv *= scale / (float)g.P;
    for (size_t p = l.p0 + l.row; p < l.p1; p += g.R) {
        const size_t o = l.base + p * g.C;
        f32x4 v = gv;
        if (relu) {
            const f32x4 yv = ld4(y + o);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = yv[k] > 0.0f ? gv[k] : 0.0f;
        }
        st4(dy + o, v);
    }
}

// ---- backward 2: dW and db, the samples in ascending order ------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
pool_fc_dw_kernel(Geo g, int N, const float* __restrict__ dout, const float* __restrict__ mean, float* __restrict__ dW,
                  float* __restrict__ db, float scale) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= g.J * g.Q) return;
    const int j = i / g.Q, cg = i - j * g.Q;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float sum = 0.0f;
    for (int n = 0; n < N; ++n) {
        const float d = dout[(size_t)n * g.J + j];
        acc += ld4(mean + (size_t)n * g.C + 4 * cg) * d;
        sum += d;
    }
    st4(dW + (size_t)j * g.C + 4 * cg, acc * scale);
    if (db && cg == 0) db[j] = scale * sum;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int make_geo(const char* who, int N, long long P, int C, int J, Geo* g) {
    DVS_REQUIRE(C >= 4 && C <= kMaxC && C % 4 == 0, "%s: C=%d must be a multiple of 4 in 4 .. 1024 (16-byte channel groups)", who, C);
    DVS_REQUIRE(J >= 1 && J <= kMaxJ, "%s: J=%d outputs must be in 1 .. 16", who, J);
    DVS_REQUIRE(N >= 1 && N <= 65535, "%s: N=%d samples must be in 1 .. 65535 (one grid row each)", who, N);
    DVS_REQUIRE(P >= 1, "%s: P=%lld: at least one pixel per sample", who, P);
    DVS_REQUIRE(P <= 0x7fffffffll, "%s: P=%lld pixels per sample exceed 2^31 - 1", who, P);
    DVS_REQUIRE((size_t)N * (size_t)P <= (SIZE_MAX / 16) / (size_t)C, "%s: N*P*C = %d*%lld*%d floats overflow a 64-bit byte offset", who,
                N, P, C);
    g->P = (size_t)P;
    g->C = C;
    g->Q = C / 4;
    g->R = kThreads / g->Q;
    g->S = (int)((P + kSlice - 1) / kSlice);
    g->J = J;
    return DVS_OK;
}

size_t ws_bytes_of(int N, const Geo& g) { return (size_t)N * g.S * g.C * sizeof(float); }

}  // namespace

extern "C" {

int dvs_pool_fc_slice_pixels(void) { return kSlice; }

size_t dvs_pool_fc_workspace(int N, long long P, int C) {
    Geo g;
    if (make_geo("dvs_pool_fc_workspace", N, P, C, 1, &g)) return 0;
    return ws_bytes_of(N, g);
}

int dvs_pool_fc_fwd(const float* y, const float* W, const float* b, float* out, float* mean, void* workspace, size_t workspace_bytes,
                    int N, long long P, int C, int J, int relu, float scale, void* stream) {
    DVS_REQUIRE(y && W && out && mean && workspace, "dvs_pool_fc_fwd: null pointer (y, W, out, mean, workspace)");
    DVS_REQUIRE(aligned16(y) && aligned16(W) && aligned16(b) && aligned16(out) && aligned16(mean) && aligned16(workspace),
                "dvs_pool_fc_fwd: misaligned pointer");
    Geo g;
    if (int rc = make_geo("dvs_pool_fc_fwd", N, P, C, J, &g)) return rc;
    DVS_REQUIRE(workspace_bytes >= ws_bytes_of(N, g), "dvs_pool_fc_fwd: workspace of %zu bytes, dvs_pool_fc_workspace asks for %zu",
                workspace_bytes, ws_bytes_of(N, g));
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(pool_slice_kernel, dim3((unsigned)g.S, (unsigned)N), dim3(kThreads), 0, st, g, y, ws, relu);
    hipLaunchKernelGGL(pool_fc_kernel, dim3((unsigned)N), dim3(kThreads), 0, st, g, ws, W, b, out, mean, scale);
    return dvs::check_launch("dvs_pool_fc_fwd");
}

int dvs_pool_fc_bwd(const float* dout, const float* y, const float* mean, const float* W, float* dy, float* dW, float* db, int N,
                    long long P, int C, int J, int relu, float scale, void* stream) {
    DVS_REQUIRE(dout && y && mean && W && dy && dW, "dvs_pool_fc_bwd: null pointer (dout, y, mean, W, dy, dW)");
    DVS_REQUIRE(aligned16(dout) && aligned16(y) && aligned16(mean) && aligned16(W) && aligned16(dy) && aligned16(dW) && aligned16(db),
                "dvs_pool_fc_bwd: misaligned pointer");
    Geo g;
    if (int rc = make_geo("dvs_pool_fc_bwd", N, P, C, J, &g)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pool_fc_dy_kernel, dim3((unsigned)g.S, (unsigned)N), dim3(kThreads), 0, st, g, dout, y, W, dy, relu, scale);
    hipLaunchKernelGGL(pool_fc_dw_kernel, dim3((unsigned)((g.J * g.Q + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, g, N, dout, mean,
                       dW, db, scale);
    return dvs::check_launch("dvs_pool_fc_bwd");
}

}  // extern "C"
