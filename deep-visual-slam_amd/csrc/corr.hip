// RAFT correlation block (model/raft/core/corr.py:12-60 + bilinear_sampler, model/raft/core/utils/utils.py:57-71).
//
//   build       all-pairs volume and its average-pool pyramid.  Pooling is linear, so level i = fmap1^T . avgpool_i(fmap2): ONE
//               batched fp32 GEMM on v_mfma_f32_32x32x2_f32 whose B operand is the concatenation [fmap2; pool1; pool2; ...] (the
//               pooled rows come from a small pre-kernel), 1/sqrt(C) in the epilogue.  The big level is written once and never
//               read back to make the coarse ones.
//   lookup      (2r+1)^2 bilinear taps per pixel and level, all levels in one launch.  The taps of one pixel and level share one
//               fractional part, so a workgroup stages the (2r+2)^2 patch of 32 pixels in LDS and blends from there.
//   lookup bwd  row p of the volume belongs to pixel p alone: one thread owns one patch cell and gathers its <= 4 taps of dout,
//               then adds into ONE gradient pyramid (plain read-modify-write, no atomics).
//   volume bwd  dfmap1 = dV . [fmap2; pools] / sqrt(C),  d[fmap2; pools] = dV^T . fmap1 / sqrt(C), then the average-pool backward
//               of the pooled rows is added into dfmap2.
//
//   on the fly  the alternate form (model/raft/core/corr.py:63-91 over model/raft/alt_cuda_corr/correlation_kernel.cu): no volume.
//               The (2r+2)^2 patch that the lookup would load from level i is computed from fmap1 and the rows of
//               [fmap2; pools] instead, then blended as above; its backward sends the patch gradient straight to dfmap1 (one owner
//               per element) and to d[fmap2; pools] (fp32 atomicAdd: many pixels hit the same row).
//
// Layout.  Feature maps are position-major [B][h*w][C] (the memory of a channels_last [B,C,h,w] tensor; contiguous NCHW goes through
// one transposing pass into the workspace).  Level i of the pyramid is a contiguous [B*h*w][h_i*w_i] matrix at float offset
// off_i of one buffer; per-sample bases are 64-bit, offsets inside a sample 32-bit (h*w * h*w < 2^31 is required).
// No float atomics anywhere on the all-pairs path: every output element has one owner and a fixed summation order, so two runs
// agree bit for bit.  The on-the-fly form keeps that for its outputs and for dfmap1; its d[fmap2; pools] is summed with float
// atomics, so dfmap2 of that form differs in the last bits from run to run.
// The process-wide precision mode does not reach these kernels (the reference casts to fp32 at raft.py:82-83).
#include "common.h"

#include <cmath>

namespace {

constexpr int kMaxLevels = 8;
constexpr int kMaxRadius = 8;
constexpr int kPix = 32;            // pixels per lookup workgroup

struct Levels {
    int L, N, Q, C;                 // levels, positions h*w, columns of all levels, channels
    int h[kMaxLevels], w[kMaxLevels], n[kMaxLevels];
    int qs[kMaxLevels + 1];         // first column of level i in the concatenation
    long long off[kMaxLevels];      // float offset of level i in the pyramid buffer
};

// volume: the all-pairs form, whose offsets inside a sample are 32-bit; the on-the-fly form has no buffer of that size
int check_cfg(const dvs_corr_cfg* c, const char* who, bool volume = true) {
    DVS_REQUIRE(c, "%s: null cfg", who);
    DVS_REQUIRE(c->B > 0 && c->C > 0 && c->H > 0 && c->W > 0, "%s: B=%d C=%d H=%d W=%d", who, c->B, c->C, c->H, c->W);
    DVS_REQUIRE(c->C % 4 == 0, "%s: C=%d must be a multiple of 4", who, c->C);
    DVS_REQUIRE(c->num_levels >= 1 && c->num_levels <= kMaxLevels, "%s: num_levels=%d (1..%d)", who, c->num_levels, kMaxLevels);
    DVS_REQUIRE(c->radius >= 0 && c->radius <= kMaxRadius, "%s: radius=%d (0..%d)", who, c->radius, kMaxRadius);
    DVS_REQUIRE((c->H >> (c->num_levels - 1)) >= 2 && (c->W >> (c->num_levels - 1)) >= 2,
                "%s: %dx%d leaves level %d with fewer than 2 rows or columns (the reference divides by W-1: NaN)", who, c->H, c->W,
                c->num_levels - 1);
    DVS_REQUIRE(!volume || (long long)c->H * c->W * c->H * c->W < (1ll << 31), "%s: (H*W)^2 must stay below 2^31", who);
    DVS_REQUIRE((long long)c->B * c->H * c->W * c->C < (1ll << 31), "%s: B*H*W*C must stay below 2^31", who);
    const long long taps = (long long)c->num_levels * (2 * c->radius + 1) * (2 * c->radius + 1);
    DVS_REQUIRE(volume || (long long)c->B * taps * c->H * c->W < (1ll << 31), "%s: B*L*(2r+1)^2*H*W must stay below 2^31", who);
    return DVS_OK;
}

Levels make_levels(const dvs_corr_cfg* c) {
    Levels lv = {};
    lv.L = c->num_levels;
    lv.N = c->H * c->W;
    lv.C = c->C;
    long long off = 0;
    int q = 0;
    for (int i = 0; i < kMaxLevels; ++i) {
        const bool on = i < lv.L;
        lv.h[i] = on ? c->H >> i : 0;
        lv.w[i] = on ? c->W >> i : 0;
        lv.n[i] = lv.h[i] * lv.w[i];
        lv.qs[i] = q;
        lv.off[i] = off;
        q += lv.n[i];
        off += (long long)c->B * lv.N * lv.n[i];
    }
    lv.qs[kMaxLevels] = q;
    lv.Q = q;
    return lv;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// workspace: [pooled fmap2 rows][their gradient][fmap1 position-major, if NCHW][fmap2 position-major, if NCHW]
struct Workspace {
    size_t pool, dpool, t1, t2, total;
};
Workspace make_workspace(const dvs_corr_cfg* c, const Levels& lv) {
    Workspace w;
    const size_t pooled = align256((size_t)c->B * (lv.Q - lv.N) * c->C * sizeof(float));
    const size_t fmap = align256((size_t)c->B * lv.N * c->C * sizeof(float));
    w.pool = 0;
    w.dpool = pooled;
    w.t1 = 2 * pooled;
    w.t2 = w.t1 + (c->fmap1_nchw ? fmap : 0);
    w.total = w.t2 + (c->fmap2_nchw ? fmap : 0);
    if (w.total == 0) w.total = 256;
    return w;
}

// workspace of the on-the-fly form: [fmap1 position-major, if NCHW][fmap2 position-major, if NCHW]
struct AltWorkspace {
    size_t t1, t2, total;
};
AltWorkspace make_alt_workspace(const dvs_corr_cfg* c, const Levels& lv) {
    const size_t fmap = align256((size_t)c->B * lv.N * c->C * sizeof(float));
    AltWorkspace w;
    w.t1 = 0;
    w.t2 = c->fmap1_nchw ? fmap : 0;
    w.total = w.t2 + (c->fmap2_nchw ? fmap : 0);
    if (w.total == 0) w.total = 256;
    return w;
}

// level of column q and what goes with it: constant indices only, so the table stays in scalar registers
struct Col {
    int n, rel;         // columns of the level, column inside it
    long long off;
};
__device__ __forceinline__ Col column(const Levels& lv, int q) {
    Col c = {lv.n[0], q, lv.off[0]};
#pragma unroll
    for (int i = 1; i < kMaxLevels; ++i) {
        if (i < lv.L && q >= lv.qs[i]) {
            c.n = lv.n[i];
            c.rel = q - lv.qs[i];
            c.off = lv.off[i];
        }
    }
    return c;
}

// row q of [fmap2; pools] of sample b (q < Q)
template <typename T>
__device__ __forceinline__ T* cat_row(const Levels& lv, T* f2, T* pool, int b, int q) {
    return q < lv.N ? f2 + ((size_t)b * lv.N + q) * lv.C : pool + ((size_t)b * (lv.Q - lv.N) + (q - lv.N)) * lv.C;
}

// ---- [B][C][N] -> [B][N][C]
__global__ __launch_bounds__(256) void corr_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int N) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* src = in + (size_t)b * C * N;
    float* dst = out + (size_t)b * C * N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c = c0 + ty + 8 * j, n = n0 + tx;
        tile[ty + 8 * j][tx] = (c < C && n < N) ? src[(size_t)c * N + n] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int n = n0 + ty + 8 * j, c = c0 + tx;
        if (n < N && c < C) dst[(size_t)n * C + c] = tile[tx][ty + 8 * j];
    }
}

// ---- pooled rows of fmap2: level i (>= 1) cell (y, x) = mean of the 2^i x 2^i block of level 0 (avg_pool2d(2, 2) i times; the
//      floors at odd sizes only drop trailing rows / columns)
__global__ __launch_bounds__(256) void corr_pool_kernel(Levels lv, const float* __restrict__ f2, float* __restrict__ pool) {
    const int c4n = lv.C / 4, rows = lv.Q - lv.N;
    const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (idx >= rows * c4n) return;
    const int row = idx / c4n, c4 = idx - row * c4n;
    const int q = row + lv.N;
    int lvl = 1;
#pragma unroll
    for (int i = 2; i < kMaxLevels; ++i)
        if (i < lv.L && q >= lv.qs[i]) lvl = i;
    int wl = lv.w[1], qs = lv.qs[1];
#pragma unroll
    for (int i = 2; i < kMaxLevels; ++i)
        if (lvl == i) {
            wl = lv.w[i];
            qs = lv.qs[i];
        }
    const int rel = q - qs, y = rel / wl, x = rel - y * wl, s = 1 << lvl, W = lv.w[0];
    const float4* src = reinterpret_cast<const float4*>(f2 + (size_t)b * lv.N * lv.C) + c4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int dy = 0; dy < s; ++dy)
        for (int dx = 0; dx < s; ++dx) {
            float4 v = src[(size_t)((y * s + dy) * W + x * s + dx) * c4n];
            acc.x += v.x;
            acc.y += v.y;
            acc.z += v.z;
            acc.w += v.w;
        }
    const float k = 1.0f / (float)(s * s);
    reinterpret_cast<float4*>(pool + ((size_t)b * rows + row) * lv.C)[c4] = make_float4(acc.x * k, acc.y * k, acc.z * k, acc.w * k);
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- the volume GEMM: V[b][p][q] = scale * sum_c fmap1[b][p][c] * cat[b][q][c].  128 x 128 tile, four waves of 64 x 64 (2 x 2 MFMA
//      tiles), K in chunks of 32 through LDS.  Both operands are K-contiguous: 16-byte loads and LDS rows of 36 floats.  A lane's
//      four k values of one 16-byte LDS read feed four MFMAs, so the k order of the chain is a fixed permutation of 0 .. C-1.
constexpr int kTM = 128, kTN = 128, kTK = 32, kLd = kTK + 4;

__global__ __launch_bounds__(256) void corr_volume_kernel(Levels lv, const float* __restrict__ f1, const float* __restrict__ f2,
                                                          const float* __restrict__ pool, float* __restrict__ pyr, float scale) {
    __shared__ __attribute__((aligned(16))) float As[kTM * kLd];
    __shared__ __attribute__((aligned(16))) float Bs[kTN * kLd];
    const int b = blockIdx.z, m0 = blockIdx.y * kTM, n0 = blockIdx.x * kTN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int lrow = tid >> 3, lk4 = tid & 7;
    const int C = lv.C;

    const float* arow[4];
    const float* brow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int p = m0 + lrow + 32 * j, q = n0 + lrow + 32 * j;
        arow[j] = p < lv.N ? f1 + ((size_t)b * lv.N + p) * C : nullptr;
        brow[j] = q < lv.Q ? cat_row(lv, f2, pool, b, q) : nullptr;
    }
    float4 ra[4], rb[4];
    auto fetch = [&](int k0) {
        const int k = k0 + lk4 * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ra[j] = (arow[j] && k < C) ? *reinterpret_cast<const float4*>(arow[j] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            rb[j] = (brow[j] && k < C) ? *reinterpret_cast<const float4*>(brow[j] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;

    const int r = lane & 31, hh = lane >> 5;
    fetch(0);
    for (int k0 = 0; k0 < C; k0 += kTK) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<float4*>(&As[(lrow + 32 * j) * kLd + lk4 * 4]) = ra[j];
            *reinterpret_cast<float4*>(&Bs[(lrow + 32 * j) * kLd + lk4 * 4]) = rb[j];
        }
        __syncthreads();
        if (k0 + kTK < C) fetch(k0 + kTK);
#pragma unroll
        for (int s = 0; s < kTK / 8; ++s) {
            float4 a[2], bb[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) a[m] = *reinterpret_cast<const float4*>(&As[(wm * 64 + m * 32 + r) * kLd + 8 * s + 4 * hh]);
#pragma unroll
            for (int n = 0; n < 2; ++n) bb[n] = *reinterpret_cast<const float4*>(&Bs[(wn * 64 + n * 32 + r) * kLd + 8 * s + 4 * hh]);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].x, bb[n].x, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].y, bb[n].y, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].z, bb[n].z, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m].w, bb[n].w, acc[m][n], 0, 0, 0);
                }
        }
    }

    // C/D map: column = lane & 31 (the B row: q), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (the A row: p)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int q = n0 + wn * 64 + n * 32 + r;
        if (q >= lv.Q) continue;
        const Col col = column(lv, q);
        float* base = pyr + col.off + (size_t)b * lv.N * col.n + col.rel;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int p = m0 + wm * 64 + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                if (p < lv.N) base[p * col.n] = acc[m][n][e] * scale;
            }
    }
}

// ---- lookup ---------------------------------------------------------------------------------------------------------------------
// Where pixel p samples level lvl: integer corner and fractional part.  The clamp of non-finite / huge coordinates lives HERE: the
// comparison happens in float BEFORE the float -> int conversion, a NaN compares false, and a pixel that fails it gets a corner
// from which every patch cell is outside the map (exactly what the reference's zero padding returns for it).
struct Anchor {
    int x0, y0;
    float fx, fy;
};
__device__ __forceinline__ Anchor anchor(const float* __restrict__ coords, int b, int p, int N, int lvl, int wl, int hl, int r) {
    Anchor a = {-(3 * r + 4), -(3 * r + 4), 0.f, 0.f};
    if (p >= N) return a;
    const float inv = 1.0f / (float)(1 << lvl);
    const float cx = coords[((size_t)b * 2 + 0) * N + p] * inv, cy = coords[((size_t)b * 2 + 1) * N + p] * inv;
    const bool ok = cx > -(float)(r + 2) && cx < (float)(wl + r + 1) && cy > -(float)(r + 2) && cy < (float)(hl + r + 1);
    if (!ok) return a;
    const float flx = floorf(cx), fly = floorf(cy);
    a.x0 = (int)flx;
    a.y0 = (int)fly;
    a.fx = cx - flx;
    a.fy = cy - fly;
    return a;
}

// patch [kPix][(2r+2)^2 | 1] in LDS -> the (2r+1)^2 taps of every pixel of the tile, channels lvl * (2r+1)^2 + tap of out
template <bool NHWC>
__device__ __forceinline__ void blend_patch(const float* patch, const Anchor* anc, float* __restrict__ out, int b, int p0, int N, int lvl,
                                            int L, int r, int tid) {
    const int S = 2 * r + 2, SSp = (S * S) | 1, T = 2 * r + 1, TT = T * T, CH = L * TT;
    for (int idx = tid; idx < kPix * TT; idx += 256) {
        const int pix = NHWC ? idx / TT : idx % kPix, tap = NHWC ? idx - pix * TT : idx / kPix;
        const int p = p0 + pix;
        if (p >= N) continue;
        const int a = tap / T, bb = tap - a * T;            // a: x offset (the slow index), bb: y offset
        const float fx = anc[pix].fx, fy = anc[pix].fy;
        const float* c = patch + pix * SSp + bb * S + a;
        const float val = c[0] * ((1.f - fx) * (1.f - fy)) + c[1] * (fx * (1.f - fy)) + c[S] * ((1.f - fx) * fy) + c[S + 1] * (fx * fy);
        const int ch = lvl * TT + tap;
        if (NHWC) out[((size_t)b * N + p) * CH + ch] = val;
        else out[((size_t)b * CH + ch) * N + p] = val;
    }
}

// gradient of patch cell (u, v) from the <= 4 taps it is a corner of: cell (u, v) is the corner of tap a = u (weight 1 - fx) and
// of tap a = u - 1 (weight fx); likewise in y.  tap_grad(tap) is dout of tap a * T + bb of this pixel and level.
template <typename F>
__device__ __forceinline__ float cell_gradient(int u, int v, int T, float fx, float fy, F tap_grad) {
    float g = 0.f;
#pragma unroll
    for (int da = 0; da < 2; ++da) {
        const int a = u - da;
        if (a < 0 || a >= T) continue;
        const float wx = da ? fx : 1.f - fx;
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const int bb = v - db;
            if (bb < 0 || bb >= T) continue;
            const float wy = db ? fy : 1.f - fy;
            g += tap_grad(a * T + bb) * (wx * wy);
        }
    }
    return g;
}

template <bool NHWC>
__global__ __launch_bounds__(256) void corr_lookup_fwd_kernel(Levels lv, const float* __restrict__ pyr, const float* __restrict__ coords,
                                                              float* __restrict__ out, int r) {
    extern __shared__ float patch[];            // [kPix][SSp]
    __shared__ Anchor anc[kPix];
    const int lvl = blockIdx.y, b = blockIdx.z, p0 = blockIdx.x * kPix, tid = threadIdx.x;
    const int S = 2 * r + 2, SS = S * S, SSp = SS | 1, N = lv.N;
    int hl = lv.h[0], wl = lv.w[0];
    long long off = lv.off[0];
#pragma unroll
    for (int i = 1; i < kMaxLevels; ++i)
        if (lvl == i) {
            hl = lv.h[i];
            wl = lv.w[i];
            off = lv.off[i];
        }
    const int nl = hl * wl;
    const float* vol = pyr + off + (size_t)b * N * nl;
    if (tid < kPix) anc[tid] = anchor(coords, b, p0 + tid, N, lvl, wl, hl, r);
    __syncthreads();
    for (int idx = tid; idx < kPix * SS; idx += 256) {
        const int pix = idx / SS, cell = idx - pix * SS, v = cell / S, u = cell - v * S;
        const int X = anc[pix].x0 - r + u, Y = anc[pix].y0 - r + v;
        float val = 0.f;
        if (X >= 0 && X < wl && Y >= 0 && Y < hl) val = vol[(p0 + pix) * nl + Y * wl + X];       // (a pixel past N has no cell inside)
        patch[pix * SSp + cell] = val;
    }
    __syncthreads();
    blend_patch<NHWC>(patch, anc, out, b, p0, N, lvl, lv.L, r, tid);
}

template <bool NHWC>
__global__ __launch_bounds__(256) void corr_lookup_bwd_kernel(Levels lv, const float* __restrict__ coords, const float* __restrict__ dout,
                                                              float* __restrict__ dpyr, int r) {
    extern __shared__ float taps[];             // [kPix][TTp]
    __shared__ Anchor anc[kPix];
    const int lvl = blockIdx.y, b = blockIdx.z, p0 = blockIdx.x * kPix, tid = threadIdx.x;
    const int S = 2 * r + 2, SS = S * S, T = 2 * r + 1, TT = T * T, TTp = TT | 1, CH = lv.L * TT, N = lv.N;
    int hl = lv.h[0], wl = lv.w[0];
    long long off = lv.off[0];
#pragma unroll
    for (int i = 1; i < kMaxLevels; ++i)
        if (lvl == i) {
            hl = lv.h[i];
            wl = lv.w[i];
            off = lv.off[i];
        }
    const int nl = hl * wl;
    float* vol = dpyr + off + (size_t)b * N * nl;
    if (tid < kPix) anc[tid] = anchor(coords, b, p0 + tid, N, lvl, wl, hl, r);
    for (int idx = tid; idx < kPix * TT; idx += 256) {
        const int pix = NHWC ? idx / TT : idx % kPix, tap = NHWC ? idx - pix * TT : idx / kPix;
        const int p = p0 + pix, ch = lvl * TT + tap;
        float v = 0.f;
        if (p < N) v = NHWC ? dout[((size_t)b * N + p) * CH + ch] : dout[((size_t)b * CH + ch) * N + p];
        taps[pix * TTp + tap] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < kPix * SS; idx += 256) {
        const int pix = idx / SS, cell = idx - pix * SS, v = cell / S, u = cell - v * S;
        const int X = anc[pix].x0 - r + u, Y = anc[pix].y0 - r + v;
        if (!(X >= 0 && X < wl && Y >= 0 && Y < hl)) continue;
        const float fx = anc[pix].fx, fy = anc[pix].fy;
        const float* t = taps + pix * TTp;
        vol[(p0 + pix) * nl + Y * wl + X] += cell_gradient(u, v, T, fx, fy, [&](int tap) { return t[tap]; });
    }
}

// ---- volume backward: two GEMMs with the gradient pyramid as the A operand.  64 x 64 tile, four waves of one 32 x 32 MFMA tile,
//      K in chunks of 32; the level rows of the pyramid start at any 4-byte address, so the staging loads are scalar and coalesced.
//   MODE 0: dfmap1[b][p][c]   = scale * sum_q G[b][p][q] * cat[b][q][c]       (M = N, K = Q)
//   MODE 1: dcat[b][q][c]     = scale * sum_p G[b][p][q] * fmap1[b][p][c]     (M = Q, K = N); rows q < N go to dfmap2, the rest to dpool
constexpr int kBT = 64, kBK = 32, kBLd = kBK + 1;

template <int MODE>
__global__ __launch_bounds__(256) void corr_volume_bwd_kernel(Levels lv, const float* __restrict__ G, const float* __restrict__ f1,
                                                              const float* __restrict__ f2, const float* __restrict__ pool,
                                                              float* __restrict__ d1, float* __restrict__ d2, float* __restrict__ dpool,
                                                              float scale) {
    __shared__ float As[kBT * kBLd];
    __shared__ float Bs[kBT * kBLd];
    const int b = blockIdx.z, m0 = blockIdx.y * kBT, n0 = blockIdx.x * kBT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int C = lv.C, N = lv.N, Q = lv.Q;
    const int M = MODE == 0 ? N : Q, K = MODE == 0 ? Q : N;

    // A element (m, k).  MODE 0: lanes run along k (= q, contiguous in a level row); MODE 1: along m (= q).
    const int am = MODE == 0 ? tid >> 5 : tid & 63, ak = MODE == 0 ? tid & 31 : tid >> 6;
    const int bn = tid & 63, bk = tid >> 6;                 // B element (n = c, k): lanes along c
    Col mcol = {0, 0, 0};
    if (MODE == 1 && m0 + am < M) mcol = column(lv, m0 + am);

    float ra[8], rb[8];
    auto fetch = [&](int k0) {
        if (MODE == 0) {
            const int q = k0 + ak;
            Col kc = {0, 0, 0};
            if (q < K) kc = column(lv, q);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int p = m0 + am + 8 * j;
                ra[j] = (q < K && p < M) ? G[kc.off + (size_t)b * N * kc.n + p * kc.n + kc.rel] : 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int p = k0 + ak + 4 * j;
                ra[j] = (p < K && m0 + am < M) ? G[mcol.off + (size_t)b * N * mcol.n + p * mcol.n + mcol.rel] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + bk + 4 * j, c = n0 + bn;
            float v = 0.f;
            if (k < K && c < C) v = MODE == 0 ? cat_row(lv, f2, pool, b, k)[c] : f1[((size_t)b * N + k) * C + c];
            rb[j] = v;
        }
    };

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int r = lane & 31, hh = lane >> 5;
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += kBK) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (MODE == 0) As[(am + 8 * j) * kBLd + ak] = ra[j];
            else As[am * kBLd + ak + 4 * j] = ra[j];
            Bs[bn * kBLd + bk + 4 * j] = rb[j];
        }
        __syncthreads();
        if (k0 + kBK < K) fetch(k0 + kBK);
#pragma unroll
        for (int s = 0; s < kBK / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(wm * 32 + r) * kBLd + 2 * s + hh], Bs[(wn * 32 + r) * kBLd + 2 * s + hh], acc, 0,
                                                       0, 0);
    }
    const int c = n0 + wn * 32 + r;
    if (c >= C) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (m >= M) continue;
        const float v = acc[e] * scale;
        if (MODE == 0) d1[((size_t)b * N + m) * C + c] = v;
        else if (m < N) d2[((size_t)b * N + m) * C + c] = v;
        else dpool[((size_t)b * (Q - N) + (m - N)) * C + c] = v;
    }
}

// ---- average-pool backward: dfmap2[b][pos][c] += sum_i dpool_i[b][cell of pos at level i][c] / 4^i (one owner per element)
__global__ __launch_bounds__(256) void corr_unpool_kernel(Levels lv, const float* __restrict__ dpool, float* __restrict__ d2) {
    const int c4n = lv.C / 4, b = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= lv.N * c4n) return;
    const int pos = idx / c4n, c4 = idx - pos * c4n, W = lv.w[0], y = pos / W, x = pos - y * W;
    float4* dst = reinterpret_cast<float4*>(d2 + ((size_t)b * lv.N + pos) * lv.C) + c4;
    float4 acc = *dst;
    const float* src = dpool + (size_t)b * (lv.Q - lv.N) * lv.C;
#pragma unroll
    for (int i = 1; i < kMaxLevels; ++i) {
        if (i >= lv.L) continue;
        const int yy = y >> i, xx = x >> i;
        if (yy >= lv.h[i] || xx >= lv.w[i]) continue;       // the rows / columns an odd size dropped
        const float k = 1.0f / (float)(1 << (2 * i));
        const float4 v = reinterpret_cast<const float4*>(src + (size_t)(lv.qs[i] - lv.N + yy * lv.w[i] + xx) * lv.C)[c4];
        acc.x += v.x * k;
        acc.y += v.y * k;
        acc.z += v.z * k;
        acc.w += v.w * k;
    }
    *dst = acc;
}

// ---- the on-the-fly form ----------------------------------------------------------------------------------------------------------
// s(p, q) = <fmap1[b][p], cat[b][q]> / sqrt(C) for the cells q of level lvl that the lookup of pixel p touches, and nothing else.
constexpr int kAltCK = 64;                  // channels of the tile's fmap1 rows in LDS at a time
constexpr int kAltLd = kAltCK + 4;          // row pitch: 16-byte aligned, and two pixels of one 16-byte read on different banks

struct Level {
    int h, w, qs;                           // rows, columns, first row of the level in [fmap2; pools]
};
__device__ __forceinline__ Level level_of(const Levels& lv, int lvl) {
    Level g = {lv.h[0], lv.w[0], lv.qs[0]};
#pragma unroll
    for (int i = 1; i < kMaxLevels; ++i)
        if (lvl == i) {
            g.h = lv.h[i];
            g.w = lv.w[i];
            g.qs = lv.qs[i];
        }
    return g;
}

// Forward.  The grid of the lookup (32 pixels x level x sample).  The patch [kPix][(2r+2)^2] is accumulated in LDS over channel
// chunks of kAltCK: per chunk the tile's fmap1 rows are staged, then every thread owns patch cells (lanes along the cells of a
// pixel, so the fmap1 reads are broadcasts) and walks the chunk of its row of [fmap2; pools] with 16-byte loads.  A cell outside
// the map is never loaded and stays 0.  Four partial sums per chunk, the chunks in ascending order: one fixed order, so the
// output repeats bit for bit.
template <bool NHWC>
__global__ __launch_bounds__(256) void altcorr_fwd_kernel(Levels lv, const float* __restrict__ f1, const float* __restrict__ f2,
                                                          const float* __restrict__ pool, const float* __restrict__ coords,
                                                          float* __restrict__ out, int r, float scale) {
    extern __shared__ __attribute__((aligned(16))) float alt_lds[];        // [kPix][kAltLd] fmap1 chunk, [kPix][SSp] patch
    __shared__ Anchor anc[kPix];
    float* rows1 = alt_lds;
    float* patch = alt_lds + kPix * kAltLd;
    const int lvl = blockIdx.y, b = blockIdx.z, p0 = blockIdx.x * kPix, tid = threadIdx.x;
    const int S = 2 * r + 2, SS = S * S, SSp = SS | 1, N = lv.N, C = lv.C;
    const Level g = level_of(lv, lvl);
    if (tid < kPix) anc[tid] = anchor(coords, b, p0 + tid, N, lvl, g.w, g.h, r);
    for (int idx = tid; idx < kPix * SSp; idx += 256) patch[idx] = 0.f;
    for (int k0 = 0; k0 < C; k0 += kAltCK) {
        const int ck4 = (C - k0 < kAltCK ? C - k0 : kAltCK) / 4;
        const bool last = k0 + kAltCK >= C;
        __syncthreads();                    // the previous chunk has been read (first pass: anchors and zeros are in place)
        for (int i = tid; i < kPix * ck4; i += 256) {
            const int pix = i / ck4, c4 = i - pix * ck4, p = p0 + pix;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p < N) v = *reinterpret_cast<const float4*>(f1 + ((size_t)b * N + p) * C + k0 + 4 * c4);
            *reinterpret_cast<float4*>(rows1 + pix * kAltLd + 4 * c4) = v;
        }
        __syncthreads();
        for (int idx = tid; idx < kPix * SS; idx += 256) {
            const int pix = idx / SS, cell = idx - pix * SS, v = cell / S, u = cell - v * S;
            const int X = anc[pix].x0 - r + u, Y = anc[pix].y0 - r + v;
            if (!(X >= 0 && X < g.w && Y >= 0 && Y < g.h)) continue;                              // (a pixel past N has no cell inside)
            const float4* a = reinterpret_cast<const float4*>(rows1 + pix * kAltLd);
            const float4* q = reinterpret_cast<const float4*>(cat_row(lv, f2, pool, b, g.qs + Y * g.w + X) + k0);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
            for (int c4 = 0; c4 < ck4; ++c4) {
                const float4 x = a[c4], y = q[c4];
                acc.x = fmaf(x.x, y.x, acc.x);
                acc.y = fmaf(x.y, y.y, acc.y);
                acc.z = fmaf(x.z, y.z, acc.z);
                acc.w = fmaf(x.w, y.w, acc.w);
            }
            const float s = patch[pix * SSp + cell] + ((acc.x + acc.y) + (acc.z + acc.w));
            patch[pix * SSp + cell] = last ? s * scale : s;
        }
    }
    __syncthreads();
    blend_patch<NHWC>(patch, anc, out, b, p0, N, lvl, lv.L, r, tid);
}

// Backward.  One workgroup owns 32 pixels of a sample and walks the levels itself, so dfmap1 has one owner per element and a fixed
// order (bit-reproducible, no atomics): per level the patch gradient g [kPix][(2r+2)^2] is gathered into LDS as the lookup
// backward does, then thread (pixel, channel), lanes along the channels, runs over the cells inside the map:
//     dfmap1[p][c]  += g * cat[q][c] / sqrt(C)          (a register; the level's sum is added to the element by its owner)
//     dcat[q][c]    += g * fmap1[p][c] / sqrt(C)        (fp32 atomicAdd: the windows of many pixels, in many workgroups, share row q)
// dcat -- dfmap2 and the pooled rows' gradient, zeroed by the caller -- therefore depends on the arrival order in its last bits.
template <bool NHWC>
__global__ __launch_bounds__(256) void altcorr_bwd_kernel(Levels lv, const float* __restrict__ f1, const float* __restrict__ f2,
                                                          const float* __restrict__ pool, const float* __restrict__ coords,
                                                          const float* __restrict__ dout, float* __restrict__ d1, float* __restrict__ d2,
                                                          float* __restrict__ dpool, int r, float scale) {
    extern __shared__ float cellg[];            // [kPix][SSp]
    __shared__ Anchor anc[kPix];
    const int b = blockIdx.y, p0 = blockIdx.x * kPix, tid = threadIdx.x;
    const int S = 2 * r + 2, SS = S * S, SSp = SS | 1, T = 2 * r + 1, TT = T * T, CH = lv.L * TT, N = lv.N, C = lv.C;
    for (int lvl = 0; lvl < lv.L; ++lvl) {
        const Level g = level_of(lv, lvl);
        __syncthreads();                        // the previous level's anchors and cells are no longer read
        if (tid < kPix) anc[tid] = anchor(coords, b, p0 + tid, N, lvl, g.w, g.h, r);
        __syncthreads();
        for (int idx = tid; idx < kPix * SS; idx += 256) {
            const int pix = NHWC ? idx / SS : idx % kPix, cell = NHWC ? idx - pix * SS : idx / kPix, v = cell / S, u = cell - v * S;
            const int X = anc[pix].x0 - r + u, Y = anc[pix].y0 - r + v, p = p0 + pix;
            float val = 0.f;
            if (X >= 0 && X < g.w && Y >= 0 && Y < g.h)                                           // (a pixel past N has no cell inside)
                val = cell_gradient(u, v, T, anc[pix].fx, anc[pix].fy, [&](int tap) {
                    const int ch = lvl * TT + tap;
                    return NHWC ? dout[((size_t)b * N + p) * CH + ch] : dout[((size_t)b * CH + ch) * N + p];
                });
            cellg[pix * SSp + cell] = val;
        }
        __syncthreads();
        for (int idx = tid; idx < kPix * C; idx += 256) {
            const int pix = idx / C, c = idx - pix * C, p = p0 + pix;
            if (p >= N) continue;
            const float fs = f1[((size_t)b * N + p) * C + c] * scale;
            const int x0 = anc[pix].x0 - r, y0 = anc[pix].y0 - r;
            float acc = 0.f;
            for (int v = 0; v < S; ++v) {
                const int Y = y0 + v;
                if (Y < 0 || Y >= g.h) continue;
                for (int u = 0; u < S; ++u) {
                    const int X = x0 + u;
                    if (X < 0 || X >= g.w) continue;
                    const int q = g.qs + Y * g.w + X;
                    const float gv = cellg[pix * SSp + v * S + u];
                    acc = fmaf(gv, cat_row(lv, f2, pool, b, q)[c], acc);
                    atomicAdd(cat_row(lv, d2, dpool, b, q) + c, gv * fs);
                }
            }
            float* o = d1 + ((size_t)b * N + p) * C + c;
            *o = lvl ? *o + acc * scale : acc * scale;
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" {

int dvs_corr_sizes(const dvs_corr_cfg* cfg, size_t* pyramid_floats, size_t* level_offsets, size_t* workspace_bytes) {
    if (int rc = check_cfg(cfg, "dvs_corr_sizes")) return rc;
    const Levels lv = make_levels(cfg);
    if (pyramid_floats) *pyramid_floats = (size_t)cfg->B * lv.N * lv.Q;
    if (level_offsets)
        for (int i = 0; i < lv.L; ++i) level_offsets[i] = (size_t)lv.off[i];
    if (workspace_bytes) *workspace_bytes = make_workspace(cfg, lv).total;
    return DVS_OK;
}

int dvs_corr_build(const dvs_corr_cfg* cfg, const float* fmap1, const float* fmap2, float* pyramid, void* workspace, void* stream) {
    if (int rc = check_cfg(cfg, "dvs_corr_build")) return rc;
    DVS_REQUIRE(fmap1 && fmap2 && pyramid && workspace, "dvs_corr_build: null pointer");
    DVS_REQUIRE(aligned16(fmap1) && aligned16(fmap2) && aligned16(workspace) && aligned4(pyramid), "dvs_corr_build: misaligned pointer");
    const Levels lv = make_levels(cfg);
    const Workspace ws = make_workspace(cfg, lv);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(workspace);
    const float* f1 = fmap1;
    const float* f2 = fmap2;
    dim3 tgrid((lv.N + 31) / 32, (cfg->C + 31) / 32, cfg->B);
    if (cfg->fmap1_nchw) {
        hipLaunchKernelGGL(corr_transpose_kernel, tgrid, dim3(256), 0, st, fmap1, reinterpret_cast<float*>(w + ws.t1), cfg->C, lv.N);
        f1 = reinterpret_cast<float*>(w + ws.t1);
    }
    if (cfg->fmap2_nchw) {
        hipLaunchKernelGGL(corr_transpose_kernel, tgrid, dim3(256), 0, st, fmap2, reinterpret_cast<float*>(w + ws.t2), cfg->C, lv.N);
        f2 = reinterpret_cast<float*>(w + ws.t2);
    }
    float* pool = reinterpret_cast<float*>(w + ws.pool);
    if (lv.L > 1) {
        const int work = (lv.Q - lv.N) * (cfg->C / 4);
        hipLaunchKernelGGL(corr_pool_kernel, dim3((work + 255) / 256, cfg->B), dim3(256), 0, st, lv, f2, pool);
    }
    const float scale = (float)(1.0 / std::sqrt((double)cfg->C));
    hipLaunchKernelGGL(corr_volume_kernel, dim3((lv.Q + kTN - 1) / kTN, (lv.N + kTM - 1) / kTM, cfg->B), dim3(256), 0, st, lv, f1, f2,
                       pool, pyramid, scale);
    return dvs::check_launch("dvs_corr_build");
}

int dvs_corr_lookup_fwd(const dvs_corr_cfg* cfg, const float* pyramid, const float* coords, float* out, int out_nhwc, void* stream) {
    if (int rc = check_cfg(cfg, "dvs_corr_lookup_fwd")) return rc;
    DVS_REQUIRE(pyramid && coords && out, "dvs_corr_lookup_fwd: null pointer");
    DVS_REQUIRE(aligned4(pyramid) && aligned4(coords) && aligned4(out), "dvs_corr_lookup_fwd: misaligned pointer");
    const Levels lv = make_levels(cfg);
    const int r = cfg->radius, S = 2 * r + 2;
    const size_t lds = (size_t)kPix * ((S * S) | 1) * sizeof(float);
    dim3 grid((lv.N + kPix - 1) / kPix, lv.L, cfg->B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (out_nhwc) hipLaunchKernelGGL(corr_lookup_fwd_kernel<true>, grid, dim3(256), lds, st, lv, pyramid, coords, out, r);
    else hipLaunchKernelGGL(corr_lookup_fwd_kernel<false>, grid, dim3(256), lds, st, lv, pyramid, coords, out, r);
    return dvs::check_launch("dvs_corr_lookup_fwd");
}

int dvs_corr_lookup_bwd(const dvs_corr_cfg* cfg, const float* coords, const float* dout, int dout_nhwc, float* dpyramid, void* stream) {
    if (int rc = check_cfg(cfg, "dvs_corr_lookup_bwd")) return rc;
    DVS_REQUIRE(coords && dout && dpyramid, "dvs_corr_lookup_bwd: null pointer");
    DVS_REQUIRE(aligned4(dpyramid) && aligned4(coords) && aligned4(dout), "dvs_corr_lookup_bwd: misaligned pointer");
    const Levels lv = make_levels(cfg);
    const int r = cfg->radius, T = 2 * r + 1;
    const size_t lds = (size_t)kPix * ((T * T) | 1) * sizeof(float);
    dim3 grid((lv.N + kPix - 1) / kPix, lv.L, cfg->B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dout_nhwc) hipLaunchKernelGGL(corr_lookup_bwd_kernel<true>, grid, dim3(256), lds, st, lv, coords, dout, dpyramid, r);
    else hipLaunchKernelGGL(corr_lookup_bwd_kernel<false>, grid, dim3(256), lds, st, lv, coords, dout, dpyramid, r);
    return dvs::check_launch("dvs_corr_lookup_bwd");
}

int dvs_corr_volume_bwd(const dvs_corr_cfg* cfg, const float* dpyramid, const float* fmap1, const float* fmap2, void* workspace,
                        float* dfmap1, float* dfmap2, void* stream) {
    if (int rc = check_cfg(cfg, "dvs_corr_volume_bwd")) return rc;
    DVS_REQUIRE(dpyramid && fmap1 && fmap2 && workspace && dfmap1 && dfmap2, "dvs_corr_volume_bwd: null pointer");
    DVS_REQUIRE(aligned16(fmap1) && aligned16(fmap2) && aligned16(workspace) && aligned16(dfmap1) && aligned16(dfmap2) &&
                aligned4(dpyramid), "dvs_corr_volume_bwd: misaligned pointer");
    const Levels lv = make_levels(cfg);
    const Workspace ws = make_workspace(cfg, lv);
    char* w = static_cast<char*>(workspace);
    const float* f1 = cfg->fmap1_nchw ? reinterpret_cast<const float*>(w + ws.t1) : fmap1;
    const float* f2 = cfg->fmap2_nchw ? reinterpret_cast<const float*>(w + ws.t2) : fmap2;
    const float* pool = reinterpret_cast<const float*>(w + ws.pool);
    float* dpool = reinterpret_cast<float*>(w + ws.dpool);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float scale = (float)(1.0 / std::sqrt((double)cfg->C));
    const unsigned cn = (cfg->C + kBT - 1) / kBT;
    hipLaunchKernelGGL(corr_volume_bwd_kernel<0>, dim3(cn, (lv.N + kBT - 1) / kBT, cfg->B), dim3(256), 0, st, lv, dpyramid, f1, f2, pool,
                       dfmap1, dfmap2, dpool, scale);
    hipLaunchKernelGGL(corr_volume_bwd_kernel<1>, dim3(cn, (lv.Q + kBT - 1) / kBT, cfg->B), dim3(256), 0, st, lv, dpyramid, f1, f2, pool,
                       dfmap1, dfmap2, dpool, scale);
    if (lv.L > 1) {
        const int work = lv.N * (cfg->C / 4);
        hipLaunchKernelGGL(corr_unpool_kernel, dim3((work + 255) / 256, cfg->B), dim3(256), 0, st, lv, dpool, dfmap2);
    }
    return dvs::check_launch("dvs_corr_volume_bwd");
}

// ---- the on-the-fly form
int dvs_altcorr_sizes(const dvs_corr_cfg* cfg, size_t* pooled_floats, size_t* workspace_bytes) {
    if (int rc = check_cfg(cfg, "dvs_altcorr_sizes", false)) return rc;
    const Levels lv = make_levels(cfg);
    const size_t pooled = (size_t)cfg->B * (lv.Q - lv.N) * cfg->C;
    if (pooled_floats) *pooled_floats = pooled ? pooled : 4;            // one level: nothing is pooled, the buffer keeps an address
    if (workspace_bytes) *workspace_bytes = make_alt_workspace(cfg, lv).total;
    return DVS_OK;
}

int dvs_altcorr_pool(const dvs_corr_cfg* cfg, const float* fmap1, const float* fmap2, float* pooled, void* workspace, void* stream) {
    if (int rc = check_cfg(cfg, "dvs_altcorr_pool", false)) return rc;
    DVS_REQUIRE(fmap1 && fmap2 && pooled && workspace, "dvs_altcorr_pool: null pointer");
    DVS_REQUIRE(aligned16(fmap1) && aligned16(fmap2) && aligned16(pooled) && aligned16(workspace), "dvs_altcorr_pool: misaligned pointer");
    const Levels lv = make_levels(cfg);
    const AltWorkspace ws = make_alt_workspace(cfg, lv);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(workspace);
    const float* f2 = fmap2;
    dim3 tgrid((lv.N + 31) / 32, (cfg->C + 31) / 32, cfg->B);
    if (cfg->fmap1_nchw)
        hipLaunchKernelGGL(corr_transpose_kernel, tgrid, dim3(256), 0, st, fmap1, reinterpret_cast<float*>(w + ws.t1), cfg->C, lv.N);
    if (cfg->fmap2_nchw) {
        hipLaunchKernelGGL(corr_transpose_kernel, tgrid, dim3(256), 0, st, fmap2, reinterpret_cast<float*>(w + ws.t2), cfg->C, lv.N);
        f2 = reinterpret_cast<float*>(w + ws.t2);
    }
    if (lv.L > 1) {
        const int work = (lv.Q - lv.N) * (cfg->C / 4);
        hipLaunchKernelGGL(corr_pool_kernel, dim3((work + 255) / 256, cfg->B), dim3(256), 0, st, lv, f2, pooled);
    }
    return dvs::check_launch("dvs_altcorr_pool");
}

int dvs_altcorr_fwd(const dvs_corr_cfg* cfg, const float* fmap1, const float* fmap2, const float* pooled, const void* workspace,
                    const float* coords, float* out, int out_nhwc, void* stream) {
    if (int rc = check_cfg(cfg, "dvs_altcorr_fwd", false)) return rc;
    DVS_REQUIRE(fmap1 && fmap2 && pooled && workspace && coords && out, "dvs_altcorr_fwd: null pointer");
    DVS_REQUIRE(aligned16(fmap1) && aligned16(fmap2) && aligned16(pooled) && aligned16(workspace) && aligned4(coords) && aligned4(out),
                "dvs_altcorr_fwd: misaligned pointer");
    const Levels lv = make_levels(cfg);
    const AltWorkspace ws = make_alt_workspace(cfg, lv);
    const char* w = static_cast<const char*>(workspace);
    const float* f1 = cfg->fmap1_nchw ? reinterpret_cast<const float*>(w + ws.t1) : fmap1;
    const float* f2 = cfg->fmap2_nchw ? reinterpret_cast<const float*>(w + ws.t2) : fmap2;
    const int r = cfg->radius, S = 2 * r + 2;
    const size_t lds = (size_t)kPix * (kAltLd + ((S * S) | 1)) * sizeof(float);
    const float scale = (float)(1.0 / std::sqrt((double)cfg->C));
    dim3 grid((lv.N + kPix - 1) / kPix, lv.L, cfg->B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (out_nhwc) hipLaunchKernelGGL(altcorr_fwd_kernel<true>, grid, dim3(256), lds, st, lv, f1, f2, pooled, coords, out, r, scale);
    else hipLaunchKernelGGL(altcorr_fwd_kernel<false>, grid, dim3(256), lds, st, lv, f1, f2, pooled, coords, out, r, scale);
    return dvs::check_launch("dvs_altcorr_fwd");
}

int dvs_altcorr_bwd(const dvs_corr_cfg* cfg, const float* fmap1, const float* fmap2, const float* pooled, const void* workspace,
                    const float* coords, const float* dout, int dout_nhwc, float* dfmap1, float* dfmap2, float* dpooled, void* stream) {
    if (int rc = check_cfg(cfg, "dvs_altcorr_bwd", false)) return rc;
    DVS_REQUIRE(fmap1 && fmap2 && pooled && workspace && coords && dout && dfmap1 && dfmap2 && dpooled, "dvs_altcorr_bwd: null pointer");
    DVS_REQUIRE(aligned16(fmap1) && aligned16(fmap2) && aligned16(pooled) && aligned16(workspace) && aligned4(coords) && aligned4(dout) &&
                aligned16(dfmap1) && aligned16(dfmap2) && aligned16(dpooled), "dvs_altcorr_bwd: misaligned pointer");
    const Levels lv = make_levels(cfg);
    const AltWorkspace ws = make_alt_workspace(cfg, lv);
    const char* w = static_cast<const char*>(workspace);
    const float* f1 = cfg->fmap1_nchw ? reinterpret_cast<const float*>(w + ws.t1) : fmap1;
    const float* f2 = cfg->fmap2_nchw ? reinterpret_cast<const float*>(w + ws.t2) : fmap2;
    const int r = cfg->radius, S = 2 * r + 2;
    const size_t lds = (size_t)kPix * ((S * S) | 1) * sizeof(float);
    const float scale = (float)(1.0 / std::sqrt((double)cfg->C));
    dim3 grid((lv.N + kPix - 1) / kPix, cfg->B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dout_nhwc)
        hipLaunchKernelGGL(altcorr_bwd_kernel<true>, grid, dim3(256), lds, st, lv, f1, f2, pooled, coords, dout, dfmap1, dfmap2, dpooled, r,
                           scale);
    else
        hipLaunchKernelGGL(altcorr_bwd_kernel<false>, grid, dim3(256), lds, st, lv, f1, f2, pooled, coords, dout, dfmap1, dfmap2, dpooled, r,
                           scale);
    return dvs::check_launch("dvs_altcorr_bwd");
}

int dvs_altcorr_unpool(const dvs_corr_cfg* cfg, const float* dpooled, float* dfmap2, void* stream) {
    if (int rc = check_cfg(cfg, "dvs_altcorr_unpool", false)) return rc;
    DVS_REQUIRE(dpooled && dfmap2, "dvs_altcorr_unpool: null pointer");
    DVS_REQUIRE(aligned16(dpooled) && aligned16(dfmap2), "dvs_altcorr_unpool: misaligned pointer");
    const Levels lv = make_levels(cfg);
    if (lv.L > 1) {
        const int work = lv.N * (cfg->C / 4);
        hipLaunchKernelGGL(corr_unpool_kernel, dim3((work + 255) / 256, cfg->B), dim3(256), 0, static_cast<hipStream_t>(stream), lv, dpooled, dfmap2);
    }
    return dvs::check_launch("dvs_altcorr_unpool");
}

}  // extern "C"
