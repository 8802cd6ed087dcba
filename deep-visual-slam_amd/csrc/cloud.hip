// Output stage of the inference path: world pose bookkeeping and the coloured point cloud, on the device.
//
//   cloud       disparity or depth + image + intrinsics + pose -> 16-byte records {x, y, z, rgb} (the PointCloud2 layout of
//               the ROS2 node's create_pointcloud2, visualizer_node.py:26-56), dense (every kept pixel, visualizer_node.py:
//               152-164, vo/utils/visualization.py:157-193) or compacted by a depth range in row-major order
//               (vo/eval_traj.py:85-121).
//   pose_chain  world <- world . T[b], frame by frame, with left . world and (translation, quaternion) per frame
//               (visualizer_node.py:149,173-190, vo/predict.py:89-90, vo/eval_traj.py:138-147).
//
// A tile is 256 lanes x 4 consecutive kept pixels.  The work is bandwidth bound (16 B read and 16 B written per pixel), so
// the aligned path reads four pixels of every plane with one 16-byte load and every record leaves as one 16-byte store.
// Compaction keeps the pixel order by construction: ballot + popcount of the lower lanes inside a wave, a scan of the four
// wave totals in LDS, per-tile counts in a workspace, an exclusive scan of those by one workgroup per image, and a scatter
// launch that evaluates the same predicate again.  Three plain launches; no workgroup ever waits for another one.
#include "common.h"

namespace {

constexpr int kLanes = 256;                 // workgroup size
constexpr int kPer = 4;                     // kept pixels per lane
constexpr int kTile = kLanes * kPer;        // kept pixels per tile

struct CloudArgs {
    const float* zsrc;      // [B,1,H,W] depth or disparity
    const float* image;     // [B,3,H,W]
    const float* K;         // [B,rs,rs]
    const float* M;         // [B,4,4] or null
    float4* records;        // [B,n_max]
    int* count;             // [B]
    int* index;             // [B,n_max] or null
    int* tiles;             // [B,ntiles] per-tile counts, then exclusive offsets (compact mode)
    int H, W, Wk, sy, sx, n_max, ntiles, rs;     // Wk: kept pixels per row
    int from_disp;
    float da, db;           // depth = 1 / (da + db * disp)
    float z_lo, z_hi;
};

// The one place a depth value is made: the counting and the scattering launch must agree bit for bit, so the
// multiply-add is spelled out instead of being left to contraction.
__device__ __forceinline__ float depth_of(float s, int from_disp, float da, float db) {
    return from_disp ? 1.0f / __builtin_fmaf(db, s, da) : s;
}

__device__ __forceinline__ bool kept(float z, float z_lo, float z_hi) {
    return z_lo < z && (!(z_hi > 0.f) || z < z_hi);
}

// Four consecutive kept pixels k0 .. k0+3 of image b: their source values, linear pixel indices and validity.
template <bool VEC>
__device__ __forceinline__ void load_z(const CloudArgs& a, int b, int k0, float z[kPer], int pix[kPer], bool in[kPer]) {
    const size_t plane = (size_t)a.H * a.W;
    if (VEC) {          // sx == 1, W % 4 == 0, aligned base: k0 % 4 == 0 never straddles a row
        int i = k0 / a.Wk, u = k0 - i * a.Wk;
        int p = i * a.sy * a.W + u;
        bool ok = k0 < a.n_max;
        float4 s = ok ? *reinterpret_cast<const float4*>(a.zsrc + b * plane + p) : make_float4(0.f, 0.f, 0.f, 0.f);
        float sv[kPer] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            in[j] = ok;
            pix[j] = p + j;
            z[j] = depth_of(sv[j], a.from_disp, a.da, a.db);
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            int k = k0 + j;
            in[j] = k < a.n_max;
            int i = k / a.Wk, jj = k - i * a.Wk;
            pix[j] = in[j] ? i * a.sy * a.W + jj * a.sx : 0;
            z[j] = depth_of(in[j] ? a.zsrc[b * plane + pix[j]] : 0.f, a.from_disp, a.da, a.db);
        }
    }
}

__device__ __forceinline__ unsigned to_byte(float c) {
    return (unsigned)fminf(fmaxf(c * 255.0f, 0.0f), 255.0f);       // clamp(0, 255).byte(): truncation
}

// ---- compact mode, launch 1: how many records each tile keeps
template <bool VEC>
__global__ __launch_bounds__(kLanes) void cloud_count_kernel(CloudArgs a) {
    __shared__ int wave_n[kLanes / dvs::kWave];
    const int b = blockIdx.y, tile = blockIdx.x;
    float z[kPer];
    int pix[kPer];
    bool in[kPer];
    load_z<VEC>(a, b, tile * kTile + threadIdx.x * kPer, z, pix, in);
    int n = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) n += __popcll(__ballot(in[j] && kept(z[j], a.z_lo, a.z_hi)));
    if ((threadIdx.x & (dvs::kWave - 1)) == 0) wave_n[threadIdx.x / dvs::kWave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < kLanes / dvs::kWave; ++w) t += wave_n[w];
        a.tiles[b * a.ntiles + tile] = t;
    }
}

// ---- compact mode, launch 2: exclusive scan of the tile counts of one image (in place), total -> count[b]
__global__ __launch_bounds__(kLanes) void cloud_scan_kernel(int* __restrict__ tiles, int* __restrict__ count, int ntiles) {
    __shared__ int part[kLanes];
    int* t = tiles + (size_t)blockIdx.x * ntiles;
    const int per = (ntiles + kLanes - 1) / kLanes;
    const int lo = min((int)threadIdx.x * per, ntiles), hi = min(lo + per, ntiles);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += t[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {                     // 256 adds by one lane: the whole launch is a few microseconds
        int run = 0;
        for (int i = 0; i < kLanes; ++i) {
            int v = part[i];
            part[i] = run;
            run += v;
        }
        count[blockIdx.x] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) {
        int v = t[i];
        t[i] = run;
        run += v;
    }
}

// ---- dense mode (one launch) and compact mode, launch 3
template <bool VEC, bool COMPACT>
__global__ __launch_bounds__(kLanes) void cloud_write_kernel(CloudArgs a) {
    __shared__ int wave_n[kLanes / dvs::kWave];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int k0 = tile * kTile + threadIdx.x * kPer;
    const size_t plane = (size_t)a.H * a.W;
    float z[kPer];
    int pix[kPer];
    bool in[kPer];
    load_z<VEC>(a, b, k0, z, pix, in);

    int slot[kPer];                             // record index of each pixel inside image b
    bool keep[kPer];
    if (COMPACT) {
        const int lane = threadIdx.x & (dvs::kWave - 1), wave = threadIdx.x / dvs::kWave;
        const unsigned long long below = (1ull << lane) - 1ull;
        int before = 0, total = 0, own = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            keep[j] = in[j] && kept(z[j], a.z_lo, a.z_hi);
            unsigned long long m = __ballot(keep[j]);
            before += __popcll(m & below);      // records of the lower lanes: they own earlier pixels
            total += __popcll(m);
            slot[j] = own;                      // records of this lane's earlier pixels
            own += keep[j] ? 1 : 0;
        }
        if (lane == 0) wave_n[wave] = total;
        __syncthreads();
        int base = a.tiles[b * a.ntiles + tile];
#pragma unroll
        for (int w = 0; w < kLanes / dvs::kWave; ++w) base += w < wave ? wave_n[w] : 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) slot[j] += base + before;
    } else {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            keep[j] = in[j];
            slot[j] = k0 + j;
        }
        if (tile == 0 && threadIdx.x == 0) a.count[b] = a.n_max;
    }

    // colours
    unsigned rgb[kPer];
    const float* img = a.image + (size_t)b * 3 * plane;
    if (VEC) {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f), g = r, bl = r;
        if (in[0]) {
            r = *reinterpret_cast<const float4*>(img + pix[0]);
            g = *reinterpret_cast<const float4*>(img + plane + pix[0]);
            bl = *reinterpret_cast<const float4*>(img + 2 * plane + pix[0]);
        }
        float rv[kPer] = {r.x, r.y, r.z, r.w}, gv[kPer] = {g.x, g.y, g.z, g.w}, bv[kPer] = {bl.x, bl.y, bl.z, bl.w};
#pragma unroll
        for (int j = 0; j < kPer; ++j) rgb[j] = (to_byte(rv[j]) << 16) | (to_byte(gv[j]) << 8) | to_byte(bv[j]);
    } else {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            rgb[j] = 0u;
            if (keep[j]) rgb[j] = (to_byte(img[pix[j]]) << 16) | (to_byte(img[plane + pix[j]]) << 8) | to_byte(img[2 * plane + pix[j]]);
        }
    }

    // camera (uniform per image: scalar loads)
    const float* Kb = a.K + (size_t)b * a.rs * a.rs;
    const float fx = Kb[0], cx = Kb[2], fy = Kb[a.rs + 1], cy = Kb[a.rs + 2];
    float m[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    if (a.M) {
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = a.M[b * 16 + i];
    }

    float4* rec = a.records + (size_t)b * a.n_max;
    int* idx = a.index ? a.index + (size_t)b * a.n_max : nullptr;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        if (!keep[j]) continue;
        int v = pix[j] / a.W, u = pix[j] - v * a.W;
        float x = ((float)u - cx) / fx * z[j];
        float y = ((float)v - cy) / fy * z[j];
        float4 o;
        if (a.M) {
            o.x = m[0] * x + m[1] * y + m[2] * z[j] + m[3];
            o.y = m[4] * x + m[5] * y + m[6] * z[j] + m[7];
            o.z = m[8] * x + m[9] * y + m[10] * z[j] + m[11];
        } else {
            o.x = x;
            o.y = y;
            o.z = z[j];
        }
        o.w = __builtin_bit_cast(float, rgb[j]);
        rec[slot[j]] = o;                       // one 16-byte store
        if (idx) idx[slot[j]] = pix[j];
    }
}

// ---- pose chain: one wave, lanes 0..15 own one entry (r, c) of the 4x4 each, serial over the frames
__device__ __forceinline__ float bcast(float v, int lane) { return __shfl(v, lane, dvs::kWave); }

__global__ __launch_bounds__(dvs::kWave) void pose_chain_kernel(const float* __restrict__ T, const float* __restrict__ left,
                                                                float* __restrict__ world, float* __restrict__ poses,
                                                                float* __restrict__ Mout, float* __restrict__ tq, int B) {
    const int lane = threadIdx.x, e = lane & 15, r = e >> 2, c = e & 3;
    float w = world[e];
    const float l = left ? left[e] : 0.f;
    for (int b = 0; b < B; ++b) {
        const float t = T[b * 16 + e];
        float acc = bcast(w, r * 4 + 0) * bcast(t, 0 * 4 + c);
        acc += bcast(w, r * 4 + 1) * bcast(t, 1 * 4 + c);
        acc += bcast(w, r * 4 + 2) * bcast(t, 2 * 4 + c);
        acc += bcast(w, r * 4 + 3) * bcast(t, 3 * 4 + c);
        w = acc;
        if (poses && lane < 16) poses[b * 16 + e] = w;
        if (Mout) {
            float mv = w;
            if (left) {
                mv = bcast(l, r * 4 + 0) * bcast(w, 0 * 4 + c);
                mv += bcast(l, r * 4 + 1) * bcast(w, 1 * 4 + c);
                mv += bcast(l, r * 4 + 2) * bcast(w, 2 * 4 + c);
                mv += bcast(l, r * 4 + 3) * bcast(w, 3 * 4 + c);
            }
            if (lane < 16) Mout[b * 16 + e] = mv;
        }
        if (tq) {
            const float r00 = bcast(w, 0), r01 = bcast(w, 1), r02 = bcast(w, 2), tx = bcast(w, 3);
            const float r10 = bcast(w, 4), r11 = bcast(w, 5), r12 = bcast(w, 6), ty = bcast(w, 7);
            const float r20 = bcast(w, 8), r21 = bcast(w, 9), r22 = bcast(w, 10), tz = bcast(w, 11);
            if (lane == 0) {
                // Shepperd: divide by the largest of |qw|, |qx|, |qy|, |qz| (4 q_i^2 = 1 +- the diagonal entries)
                const float tr = r00 + r11 + r22;
                float qx, qy, qz, qw;
                if (tr >= r00 && tr >= r11 && tr >= r22) {
                    float s = 2.0f * sqrtf(fmaxf(1.0f + tr, 0.f));
                    qw = 0.25f * s;
                    qx = (r21 - r12) / s;
                    qy = (r02 - r20) / s;
                    qz = (r10 - r01) / s;
                } else if (r00 >= r11 && r00 >= r22) {
                    float s = 2.0f * sqrtf(fmaxf(1.0f + r00 - r11 - r22, 0.f));
                    qw = (r21 - r12) / s;
                    qx = 0.25f * s;
                    qy = (r01 + r10) / s;
                    qz = (r02 + r20) / s;
                } else if (r11 >= r22) {
                    float s = 2.0f * sqrtf(fmaxf(1.0f + r11 - r00 - r22, 0.f));
                    qw = (r02 - r20) / s;
                    qx = (r01 + r10) / s;
                    qy = 0.25f * s;
                    qz = (r12 + r21) / s;
                } else {
                    float s = 2.0f * sqrtf(fmaxf(1.0f + r22 - r00 - r11, 0.f));
                    qw = (r10 - r01) / s;
                    qx = (r02 + r20) / s;
                    qy = (r12 + r21) / s;
                    qz = 0.25f * s;
                }
                float n = 1.0f / sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);
                if (qw < 0.f) n = -n;
                float* o = tq + b * 7;
                o[0] = tx;
                o[1] = ty;
                o[2] = tz;
                o[3] = qx * n;
                o[4] = qy * n;
                o[5] = qz * n;
                o[6] = qw * n;
            }
        }
    }
    if (lane < 16) world[e] = w;
}

int check_cfg(const dvs_cloud_cfg* c, const char* who) {
    DVS_REQUIRE(c, "%s: null cfg", who);
    DVS_REQUIRE(c->B > 0 && c->H > 0 && c->W > 0, "%s: B=%d H=%d W=%d", who, c->B, c->H, c->W);
    DVS_REQUIRE(c->stride_y >= 1 && c->stride_x >= 1, "%s: stride %d x %d (must be >= 1)", who, c->stride_y, c->stride_x);
    DVS_REQUIRE(c->k_row_stride == 3 || c->k_row_stride == 4, "%s: k_row_stride=%d (3 or 4)", who, c->k_row_stride);
    DVS_REQUIRE(!c->from_disp || (c->min_depth > 0.f && c->min_depth < c->max_depth),
                "%s: from_disp needs 0 < min_depth < max_depth (got %g, %g)", who, c->min_depth, c->max_depth);
    DVS_REQUIRE((long long)c->B * c->H * c->W < (1ll << 30), "%s: B*H*W too large", who);
    return DVS_OK;
}

inline int kept_h(const dvs_cloud_cfg* c) { return (c->H + c->stride_y - 1) / c->stride_y; }
inline int kept_w(const dvs_cloud_cfg* c) { return (c->W + c->stride_x - 1) / c->stride_x; }

}  // namespace

extern "C" {

int dvs_cloud_capacity(const dvs_cloud_cfg* cfg, int* n_max) {
    if (int rc = check_cfg(cfg, "dvs_cloud_capacity")) return rc;
    DVS_REQUIRE(n_max, "dvs_cloud_capacity: null pointer");
    *n_max = kept_h(cfg) * kept_w(cfg);
    return DVS_OK;
}

size_t dvs_cloud_workspace(const dvs_cloud_cfg* cfg) {
    if (check_cfg(cfg, "dvs_cloud_workspace") != DVS_OK || !cfg->compact) return 0;
    size_t ntiles = ((size_t)kept_h(cfg) * kept_w(cfg) + kTile - 1) / kTile;
    return (ntiles * cfg->B * sizeof(int) + 255) & ~(size_t)255;
}

int dvs_cloud_fwd(const dvs_cloud_cfg* cfg, const float* depth_or_disp, const float* image, const float* K, const float* M,
                  float* records, int* count, int* index, void* workspace, void* stream) {
    if (int rc = check_cfg(cfg, "dvs_cloud_fwd")) return rc;
    DVS_REQUIRE(depth_or_disp && image && K && records && count, "dvs_cloud_fwd: null pointer");
    DVS_REQUIRE(!cfg->compact || workspace, "dvs_cloud_fwd: null workspace in compact mode");
    DVS_REQUIRE(((uintptr_t)records & 15) == 0, "dvs_cloud_fwd: records must be 16-byte aligned");
    DVS_REQUIRE(((uintptr_t)depth_or_disp & 3) == 0 && ((uintptr_t)image & 3) == 0 && ((uintptr_t)K & 3) == 0 &&
                ((uintptr_t)M & 3) == 0 && ((uintptr_t)count & 3) == 0 && ((uintptr_t)index & 3) == 0 &&
                ((uintptr_t)workspace & 3) == 0, "dvs_cloud_fwd: misaligned pointer");
    CloudArgs a;
    a.zsrc = depth_or_disp;
    a.image = image;
    a.K = K;
    a.M = M;
    a.records = reinterpret_cast<float4*>(records);
    a.count = count;
    a.index = index;
    a.tiles = static_cast<int*>(workspace);
    a.H = cfg->H;
    a.W = cfg->W;
    a.sy = cfg->stride_y;
    a.sx = cfg->stride_x;
    a.Wk = kept_w(cfg);
    a.n_max = kept_h(cfg) * a.Wk;
    a.ntiles = (a.n_max + kTile - 1) / kTile;
    a.rs = cfg->k_row_stride;
    a.from_disp = cfg->from_disp ? 1 : 0;
    a.da = a.from_disp ? (float)(1.0 / (double)cfg->max_depth) : 0.f;
    a.db = a.from_disp ? (float)(1.0 / (double)cfg->min_depth - 1.0 / (double)cfg->max_depth) : 0.f;
    a.z_lo = cfg->z_lo;
    a.z_hi = cfg->z_hi;
    // 16-byte loads: four consecutive kept pixels are four consecutive floats of one row, at a 16-byte address
    const bool vec = a.sx == 1 && a.W % 4 == 0 && ((uintptr_t)depth_or_disp & 15) == 0 && ((uintptr_t)image & 15) == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid((unsigned)a.ntiles, (unsigned)cfg->B), block(kLanes);
    if (cfg->compact) {
        if (vec) hipLaunchKernelGGL(cloud_count_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(cloud_count_kernel<false>, grid, block, 0, st, a);
        hipLaunchKernelGGL(cloud_scan_kernel, dim3((unsigned)cfg->B), block, 0, st, a.tiles, count, a.ntiles);
        if (vec) hipLaunchKernelGGL((cloud_write_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((cloud_write_kernel<false, true>), grid, block, 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((cloud_write_kernel<true, false>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((cloud_write_kernel<false, false>), grid, block, 0, st, a);
    }
    return dvs::check_launch("dvs_cloud_fwd");
}

int dvs_pose_chain(const float* T, const float* left, float* world, float* poses, float* M, float* tq, int B, void* stream) {
    DVS_REQUIRE(T && world, "dvs_pose_chain: null pointer");
    DVS_REQUIRE(B > 0, "dvs_pose_chain: B=%d", B);
    hipLaunchKernelGGL(pose_chain_kernel, dim3(1), dim3(dvs::kWave), 0, static_cast<hipStream_t>(stream), T, left, world, poses,
                       M, tq, B);
    return dvs::check_launch("dvs_pose_chain");
}

}  // extern "C"
