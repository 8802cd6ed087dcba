// Camera pose from a measured flow and the depth of its source frame: the inverse of rigidflow.hip.  A dense reprojection-error
// Gauss-Newton fit on SE(3) with Huber weights, the per-pair form of what the reference's back end does on the CPU with g2o
// (slam/optimizer.py:222-319, EdgeProjectD3VO under RobustKernelHuber).
//
//   dvs_pose_fit_workspace   bytes of partial sums the fit needs for (N, H, W)
//   dvs_pose_fit             `iters` pairs of (accumulate, update), and one more accumulate whose sums are handed out
//
// ACCUMULATE (one launch for all N images).  Per pixel (x, y), d = depth, (fu, fv) = flow, iK = inv_K, fp32, every operation
// rounded on its own (contraction is off for the whole file):
//
//   (X, Y, Z) = d * (rx, ry, rz)                             the ray of pixelfield.h, as dvs_rigid_flow
//   qx = ((T[0][0]*X + T[0][1]*Y) + T[0][2]*Z) + T[0][3]     qy, qz: rows 1, 2
//   cx = ((K[0][0]*qx + K[0][1]*qy) + K[0][2]*qz) + K[0][3]  cy, cz: rows 1, 2
//   den = cz + eps;  px = cx / den, py = cy / den            the correctly rounded quotient
//   tx = x + fu, ty = y + fv                                 the measured target
//   ex = px - tx, ey = py - ty                               the residual
//   judged = d finite and > 0, fu and fv finite, valid absent or non-zero, cz > 0, 0 <= tx <= W-1, 0 <= ty <= H-1, ex and ey finite
//   e2 = ex*ex + ey*ey;  w = 1 if e2 <= huber*huber, else huber / sqrt(e2)            sqrt and quotient correctly rounded
//   A[r][k] = (K[r][k] - p_r*K[2][k]) / den                  r = 0, 1 (p_0 = px, p_1 = py), k = 0, 1, 2
//   J[r] = (A[r][0], A[r][1], A[r][2], A[r][2]*qy - A[r][1]*qz, A[r][0]*qz - A[r][2]*qx, A[r][1]*qx - A[r][0]*qy)
//
// J is the derivative of (px, py) for a left perturbation T <- exp(xi) T, xi = (nu, omega), translation first.  A judged pixel
// gives one fp32 TERM to each of 30 sums, which is widened and added in fp64:
//
//   sum[idx(i, j)] += w * (J[0][i]*J[0][j] + J[1][i]*J[1][j])      0 <= i <= j < 6, idx row-major over the upper triangle: 0 .. 20
//   sum[21 + i]    += w * (J[0][i]*ex + J[1][i]*ey)                i < 6
//   sum[27] += w * e2;   sum[28] += w;   sum[29] += 1
//
// A lane owns four consecutive pixels of a row (pixelfield.h: its lane geometry, its views, its vector or scalar loads) and
// walks the image with a grid stride; the number of workgroups per image depends on (H, W) alone.  30 fp64 accumulators a lane,
// a 64-lane butterfly of shuffles, the four waves through LDS, and ONE row of 30 doubles per workgroup into the workspace.
// There are no atomics and no memset: the sums repeat bit for bit and an image's sums do not depend on the rest of the batch.
//
// UPDATE (one launch, one workgroup per image, fp64): the rows of an image are staged in LDS by independent loads (a chain of
// dependent global loads, one per row, was the larger part of an iteration), added in row order by lanes 0 .. 29, then by lane 0
//
//   A = H + damping * diag(H);  A = L L^T (Cholesky);  L y = -g, L^T xi = y
//   theta^2 = |omega|^2, W = [omega]x:  R = I + a W + b W^2, V = I + b W + c W^2, t = V nu
//     a = sin(theta) / theta, b = (1 - cos(theta)) / theta^2, c = (theta - sin(theta)) / theta^3
//     theta^2 < 1e-4:  a = 1 - theta^2/6 + theta^4/120, b = 1/2 - theta^2/24 + theta^4/720, c = 1/6 - theta^2/120 + theta^4/5040
//   T <- [R t; 0 1] T, rounded to fp32
//
// The step is skipped -- T keeps its bits for this and every later iteration, status = 1 -- when fewer than 6 pixels were judged,
// a sum, xi or the new T is not finite, or a pivot is not positive.
#include "pixelfield.h"

#pragma clang fp contract(off)

namespace {

using namespace dvs;
constexpr int kThreads = kPixThreads;
constexpr int kSums = 30;                           // 21 of J^T J, 6 of J^T e, the cost, the weights, the count
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxGroups = 256;                     // workgroups per image at the most: rows the update adds one after another

struct Args {
    Plane depth;
    const float *K, *iK, *T;                        // dense [N][4][4]
    Field flow;
    const unsigned char* valid;                     // dense [N][H][W], may be null
    double* partial;                                // [N][groups][kSums]
    int H, W;
    int quads;                                      // ceil(W / kPix): lanes per row
    unsigned lanes;                                 // H * quads
    float huber, eps;
};

struct Camera {
    float K[3][4], T[3][4], iK[3][3];
};

__device__ __forceinline__ Camera camera_of(const Args& s, int n) {
    const float* __restrict__ K = s.K + (size_t)n * 16;
    const float* __restrict__ T = s.T + (size_t)n * 16;
    Camera c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) c.K[i][j] = K[4 * i + j], c.T[i][j] = T[4 * i + j];
    load_inv_K(s.iK + (size_t)n * 16, c.iK);
    return c;
}

// the 30 terms of one pixel, added to acc where the pixel is judged
__device__ __forceinline__ void pixel(const Camera& c, int xi, int yi, float d, float fu, float fv, bool ok, int H, int W, float eps,
                                      float huber, float huber2, double (&acc)[kSums]) {
    const float x = (float)xi, y = (float)yi;
    float X, Y, Z;
    back_project(c.iK, x, y, d, &X, &Y, &Z);
    const float qx = ((c.T[0][0] * X + c.T[0][1] * Y) + c.T[0][2] * Z) + c.T[0][3];
    const float qy = ((c.T[1][0] * X + c.T[1][1] * Y) + c.T[1][2] * Z) + c.T[1][3];
    const float qz = ((c.T[2][0] * X + c.T[2][1] * Y) + c.T[2][2] * Z) + c.T[2][3];
    const float cx = ((c.K[0][0] * qx + c.K[0][1] * qy) + c.K[0][2] * qz) + c.K[0][3];
    const float cy = ((c.K[1][0] * qx + c.K[1][1] * qy) + c.K[1][2] * qz) + c.K[1][3];
    const float cz = ((c.K[2][0] * qx + c.K[2][1] * qy) + c.K[2][2] * qz) + c.K[2][3];
    const float den = cz + eps;
    const float px = cx / den, py = cy / den;
    const float tx = x + fu, ty = y + fv;
    const float ex = px - tx, ey = py - ty;
    const bool judged = ok && __builtin_isfinite(d) && d > 0.0f && __builtin_isfinite(fu) && __builtin_isfinite(fv) && cz > 0.0f &&
                        tx >= 0.0f && tx <= (float)(W - 1) && ty >= 0.0f && ty <= (float)(H - 1) && __builtin_isfinite(ex) &&
                        __builtin_isfinite(ey);
    if (!judged) return;
    const float e2 = ex * ex + ey * ey;
    const float w = e2 <= huber2 ? 1.0f : huber / __builtin_sqrtf(e2);
    float J[2][6];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float p = r ? py : px;
        const float a0 = (c.K[r][0] - p * c.K[2][0]) / den;
        const float a1 = (c.K[r][1] - p * c.K[2][1]) / den;
        const float a2 = (c.K[r][2] - p * c.K[2][2]) / den;
        J[r][0] = a0, J[r][1] = a1, J[r][2] = a2;
        J[r][3] = a2 * qy - a1 * qz;
        J[r][4] = a0 * qz - a2 * qx;
        J[r][5] = a1 * qx - a0 * qy;
    }
    int idx = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) acc[idx++] += (double)(w * (J[0][i] * J[0][j] + J[1][i] * J[1][j]));
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += (double)(w * (J[0][i] * ex + J[1][i] * ey));
    acc[27] += (double)(w * e2);
    acc[28] += (double)w;
    acc[29] += 1.0;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) pose_fit_accumulate(Args s) {
    __shared__ double part[kWaves][kSums];
    const int n = blockIdx.y;
    const Camera cam = camera_of(s, n);
    const float huber2 = s.huber * s.huber;
    double acc[kSums];
#pragma unroll
    for (int i = 0; i < kSums; ++i) acc[i] = 0.0;
    const unsigned stride = gridDim.x * kThreads;                     // host: lanes < 2^31 - kThreads, stride <= 2^16
    for (unsigned g = blockIdx.x * kThreads + threadIdx.x; g < s.lanes; g += stride) {
        unsigned y;
        int x;
        lane_pixels(g, s.quads, &y, &x);
        const int count = s.W - x;
        const float* fp = at(s.flow, n, y, x);
        const size_t o = ((size_t)n * (size_t)s.H + y) * (size_t)s.W + x;             // of the dense valid [N][H][W]
        float d[kPix], fu[kPix], fv[kPix];
        load_quad<VEC>(at(s.depth, n, y, x), count, d);
        load_quad<VEC>(fp, count, fu);
        load_quad<VEC>(fp + s.flow.plane, count, fv);
        const unsigned ok = load_mask<VEC>(s.valid ? s.valid + o : nullptr, count);
#pragma unroll
        for (int k = 0; k < kPix; ++k)
            pixel(cam, x + k, (int)y, d[k], fu[k], fv[k], (ok >> (8 * k) & 255u) != 0, s.H, s.W, s.eps, s.huber, huber2, acc);
    }
#pragma unroll
    for (int i = 0; i < kSums; ++i) acc[i] = wave_sum(acc[i]);
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) {
#pragma unroll
        for (int i = 0; i < kSums; ++i) part[wave][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        double v = part[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < kWaves; ++k) v += part[k][threadIdx.x];
        s.partial[((size_t)n * gridDim.x + blockIdx.x) * kSums + threadIdx.x] = v;
    }
}

// ---- the update -------------------------------------------------------------------------------------------------------------------
struct Step {
    const double* partial;                          // [N][groups][kSums]; null: nothing is summed (the copy of T0 alone)
    int groups;
    const float* Tin;                               // T0 in the first launch of a call, T afterwards
    float* Tout;
    int* status;
    double* normal;                                 // [N][kSums] or null: the ordered sums, handed out
    int solve;                                      // 0: sum (and hand out) only
    int first;                                      // the first launch of a call: status starts at 0, whatever the buffer holds
    double damping;
};

__device__ __forceinline__ bool finite(double v) { return __builtin_isfinite(v); }

// one Gauss-Newton step from the 30 sums; T (row-major 4x4, fp32) is replaced where the step is taken.  False: T is untouched.
__device__ bool gauss_newton_step(const double* s, float* T, double damping) {
    if (!(s[kSums - 1] >= 6.0)) return false;
#pragma unroll
    for (int i = 0; i < kSums; ++i)
        if (!finite(s[i])) return false;
    double A[6][6], L[6][6];
    int idx = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = s[idx++];
#pragma unroll
    for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + damping * A[i][i];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double p = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) p = p - L[j][k] * L[j][k];
        if (!(p > 0.0)) return false;
        L[j][j] = sqrt(p);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double yv[6], xi[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -s[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * yv[k];
        yv[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = yv[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * xi[k];
        xi[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (!finite(xi[i])) return false;
    const double wx = xi[3], wy = xi[4], wz = xi[5];
    const double th2 = (wx * wx + wy * wy) + wz * wz;
    double a, b, c;
    if (th2 < 1e-4) {
        const double th4 = th2 * th2;
        a = (1.0 - th2 / 6.0) + th4 / 120.0;
        b = (0.5 - th2 / 24.0) + th4 / 720.0;
        c = (1.0 / 6.0 - th2 / 120.0) + th4 / 5040.0;
    } else {
        const double th = sqrt(th2);
        const double sn = sin(th), cs = cos(th);
        a = sn / th;
        b = (1.0 - cs) / th2;
        c = (th - sn) / (th2 * th);
    }
    const double Wm[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
    double W2[3][3], E[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W2[i][j] = (Wm[i][0] * Wm[0][j] + Wm[i][1] * Wm[1][j]) + Wm[i][2] * Wm[2][j];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double V[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double id = i == j ? 1.0 : 0.0;
            E[i][j] = (id + a * Wm[i][j]) + b * W2[i][j];
            V[j] = (id + b * Wm[i][j]) + c * W2[i][j];
        }
        E[i][3] = (V[0] * xi[0] + V[1] * xi[1]) + V[2] * xi[2];
    }
    float out[12];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double v = ((E[i][0] * (double)T[j] + E[i][1] * (double)T[4 + j]) + E[i][2] * (double)T[8 + j]) + E[i][3] * (double)T[12 + j];
            out[4 * i + j] = (float)v;
            if (!__builtin_isfinite(out[4 * i + j])) return false;
        }
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = out[i];                       // the bottom row is T's own: [R t; 0 1] leaves it
    return true;
}

__global__ void __launch_bounds__(kThreads) pose_fit_update(Step u) {
    __shared__ double rows[kMaxGroups * kSums];     // the image's rows, staged by independent loads: 60 KB
    __shared__ double sum[kSums];
    const int n = blockIdx.x;
    if (u.partial) {
        const double* p = u.partial + (size_t)n * u.groups * kSums;
        for (int i = threadIdx.x; i < u.groups * kSums; i += kThreads) rows[i] = p[i];
    }
    __syncthreads();
    if (u.partial && threadIdx.x < kSums) {
        double v = rows[threadIdx.x];
        for (int r = 1; r < u.groups; ++r) v += rows[r * kSums + threadIdx.x];  // in row order
        sum[threadIdx.x] = v;
        if (u.normal) u.normal[(size_t)n * kSums + threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = u.Tin[(size_t)n * 16 + i];
    int st = u.first ? 0 : u.status[n];
    if (u.solve && st == 0) st = gauss_newton_step(sum, T, u.damping) ? 0 : 1;
#pragma unroll
    for (int i = 0; i < 16; ++i) u.Tout[(size_t)n * 16 + i] = T[i];
    u.status[n] = st;
}

// workgroups per image: every workgroup walks the same number of strides, and (H, W) alone decide
int groups_of(int H, int quads) {
    const long long blocks = ((long long)H * quads + kThreads - 1) / kThreads;
    const long long walks = (blocks + kMaxGroups - 1) / kMaxGroups;
    return (int)((blocks + walks - 1) / walks);
}

}  // namespace

extern "C" {

size_t dvs_pose_fit_workspace(int N, int H, int W) {
    const int quads = quads_of(N, H, W);
    return quads ? (size_t)N * (size_t)groups_of(H, quads) * kSums * sizeof(double) : 0;
}

int dvs_pose_fit(const float* depth, long long depth_image_stride, long long depth_row_stride, const float* K, const float* inv_K,
                 const float* T0, const float* flow, long long flow_image_stride, long long flow_plane_stride, long long flow_row_stride,
                 const unsigned char* valid, float* T, int* status, double* normal, void* workspace, size_t workspace_bytes, int N, int H,
                 int W, int iters, float huber, float damping, float eps, void* stream) {
    const char* who = "dvs_pose_fit";
    Args s;
    if (int rc = check_shape(who, N, H, W, &s.quads)) return rc;
    s.depth = Plane{depth, depth_image_stride, depth_row_stride};
    s.flow = Field{flow, flow_image_stride, flow_plane_stride, flow_row_stride};
    if (int rc = check_plane(who, "depth", s.depth, H, W)) return rc;
    if (int rc = check_floats(who, "K", K)) return rc;
    if (int rc = check_floats(who, "inv_K", inv_K)) return rc;
    if (int rc = check_floats(who, "T0", T0)) return rc;
    if (int rc = check_field(who, "flow", s.flow, H, W)) return rc;
    DVS_REQUIRE(T && status && workspace, "dvs_pose_fit: null pointer (T, status or workspace)");
    DVS_REQUIRE(aligned(T, 4) && aligned(status, 4) && aligned(normal, 8) && aligned(workspace, 8),
                "dvs_pose_fit: misaligned pointer (T, status, normal or workspace)");
    DVS_REQUIRE(iters >= 0 && iters <= 64, "dvs_pose_fit: iters=%d must be in 0 .. 64", iters);
    DVS_REQUIRE(huber > 0.0f, "dvs_pose_fit: huber=%g must be above 0 (+inf: plain least squares)", (double)huber);
    DVS_REQUIRE(finite_nonneg(damping) && finite_nonneg(eps), "dvs_pose_fit: damping=%g, eps=%g must be finite and not negative",
                (double)damping, (double)eps);
    const int groups = groups_of(H, s.quads);
    const size_t need = (size_t)N * (size_t)groups * kSums * sizeof(double);
    DVS_REQUIRE(workspace_bytes >= need, "dvs_pose_fit: workspace of %zu bytes is below dvs_pose_fit_workspace = %zu", workspace_bytes, need);
    const long long pixels = (long long)N * H * W;
    // T may be exactly T0 (fitted in place): T0 then stands for no range of its own, and the other outputs are held against T
    const Span ins[] = {span("depth", s.depth, N, H, W), span("K", K, 64ll * N), span("inv_K", inv_K, 64ll * N),
                        span("T0", T == T0 ? nullptr : T0, 64ll * N), span("flow", s.flow, N, H, W), span("valid", valid, pixels)};
    const Span outs[] = {span("T", T, 64ll * N), span("status", status, 4ll * N), span("normal", normal, 8ll * kSums * N),
                         span("workspace", workspace, (long long)need)};
    if (int rc = check_overlap(who, outs, ins, "input")) return rc;
    if (int rc = check_overlap(who, outs, outs, "output")) return rc;
    s.K = K, s.iK = inv_K, s.T = T0;
    s.valid = valid, s.partial = static_cast<double*>(workspace);
    s.H = H, s.W = W, s.lanes = (unsigned)H * (unsigned)s.quads;
    s.huber = huber, s.eps = eps;
    const bool vector = W % 4 == 0 && vec(s.depth) && vec(s.flow) && aligned(valid, 4);
    Step u;
    u.partial = s.partial, u.groups = groups, u.Tin = T0, u.Tout = T, u.status = status, u.normal = nullptr;
    u.solve = 1, u.first = 1, u.damping = (double)damping;
    const dim3 grid((unsigned)groups, (unsigned)N);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int passes = iters + (normal ? 1 : 0);
    for (int it = 0; it < passes; ++it) {
        if (vector) hipLaunchKernelGGL(pose_fit_accumulate<true>, grid, dim3(kThreads), 0, st, s);
        else hipLaunchKernelGGL(pose_fit_accumulate<false>, grid, dim3(kThreads), 0, st, s);
        if (it == iters) u.solve = 0, u.normal = normal;              // the last pass of a call that hands the sums out
        hipLaunchKernelGGL(pose_fit_update, dim3((unsigned)N), dim3(kThreads), 0, st, u);
        const int rc = check_launch(who);
        if (rc != DVS_OK) return rc;
        s.T = u.Tin = T, u.first = 0;
    }
    if (passes == 0) {                                                // nothing to fit and nothing to hand out: T = T0, status = 0
        u.partial = nullptr, u.solve = 0;
        hipLaunchKernelGGL(pose_fit_update, dim3((unsigned)N), dim3(kThreads), 0, st, u);
    }
    return check_launch(who);
}

}  // extern "C"
