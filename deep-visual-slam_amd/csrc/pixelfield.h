// What the per-pixel kernels over a flow [N][2][H][W], a depth [N][H][W] and a byte mask [N][H][W] share: flowcons.hip, rigidflow.hip
// and posefit.hip.  DESIGN.md section 27 states the rule once; each of the three files states its own arithmetic.
//
// SHAPE.  N in 1 .. 65535 (the image rides in a grid dimension), H and W in 1 .. 2^24 (pixel coordinates are exact in fp32).  A lane
// owns kPix = 4 consecutive pixels of a row: lane g = y * quads + x / 4 of an image, quads = ceil(W / 4), H * quads < 2^31 - 256.
// VIEWS, in element strides, read in place: Plane (the depth) holds d of (n, y, x) at p[n * image + y * row + x]; Field (a flow)
// holds u there and v one `plane` further on.  Rows are dense and nothing overlaps itself: row >= W, plane >= (H - 1) * row + W,
// image >= what an image holds, every stride below 2^40, p 4-byte aligned.  The byte mask and every output are dense, and an
// output whose bytes overlap an input's (or, where a caller asks, another output's) is refused.
// VECTOR FORM.  A lane's four floats are one 16-byte access and its four mask bytes one dword when W % 4 == 0, every stride of the
// view is a multiple of 4 and its pointer 16-byte aligned (vec()), a dense float output 16-byte and a byte field 4-byte aligned.
// Else the scalar form moves single elements: a float past the row's tail reads as NaN (no kernel of the family judges a NaN), a
// mask byte past it as 0, and nothing past it is stored.
// THE RAY.  rx = (iK[0][0]*x + iK[0][1]*y) + iK[0][2], ry and rz from rows 1 and 2, (X, Y, Z) = d * (rx, ry, rz): the reference's
// BackprojectDepth (vo/learner_func.py:106-131) in pixel coordinates.  What follows the ray is each kernel's own: rigidflow.hip
// multiplies by P = K T, posefit.hip applies T and then K, and the two round differently.
//
// fp32, every operation rounded on its own.  The pragma below has to stand HERE, before the first arithmetic of this header: one that
// the including file places after its #include lines leaves these functions under the compiler's default, back_project is
// contracted into fma, and the bit-exact restatements of the kernels no longer hold.  It stays in force for the including file.
#pragma once
#include "common.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

namespace dvs {

constexpr int kPix = 4;                             // pixels per lane: four bytes = one dword, four floats = 16 bytes
constexpr int kPixThreads = 256;                    // lanes per workgroup of the family's kernels
constexpr long long kStrideLimit = 1ll << 40;       // every element stride of a view is below this

struct Plane {
    const float* p;
    long long image, row;
};

struct Field {
    const float* p;                                 // may be null where a caller makes the flow optional: no view, vec() holds
    long long image, plane, row;
};

// ---- host: shape ------------------------------------------------------------------------------------------------------------------
// lanes per row of a shape the family takes, 0 for one it refuses
inline int quads_of(int N, int H, int W) {
    if (N < 1 || N > 65535 || H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24)) return 0;
    const long long quads = ((long long)W + kPix - 1) / kPix;
    return (long long)H * quads < (1ll << 31) - kPixThreads ? (int)quads : 0;
}

inline int check_shape(const char* who, int N, int H, int W, int* quads) {
    DVS_REQUIRE(N >= 1 && N <= 65535, "%s: N=%d images must be in 1 .. 65535", who, N);
    DVS_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24), "%s: H=%d, W=%d must be in 1 .. 2^24 (pixel coordinates are exact in fp32)",
                who, H, W);
    *quads = quads_of(N, H, W);
    DVS_REQUIRE(*quads > 0, "%s: H * W = %d x %d pixels per image exceed 2^31 - 1 lanes of four", who, H, W);
    return DVS_OK;
}

// ---- host: views ------------------------------------------------------------------------------------------------------------------
inline long long extent_of(long long row, int H, int W) { return (long long)(H - 1) * row + W; }       // elements of one plane

// a non-null pointer to floats: K, inv_K, T (dense [N][4][4]) and the head of either view
inline int check_floats(const char* who, const char* name, const float* p) {
    DVS_REQUIRE(p, "%s: null pointer (%s)", who, name);
    DVS_REQUIRE(aligned(p, 4), "%s: misaligned pointer (%s)", who, name);
    return DVS_OK;
}

inline int check_rows(const char* who, const char* name, const float* p, long long row, int W) {
    if (int rc = check_floats(who, name, p)) return rc;
    DVS_REQUIRE(row >= W, "%s: %s row stride %lld is below W=%d", who, name, row, W);
    return DVS_OK;
}

inline int check_plane(const char* who, const char* name, const Plane& v, int H, int W) {
    if (int rc = check_rows(who, name, v.p, v.row, W)) return rc;
    DVS_REQUIRE(v.row < kStrideLimit && v.image < kStrideLimit, "%s: %s strides %lld, %lld out of range", who, name, v.image, v.row);
    const long long extent = extent_of(v.row, H, W);
    DVS_REQUIRE(v.image >= extent, "%s: %s image stride %lld is below (H - 1) * row stride + W = %lld", who, name, v.image, extent);
    return DVS_OK;
}

inline int check_field(const char* who, const char* name, const Field& v, int H, int W) {
    if (int rc = check_rows(who, name, v.p, v.row, W)) return rc;
    DVS_REQUIRE(v.row < kStrideLimit && v.plane < kStrideLimit && v.image < kStrideLimit, "%s: %s strides %lld, %lld, %lld out of range", who,
                name, v.image, v.plane, v.row);
    const long long extent = extent_of(v.row, H, W);
    DVS_REQUIRE(v.plane >= extent, "%s: %s plane stride %lld is below (H - 1) * row stride + W = %lld", who, name, v.plane, extent);
    DVS_REQUIRE(v.image >= v.plane + extent, "%s: %s image stride %lld is below plane stride + (H - 1) * row stride + W = %lld", who, name,
                v.image, v.plane + extent);
    return DVS_OK;
}

inline bool vec(const Plane& v) { return v.row % 4 == 0 && v.image % 4 == 0 && aligned(v.p, 16); }
inline bool vec(const Field& v) { return v.row % 4 == 0 && v.plane % 4 == 0 && v.image % 4 == 0 && aligned(v.p, 16); }

// ---- host: overlap ----------------------------------------------------------------------------------------------------------------
struct Span {                                       // the bytes [lo, hi) an argument covers; empty for a null pointer
    const char* name;
    uintptr_t lo, hi;
};

inline Span span(const char* name, const void* p, long long bytes) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return Span{name, lo, p ? lo + (uintptr_t)bytes : lo};
}
inline Span span(const char* name, const Plane& v, int N, int H, int W) {
    return span(name, v.p, 4 * ((long long)(N - 1) * v.image + extent_of(v.row, H, W)));
}
inline Span span(const char* name, const Field& v, int N, int H, int W) {
    return span(name, v.p, 4 * ((long long)(N - 1) * v.image + v.plane + extent_of(v.row, H, W)));
}

// no output may overlap one of `others`, which are inputs or outputs as `kind` says.  A span is not held against itself, and
// "itself" is the same ELEMENT: pass the very array `outs` as `others` for outputs against outputs, never a copy of it
template <int A, int B>
int check_overlap(const char* who, const Span (&outs)[A], const Span (&others)[B], const char* kind) {
    for (const Span& o : outs)
        for (const Span& i : others)
            DVS_REQUIRE(&o == &i || !(o.lo < i.hi && i.lo < o.hi), "%s: output %s overlaps %s %s", who, o.name, kind, i.name);
    return DVS_OK;
}

// ---- device: the lane's pixels ----------------------------------------------------------------------------------------------------
// lane g of an image owns (x .. x + 3, y); y >= H for a lane past the image
__device__ __forceinline__ void lane_pixels(unsigned g, int quads, unsigned* y, int* x) {
    *y = g / (unsigned)quads;
    *x = (int)(g - *y * (unsigned)quads) * kPix;
}

template <class View>                                                  // Plane: d; Field: u, and v at + plane
__device__ __forceinline__ const float* at(const View& v, int n, unsigned y, int x) {
    return v.p + (size_t)n * (size_t)v.image + (size_t)y * (size_t)v.row + x;
}

// ---- device: loads and stores of a lane's four; `count` = W - x, the elements from p on that the row still holds --------------------
template <bool VEC>
__device__ __forceinline__ void load_quad(const float* p, int count, float (&v)[kPix]) {
    if (VEC) {                                                        // W % 4 == 0: the four are in the row, 16-byte aligned
        const float4 a = *reinterpret_cast<const float4*>(p);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k) v[k] = k < count ? p[k] : NAN;
    }
}

// the four mask bytes as one dword, byte k = pixel x + k; no mask (null): every pixel takes part
template <bool VEC>
__device__ __forceinline__ unsigned load_mask(const unsigned char* p, int count) {
    if (!p) return 0x01010101u;
    if (VEC) return *reinterpret_cast<const unsigned*>(p);
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < kPix; ++k)
        if (k < count) m |= (unsigned)p[k] << (8 * k);
    return m;
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float* p, int count, const float (&v)[kPix]) {
    if (VEC) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k)
            if (k < count) p[k] = v[k];
    }
}

template <bool VEC>
__device__ __forceinline__ void store_mask(unsigned char* p, int count, unsigned m) {
    if (VEC) {
        *reinterpret_cast<unsigned*>(p) = m;
    } else {
#pragma unroll
        for (int k = 0; k < kPix; ++k)
            if (k < count) p[k] = (unsigned char)(m >> (8 * k) & 255u);
    }
}

// ---- device: the ray --------------------------------------------------------------------------------------------------------------
// the three rows of one image's inv_K [4][4] that count
__device__ __forceinline__ void load_inv_K(const float* __restrict__ m, float (&iK)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) iK[i][j] = m[4 * i + j];
}

__device__ __forceinline__ void back_project(const float (&iK)[3][3], float x, float y, float d, float* X, float* Y, float* Z) {
    const float rx = (iK[0][0] * x + iK[0][1] * y) + iK[0][2];
    const float ry = (iK[1][0] * x + iK[1][1] * y) + iK[1][2];
    const float rz = (iK[2][0] * x + iK[2][1] * y) + iK[2][2];
    *X = d * rx, *Y = d * ry, *Z = d * rz;
}

}  // namespace dvs
