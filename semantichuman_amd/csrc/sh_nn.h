// What the scan-fitting sources (scan.hip, align.hip, surface.hip) share: the live-row count of a body, the fp64 wave sum, the
// squared distance and a face's cross product in their one fixed form, the check of a face's corners and the split of a target range into chunks.
#pragma once
#include "sh_common.h"
#include <math.h>
#include <type_traits>

constexpr int NN_WG_SLOTS = 2048;   // workgroups the chip holds at once (256 CUs x 8): the automatic split aims at this many

__device__ __forceinline__ int clamp_count(const int32_t* cnt, int b, int rows) {
    if (!cnt) return rows;
    const int c = cnt[b];
    return c < 0 ? 0 : (c > rows ? rows : c);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The distance of the header, in its one fixed form.
__device__ __forceinline__ float nn_d2(float qx, float qy, float qz, float tx, float ty, float tz) {
    const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

// The robust terms of the header ("Robust terms"), each in its one fixed fp32 form, every operation rounded on its own.  u: a
// pair's squared distance after truncation; scale2 = sigma^2 > 0.  ROBUST == SH_ROBUST_NONE is the identity / the constant 1 and
// costs nothing.  Huber is written as a select, so u == 0 never reaches the division.
template <int ROBUST>
__device__ __forceinline__ float robust_rho(float u, float scale2) {
#pragma clang fp contract(off)
    if constexpr (ROBUST == SH_ROBUST_GEMAN_MCCLURE) {
        const float t = scale2 / (scale2 + u);
        return u * t;
    } else if constexpr (ROBUST == SH_ROBUST_HUBER) {
        const float r = 2.0f * sqrtf(scale2 * u) - scale2;
        return u <= scale2 ? u : r;
    } else {
        return u;
    }
}

template <int ROBUST>
__device__ __forceinline__ float robust_weight(float u, float scale2) {
#pragma clang fp contract(off)
    if constexpr (ROBUST == SH_ROBUST_GEMAN_MCCLURE) {
        const float t = scale2 / (scale2 + u);
        return t * t;
    } else if constexpr (ROBUST == SH_ROBUST_HUBER) {
        const bool inside = u <= scale2;
        return inside ? 1.0f : sqrtf(scale2 / (inside ? 1.0f : u));
    } else {
        return 1.0f;
    }
}

// The checks every `_robust` entry point makes of its two extra arguments.
static inline int robust_check(const char* who, int robust, float scale2) {
    SH_REQUIRE(robust == SH_ROBUST_NONE || robust == SH_ROBUST_GEMAN_MCCLURE || robust == SH_ROBUST_HUBER, SH_ERR_INVALID_ARG,
               "%s: unknown robust form %d", who, robust);
    SH_REQUIRE(robust == SH_ROBUST_NONE || (scale2 > 0.f && scale2 < INFINITY), SH_ERR_INVALID_ARG,
               "%s: scale2 must be finite and > 0 with a robust form (got %g)", who, (double)scale2);
    return SH_OK;
}

// f(std::integral_constant<int, robust>): how a launcher picks the instantiation of a checked robust form.
template <class F>
static inline void robust_dispatch(int robust, F&& f) {
    if (robust == SH_ROBUST_GEMAN_MCCLURE) f(std::integral_constant<int, SH_ROBUST_GEMAN_MCCLURE>{});
    else if (robust == SH_ROBUST_HUBER) f(std::integral_constant<int, SH_ROBUST_HUBER>{});
    else f(std::integral_constant<int, SH_ROBUST_NONE>{});
}

// The cross product (b - a) x (c - a) of a face's corners, the header's expression ("Vertex normals") in its one fixed form: fp32
// differences from corner a, one fused multiply-add per component and no other contraction, so that every kernel that forms a
// face's normal (vertex_normals_kernel, face_normals_kernel, align.hip's face_normal) and the numpy transcriptions round alike.
__device__ __forceinline__ void face_cross(const float* a, const float* b, const float* c, float& cx, float& cy, float& cz) {
#pragma clang fp contract(off)
    const float ax = a[0], ay = a[1], az = a[2];
    const float abx = b[0] - ax, aby = b[1] - ay, abz = b[2] - az;
    const float acx = c[0] - ax, acy = c[1] - ay, acz = c[2] - az;
    cx = __builtin_fmaf(aby, acz, -(abz * acy));
    cy = __builtin_fmaf(abz, acx, -(abx * acz));
    cz = __builtin_fmaf(abx, acy, -(aby * acx));
}

// The three corners of face f (f inside the table); true when each is a vertex, i.e. lies in [0, n).  Every kernel that turns a
// face into rows of the model passes over a face that fails this.
__device__ __forceinline__ bool face_corners(const int32_t* __restrict__ faces, int f, int n, int& i0, int& i1, int& i2) {
    i0 = faces[3L * f]; i1 = faces[3L * f + 1]; i2 = faces[3L * f + 2];
    return (unsigned)i0 < (unsigned)n && (unsigned)i1 < (unsigned)n && (unsigned)i2 < (unsigned)n;
}

// One Jacobi rotation of the symmetric N x N matrix `a` in the plane (P, Q), accumulated into the eigenvector matrix `v`.
// Select form: a zero off-diagonal element gives the identity rotation, no branch.  N is deduced: align.hip's 4 x 4 (Horn's
// matrix) and cloud_normals.hip's 3 x 3 (a neighbourhood's covariance) run the same expressions.
template <int P, int Q, int N>
__device__ __forceinline__ void jacobi_rotate(double (&a)[N][N], double (&v)[N][N]) {
    const double apq = a[P][Q];
    const double tau = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
    t = (apq != 0.0 && t == t) ? t : 0.0;                                // apq == 0, or tau = +-inf / NaN: nothing to rotate
    const double c = 1.0 / sqrt(1.0 + t * t), sn = t * c;
#pragma unroll
    for (int k = 0; k < N; ++k) {                                        // columns P, Q
        const double akp = a[k][P], akq = a[k][Q];
        a[k][P] = c * akp - sn * akq; a[k][Q] = sn * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {                                        // rows P, Q
        const double apk = a[P][k], aqk = a[Q][k];
        a[P][k] = c * apk - sn * aqk; a[Q][k] = sn * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - sn * vkq; v[k][Q] = sn * vkp + c * vkq;
    }
}

// The split actually run for a request of `chunks` (0 = automatic: fill the chip) over nt targets in LDS tiles of `tile`, with
// `qt` queries per workgroup: whole tiles per chunk, no empty chunk.  Rounding the result once more changes nothing.
static inline int nn_resolve_chunks(int B, int nq, int nt, int tile, int qt, int chunks, int* tiles_per_chunk) {
    const int tiles = nt > 0 ? sh_cdiv(nt, tile) : 1;
    long c = chunks;
    if (c <= 0) {
        const long wgs = (long)sh_cdiv(nq > 0 ? nq : 1, qt) * (B > 0 ? B : 1);
        c = (NN_WG_SLOTS + wgs - 1) / wgs;
    }
    if (c > tiles) c = tiles;
    if (c < 1) c = 1;
    const int tpc = sh_cdiv(tiles, (int)c);
    *tiles_per_chunk = tpc;
    return sh_cdiv(tiles, tpc);
}
