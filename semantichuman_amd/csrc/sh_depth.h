// What the depth-image sources (depth.hip, depth_field.hip) share: a pixel's depth and the two tests on it, in the one fixed form
// of include/sh_kernels.h ("Depth images").  Booleans and one rounded product: nothing here can differ between the callers.
#pragma once
#include <limits.h>
#include "sh_common.h"

__device__ __forceinline__ bool depth_raw_ok(float) { return true; }
__device__ __forceinline__ bool depth_raw_ok(uint16_t raw) { return raw != 0; }

// z = fl((float)raw * depth_scale), both input types
template <typename T>
__device__ __forceinline__ float depth_z(T raw, float depth_scale) {
#pragma clang fp contract(off)
    return (float)raw * depth_scale;
}

// "There is a reading": z finite and positive, and not the word 0.  A NaN compares false.
template <typename T>
__device__ __forceinline__ bool depth_reading(T raw, float z) { return z > 0.f && z < INFINITY && depth_raw_ok(raw); }

// "Valid" of the header: a reading inside [z_near, z_far] that the mask (m, may be null; p the pixel's offset in it) does not
// exclude.  The mask is read only where everything else holds.
template <typename T>
__device__ __forceinline__ bool depth_valid(T raw, float z, float z_near, float z_far, const uint8_t* m, long p) {
    return z > 0.f && z < INFINITY && z_near <= z && z <= z_far && depth_raw_ok(raw) && (!m || m[p] != 0);
}

// "Camera rays", the forward model: a camera-frame point with Z > 0 -> (uf, vf) under k = (fx, fy, cx, cy), the coefficients
// d = (k1, k2, p1, p2, k3, k4, k5, k6) and the fold-back limit, every operation in fp32 and rounded on its own, in the header's
// order.  false: the point lies beyond the limit (a NaN included) and is outside whatever the polynomial would say.  The one
// text of it for free_space.hip and depth.hip.
__device__ __forceinline__ bool camera_project(float X, float Y, float Z, const float* k, const float* d, float limit, float& uf, float& vf) {
#pragma clang fp contract(off)
    const float a = X / Z, b = Y / Z;
    const float a2 = a * a, b2 = b * b;
    const float r2 = a2 + b2;
    if (!(r2 <= limit)) return false;
    const float r4 = r2 * r2;
    const float r6 = r4 * r2;
    const float num = ((1.f + d[0] * r2) + d[1] * r4) + d[4] * r6;
    const float den = ((1.f + d[5] * r2) + d[6] * r4) + d[7] * r6;
    const float rad = num / den;
    const float ab = a * b;
    const float tx = (2.f * d[2]) * ab + d[3] * (r2 + 2.f * a2);
    const float ty = d[2] * (r2 + 2.f * b2) + (2.f * d[3]) * ab;
    uf = k[0] * (a * rad + tx) + k[2];
    vf = k[1] * (b * rad + ty) + k[3];
    return true;
}

// What every depth entry point asks of the inputs they share; `who` names the caller in the message.
static inline int depth_check_inputs(const char* who, const void* depth, int dtype, const float* intr, int B, int H, int W) {
    SH_REQUIRE(dtype == SH_DEPTH_F32 || dtype == SH_DEPTH_U16, SH_ERR_INVALID_ARG, "%s: unknown depth dtype %d", who, dtype);
    SH_REQUIRE(depth && intr, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(B >= 0 && H >= 0 && W >= 0, SH_ERR_INVALID_ARG, "%s: negative size (B %d, H %d, W %d)", who, B, H, W);
    return SH_OK;
}
