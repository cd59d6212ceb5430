// Camera rays (include/sh_kernels.h, "Camera rays"): the pixel -> ray table of a calibrated depth camera under OpenCV's
// 8-coefficient rational model, its fold-back limit and whether every pixel has a ray.  The reference has no counterpart.
// The inverse has no closed form: every sample runs the header's 20 fixed-point steps and one forward evaluation in fp64, every
// operation rounded on its own, so the table is a pure function of (intrinsics, coefficients, pixel): the same bits for a camera
// alone and in any batch.  Two launches: one thread per pixel centre writes the table; one workgroup per camera then folds the
// table and the image rectangle's boundary samples into the limit - a float maximum and a logical and, neither of which depends
// on the order, so no atomics and no workspace.  Runs once per calibrated camera, at packing time.
#include <climits>

#include "sh_common.h"

#pragma clang fp contract(off)          // the header's expressions, in the whole file

namespace {

constexpr int RAY_NT = 256;             // the table kernel: one thread per pixel centre
constexpr int LIMIT_NT = 1024;          // the limit kernel: one workgroup per camera
constexpr int STEPS = 20;               // a definition, not a tuning result (the header)

struct CamModel { double fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6; };

__device__ __forceinline__ CamModel load_model(const float* __restrict__ intr, const float* __restrict__ dist, int c) {
    const float* k = intr + 4L * c;
    const float* d = dist + 8L * c;
    return {(double)k[0], (double)k[1], (double)k[2], (double)k[3], (double)d[0], (double)d[1], (double)d[2], (double)d[3],
            (double)d[4], (double)d[5], (double)d[6], (double)d[7]};
}

// The header's inverse at the sample (u, v): false - no ray - when the reprojection misses by more than 1e-3 pixel on an axis,
// num or den is not positive, or anything is NaN (every compare is then false).
__device__ __forceinline__ bool invert(const CamModel& m, double u, double v, double& x, double& y) {
    const double xd = (u - m.cx) / m.fx, yd = (v - m.cy) / m.fy;
    x = xd; y = yd;
    double num = 1.0, den = 1.0, tx = 0.0, ty = 0.0;
    for (int it = 0; it <= STEPS; ++it) {                                // STEPS updates, then the terms once more at the result
        const double a2 = x * x, b2 = y * y;
        const double r2 = a2 + b2;
        const double r4 = r2 * r2;
        const double r6 = r4 * r2;
        num = ((1.0 + m.k1 * r2) + m.k2 * r4) + m.k3 * r6;
        den = ((1.0 + m.k4 * r2) + m.k5 * r4) + m.k6 * r6;
        const double ab = x * y;
        tx = (2.0 * m.p1) * ab + m.p2 * (r2 + 2.0 * a2);
        ty = m.p1 * (r2 + 2.0 * b2) + (2.0 * m.p2) * ab;
        if (it == STEPS) break;
        const double s = den / num;
        x = (xd - tx) * s;
        y = (yd - ty) * s;
    }
    const double rad = num / den;
    const double uu = m.fx * (x * rad + tx) + m.cx, vv = m.fy * (y * rad + ty) + m.cy;
    return fabs(uu - u) <= 1e-3 && fabs(vv - v) <= 1e-3 && num > 0.0 && den > 0.0;
}

// grid (cdiv(H * W, RAY_NT), camera), thread = one pixel centre.
__global__ __launch_bounds__(RAY_NT) void camera_rays_kernel(const float* __restrict__ intr, const float* __restrict__ dist, int H, int W,
                                                            float* __restrict__ rays) {
    const int c = blockIdx.y;
    const long p = (long)blockIdx.x * RAY_NT + threadIdx.x, image = (long)H * W;
    if (p >= image) return;
    const int v = (int)(p / W), u = (int)(p - (long)v * W);
    const CamModel m = load_model(intr, dist, c);
    double x, y;
    const bool ok = invert(m, (double)u, (double)v, x, y);
    const float nan = __int_as_float(0x7fc00000);
    float2 r = {ok ? (float)x : nan, ok ? (float)y : nan};
    reinterpret_cast<float2*>(rays)[c * image + p] = r;
}

// The header's r2 of a ray: fp32, the form the forward model compares with the limit.
__device__ __forceinline__ float ray_r2(float a, float b) { return a * a + b * b; }

// grid (camera), LIMIT_NT threads: the maximum of r2 over the table's rays and the converged boundary samples, and whether the
// table holds no NaN.  The boundary: i = 0 .. W on the lines v = -0.5 and v = H - 0.5, j = 0 .. H on u = -0.5 and u = W - 0.5.
__global__ __launch_bounds__(LIMIT_NT) void camera_limit_kernel(const float* __restrict__ intr, const float* __restrict__ dist, int H, int W,
                                                               const float* __restrict__ rays, float* __restrict__ limit,
                                                               int32_t* __restrict__ complete) {
    __shared__ float smax[LIMIT_NT / 64];
    __shared__ int sall[LIMIT_NT / 64];
    const int c = blockIdx.x, tid = threadIdx.x;
    const long image = (long)H * W;
    const float2* t = reinterpret_cast<const float2*>(rays) + c * image;
    float best = 0.f;
    bool all = true;
    for (long p = tid; p < image; p += LIMIT_NT) {
        const float2 r = t[p];
        const bool has = r.x == r.x && r.y == r.y;
        all = all && has;
        if (has) best = fmaxf(best, ray_r2(r.x, r.y));
    }
    const CamModel m = load_model(intr, dist, c);
    const int top = W + 1, side = H + 1;
    for (int s = tid; s < 2 * (top + side); s += LIMIT_NT) {
        double u, v;
        if (s < 2 * top) { u = (double)(s % top) - 0.5; v = s < top ? -0.5 : (double)H - 0.5; }
        else { const int j = s - 2 * top; v = (double)(j % side) - 0.5; u = j < side ? -0.5 : (double)W - 0.5; }
        double x, y;
        if (invert(m, u, v, x, y)) best = fmaxf(best, ray_r2((float)x, (float)y));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    const bool wave_all = __ballot(!all) == 0ull;
    const int lane = tid & 63, w = sh_wave_id();
    if (lane == 0) { smax[w] = best; sall[w] = wave_all; }
    __syncthreads();
    if (tid == 0) {
        float mx = 0.f;
        int ok = 1;
        for (int i = 0; i < LIMIT_NT / 64; ++i) { mx = fmaxf(mx, smax[i]); ok = ok && sall[i]; }
        limit[c] = mx;
        complete[c] = ok;
    }
}

}  // namespace

extern "C" {

int sh_camera_rays(const float* intr, const float* dist, int C, int H, int W, float* rays, float* limit, int32_t* complete, sh_stream_t stream) {
    const char* who = "sh_camera_rays";
    SH_REQUIRE(intr && dist && rays && limit && complete, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(C >= 0 && H >= 0 && W >= 0, SH_ERR_INVALID_ARG, "%s: negative size (C %d, H %d, W %d)", who, C, H, W);
    SH_REQUIRE(C <= 65535 && (long)H * W <= INT_MAX - 2L * (H + W + 2), SH_ERR_UNSUPPORTED, "%s: C or H * W too large", who);
    if (C == 0 || H == 0 || W == 0) return SH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ShProfScope ps(st, "camera_rays_kernel|C=%d H=%d W=%d", C, H, W);
        const dim3 grid((unsigned)(((long)H * W + RAY_NT - 1) / RAY_NT), (unsigned)C);
        SH_LAUNCH_PS(ps, camera_rays_kernel, grid, dim3(RAY_NT), 0, st, intr, dist, H, W, rays);
    }
    {
        ShProfScope ps(st, "camera_limit_kernel|C=%d H=%d W=%d", C, H, W);
        SH_LAUNCH_PS(ps, camera_limit_kernel, dim3((unsigned)C), dim3(LIMIT_NT), 0, st, intr, dist, H, W, static_cast<const float*>(rays), limit, complete);
    }
    SH_CHECK_LAUNCH("camera_rays");
    return SH_OK;
}

}  // extern "C"
