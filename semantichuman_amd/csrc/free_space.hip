// Free space and silhouette from a depth field (include/sh_kernels.h, "Depth field"): every model vertex is projected into its
// body's image, one pixel is read, and the vertex is charged for standing in front of the surface the sensor measured (kind 1)
// or for projecting onto a pixel the sensor saw through (kind 2: its offset from the ray of the nearest pixel that is not
// empty).  The reference has no counterpart.  No search, no atomics, every output element one plain store; the per-vertex
// expressions are the header's, each operation rounded on its own.
// One kernel per pass serves one camera and the V cameras of a rig ("Free space from a rig"): the model -> camera maps come from
// one small kernel and the vertices are carried into each camera's frame inside the term kernels.  One camera is a rig of one
// whose vertices are in the camera's frame already: V = 1 and no cam, and the kernels take the vertex and hand back the gradient
// as they are - the rig's layouts at V = 1 are the one-camera layouts word for word, and so is the order of the sums.
#include <climits>

#include "sh_depth.h"
#include "sh_nn.h"

#pragma clang fp contract(off)          // the header's expressions, in the whole file

namespace {

struct FsArgs {
    const float* x; long x_sb; int n;
    const uint8_t* cls; const float* z; const int32_t* nearest; const float* intr;
    int H, W;
    const uint8_t* v_mask; long mask_sb;
    float margin;
};
struct FsTerm { int kind; float term, gx, gy, gz; };
// "Camera rays": the ray tables [images][H][W][2], coefficients [images][8] and limits [images] of the field's cameras; camera
// (b, v) is image b * stride + v, or with stride == 0 just v - one calibration per camera, shared by all bodies.
struct FsRays { const float* rays; const float* dist; const float* limit; int stride; };

// The header's case list for a camera-frame point (X, Y, Z) under the intrinsics k = (fx, fy, cx, cy) and image `image` of the field.
// DIST, "Camera rays": k is followed by the camera's 8 coefficients and its limit, the projection is the distorted one, and the
// silhouette ray is read from `table`, the camera's ray table; a NaN there: no term.
template <bool DIST>
__device__ __forceinline__ FsTerm fs_case(const FsArgs& a, long image, const float* k, float X, float Y, float Z, const float* table) {
    const float fx = k[0], fy = k[1], cx = k[2], cy = k[3];
    FsTerm r = {SH_FS_OUTSIDE, 0.f, 0.f, 0.f, 0.f};
    if (!(Z > 0.f)) return r;                                            // a NaN included
    float uf, vf;
    if constexpr (DIST) {
        if (!camera_project(X, Y, Z, k, k + 4, k[12], uf, vf)) return r;
    } else {
        uf = (X * fx) / Z + cx; vf = (Y * fy) / Z + cy;
    }
    const bool inside = uf >= -0.5f && uf < (float)a.W - 0.5f && vf >= -0.5f && vf < (float)a.H - 0.5f;   // a NaN is outside
    if (!inside) return r;
    const int u = min((int)floorf(uf + 0.5f), a.W - 1), v = min((int)floorf(vf + 0.5f), a.H - 1);        // the min never binds: no read beyond the image whatever the rounding
    const long px = (image * a.H + v) * a.W + u;
    const int c = a.cls[px];
    r.kind = SH_FS_NONE;
    if (c == SH_FIELD_SURFACE) {
        const float e = (a.z[px] - a.margin) - Z;
        if (e > 0.f) {
            r.kind = SH_FS_FREE;
            r.term = e * e;
            r.gz = -2.f * e;
        }
    } else if (c == SH_FIELD_EMPTY) {
        const int q = a.nearest[px];
        if (q >= 0) {
            const int vq = q / a.W, uq = q - vq * a.W;
            float ra, rb;
            if constexpr (DIST) {
                ra = table[2L * q]; rb = table[2L * q + 1];
            } else {
                ra = ((float)uq - cx) / fx; rb = ((float)vq - cy) / fy;
            }
            if (!DIST || (ra == ra && rb == rb)) {
                const float rx = X - ra * Z, ry = Y - rb * Z;
                r.kind = SH_FS_SILHOUETTE;
                r.term = rx * rx + ry * ry;
                r.gx = 2.f * rx;
                r.gy = 2.f * ry;
                r.gz = -2.f * (ra * rx + rb * ry);
            }
        }
    } else {
        r.kind = SH_FS_UNKNOWN;
    }
    return r;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int VIEWS_NT = 1024;          // the forward workgroup: the terms are written by all of it, folded by its first 256 threads
constexpr int VIEW_WORDS = 16;          // a view's record in LDS: the 12 words of cam (M row-major, c), then fx, fy, cx, cy
constexpr int DIST_VIEW_WORDS = 25;     // "Camera rays": then the 8 coefficients and the limit
constexpr int view_words(bool dist) { return dist ? DIST_VIEW_WORDS : VIEW_WORDS; }

// grid (cdiv(B * V, 64)), thread = one (body, view): the header's fp64 expressions, in its order.
__global__ __launch_bounds__(64) void free_space_cameras_kernel(const float* __restrict__ pose, const float* __restrict__ ext, int BV, int V,
                                                               float* __restrict__ cam) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= BV) return;
    const int b = j / V;
    double a[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, e[12];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        if (pose) a[k] = (double)pose[12L * b + k];
        const float w = ext[12L * j + k];
        ok = ok && w == w;
        e[k] = (double)w;
    }
    double kx[3][3];                                                     // kx[j]: the j-th row of the adjugate's transpose
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double* p = a + 3 * ((r + 1) % 3);
        const double* q = a + 3 * ((r + 2) % 3);
        kx[r][0] = p[1] * q[2] - p[2] * q[1];
        kx[r][1] = p[2] * q[0] - p[0] * q[2];
        kx[r][2] = p[0] * q[1] - p[1] * q[0];
    }
    const double det = (a[0] * kx[0][0] + a[1] * kx[0][1]) + a[2] * kx[0][2];
    ok = ok && det != 0.0 && fabs(det) <= 1.7976931348623157e308 && det == det;
    double inv[3][3], p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) inv[i][c] = kx[c][i] / det;
        p[i] = ((inv[i][0] * a[9] + inv[i][1] * a[10]) + inv[i][2] * a[11]) + e[9 + i];
    }
    float* o = cam + 12L * j;
    const float nan = __int_as_float(0x7fc00000);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * i + c] = ok ? (float)((e[i] * inv[0][c] + e[3 + i] * inv[1][c]) + e[6 + i] * inv[2][c]) : nan;
        o[9 + i] = ok ? (float)(-((e[i] * p[0] + e[3 + i] * p[1]) + e[6 + i] * p[2])) : nan;
    }
}

// The body's V records into LDS (ends with a barrier): every later read of them is a broadcast.  Without cam (CAM false) the
// twelve words of the map are neither staged nor read.  CAM is a template parameter because a test of cam around the load keeps
// hipcc from unrolling this loop as it does for a rig.
template <int NT, bool CAM, bool DIST>
__device__ __forceinline__ void stage_views(const FsArgs& a, const float* __restrict__ cam, int V, int b, float* sv, const FsRays& fr) {
    constexpr int WORDS = view_words(DIST);
    for (int i = threadIdx.x; i < V * WORDS; i += NT) {
        const int v = i / WORDS, k = i - v * WORDS;
        const long rec = (long)b * V + v;
        if constexpr (DIST) {
            const long c = fr.stride ? (long)b * fr.stride + v : (long)v;
            if (k >= 16) sv[i] = k < 24 ? fr.dist[8 * c + (k - 16)] : fr.limit[c];
            else if (k >= 12) sv[i] = a.intr[4 * rec + (k - 12)];
            else if (CAM) sv[i] = cam[12 * rec + k];
        } else if constexpr (CAM) sv[i] = k < 12 ? cam[12 * rec + k] : a.intr[4 * rec + (k - 12)];
        else if (k >= 12) sv[i] = a.intr[4 * rec + (k - 12)];
    }
    __syncthreads();
}

// The header's Q = M x + c of one view's record, then the case list under that view's intrinsics and image.  CAM false: x is in
// the camera's frame already and is taken as it is - under an identity record 0 * inf would make a vertex at Z = +inf a NaN.
template <bool CAM, bool DIST>
__device__ __forceinline__ FsTerm fs_view(const FsArgs& a, const float* rec, long image, float x0, float x1, float x2, const float* table) {
    if constexpr (!CAM) return fs_case<DIST>(a, image, rec + 12, x0, x1, x2, table);
    const float X = ((rec[0] * x0 + rec[1] * x1) + rec[2] * x2) + rec[9];
    const float Y = ((rec[3] * x0 + rec[4] * x1) + rec[5] * x2) + rec[10];
    const float Z = ((rec[6] * x0 + rec[7] * x1) + rec[8] * x2) + rec[11];
    return fs_case<DIST>(a, image, rec + 12, X, Y, Z, table);
}

// The ray table of camera (b, v) under fr (nullptr without one).
template <bool DIST>
__device__ __forceinline__ const float* fs_table(const FsArgs& a, const FsRays& fr, int b, int v) {
    if constexpr (!DIST) return nullptr;
    return fr.rays + 2L * a.H * a.W * (fr.stride ? (long)b * fr.stride + v : (long)v);
}

// grid (body), VIEWS_NT threads.  (1) Every thread takes vertices tid, tid + VIEWS_NT, ... and, in a uniform loop over the views,
// stores term and kind.  (2) After the barrier the first 256 threads read them back in the header's order - thread t the vertices
// t, t + 256, ..., the views ascending inside a vertex - into the two fp64 sums; the wave butterfly and the four wave sums as in
// chamfer_fwd_kernel.  (3) The counts are integers: per view, all threads count the stored kinds.  CAM false: cam == nullptr, one
// camera, V = 1.  The form is a template parameter in both kernels: the rig's instantiations are the code they were before.
template <bool CAM, bool DIST>
__global__ __launch_bounds__(VIEWS_NT) void free_space_fwd_kernel(FsArgs a, const float* __restrict__ cam, int V, float* term, uint8_t* kind,
                                                                 float* __restrict__ loss, int32_t* __restrict__ counts, FsRays fr) {
    constexpr int WORDS = view_words(DIST);
    __shared__ float sv[SH_DEPTH_MAX_VIEWS * WORDS];
    __shared__ double red[2][4];
    __shared__ int redi[SH_DEPTH_MAX_VIEWS][3][VIEWS_NT / 64];
    __shared__ int reda[VIEWS_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    stage_views<VIEWS_NT, CAM, DIST>(a, cam, V, b, sv, fr);
    const uint8_t* mb = a.v_mask ? a.v_mask + (long)b * a.mask_sb : nullptr;
    const long plane = (long)b * V * a.n;
    int na = 0;
    for (int i = tid; i < a.n; i += VIEWS_NT) {
        const bool active = !mb || mb[i] != 0;
        na += active;
        const float* p = a.x + (long)b * a.x_sb + 3L * i;
        const float x0 = p[0], x1 = p[1], x2 = p[2];
        for (int v = 0; v < V; ++v) {                                    // uniform
            FsTerm r = {SH_FS_NONE, 0.f, 0.f, 0.f, 0.f};
            if (active) r = fs_view<CAM, DIST>(a, sv + WORDS * v, (long)b * V + v, x0, x1, x2, fs_table<DIST>(a, fr, b, v));
            term[plane + (long)v * a.n + i] = r.term;
            kind[plane + (long)v * a.n + i] = (uint8_t)r.kind;
        }
    }
    na = wave_sum_i(na);
    if ((tid & 63) == 0) reda[wave] = na;
    __syncthreads();                                                     // the workgroup's own stores are visible to it from here on
    double s1 = 0.0, s2 = 0.0;
    if (tid < 256) {
        for (int i = tid; i < a.n; i += 256) {
            for (int v = 0; v < V; ++v) {
                const int k = kind[plane + (long)v * a.n + i];
                const float t = term[plane + (long)v * a.n + i];
                if (k == SH_FS_FREE) s1 += (double)t;
                if (k == SH_FS_SILHOUETTE) s2 += (double)t;
            }
        }
    }
    s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
    if ((tid & 63) == 0 && wave < 4) { red[0][wave] = s1; red[1][wave] = s2; }
    for (int v = 0; v < V; ++v) {
        int k1 = 0, k2 = 0, k4 = 0;
        for (int i = tid; i < a.n; i += VIEWS_NT) {
            const int k = kind[plane + (long)v * a.n + i];
            k1 += k == SH_FS_FREE; k2 += k == SH_FS_SILHOUETTE; k4 += k == SH_FS_OUTSIDE;
        }
        k1 = wave_sum_i(k1); k2 = wave_sum_i(k2); k4 = wave_sum_i(k4);
        if ((tid & 63) == 0) { redi[v][0][wave] = k1; redi[v][1][wave] = k2; redi[v][2][wave] = k4; }
    }
    __syncthreads();
    int n_act = 0;
    for (int w = 0; w < VIEWS_NT / 64; ++w) n_act += reda[w];
    if (tid == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < 4; ++w) { t1 += red[0][w]; t2 += red[1][w]; }
        loss[2 * b] = n_act > 0 ? (float)(t1 / (double)n_act) : 0.f;
        loss[2 * b + 1] = n_act > 0 ? (float)(t2 / (double)n_act) : 0.f;
    }
    if (tid < V) {
        int32_t* c = counts + 4L * ((long)b * V + tid);
        c[0] = n_act;
        for (int j = 0; j < 3; ++j) {
            int s = 0;
            for (int w = 0; w < VIEWS_NT / 64; ++w) s += redi[tid][j][w];
            c[1 + j] = s;
        }
    }
}

// grid (row tile of 256, body), thread = one row of g_x: per view the case list once more, its gradient times
// fl(gL[b][k] * fl(1 / n_act)), carried back by M^T and added in fp32, the views ascending.  CAM false: cam == nullptr, one camera,
// V = 1, and that product is the row itself - through an identity record -0 + 0 would lose the sign of a zero.
template <bool CAM, bool DIST>
__global__ __launch_bounds__(256) void free_space_bwd_kernel(FsArgs a, const float* __restrict__ cam, int V, int rows,
                                                            const int32_t* __restrict__ counts, const float* __restrict__ gL,
                                                            float* __restrict__ g_x, FsRays fr) {
    constexpr int WORDS = view_words(DIST);
    __shared__ float sv[SH_DEPTH_MAX_VIEWS * WORDS];
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    stage_views<256, CAM, DIST>(a, cam, V, b, sv, fr);
    if (i >= rows) return;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (i < a.n && (!a.v_mask || a.v_mask[(long)b * a.mask_sb + i] != 0)) {
        const float* p = a.x + (long)b * a.x_sb + 3L * i;
        const float x0 = p[0], x1 = p[1], x2 = p[2];
        const float inv = 1.f / (float)counts[4L * b * V];              // n_act >= 1: this vertex is active
        const float s_free = gL[2 * b] * inv, s_sil = gL[2 * b + 1] * inv;
        for (int v = 0; v < V; ++v) {                                    // uniform
            const float* rec = sv + WORDS * v;
            const FsTerm r = fs_view<CAM, DIST>(a, rec, (long)b * V + v, x0, x1, x2, fs_table<DIST>(a, fr, b, v));
            if (r.kind == SH_FS_FREE || r.kind == SH_FS_SILHOUETTE) {
                const float s = r.kind == SH_FS_SILHOUETTE ? s_sil : s_free;
                const float w0 = s * r.gx, w1 = s * r.gy, w2 = s * r.gz;
                if constexpr (!CAM) {
                    g0 = w0; g1 = w1; g2 = w2;
                } else {
                    g0 += (rec[0] * w0 + rec[3] * w1) + rec[6] * w2;
                    g1 += (rec[1] * w0 + rec[4] * w1) + rec[7] * w2;
                    g2 += (rec[2] * w0 + rec[5] * w1) + rec[8] * w2;
                }
            }
        }
    }
    float* o = g_x + ((long)b * rows + i) * 3;
    o[0] = g0; o[1] = g1; o[2] = g2;
}

// What the four entry points ask of their arguments; `who` names the one that was called in every error text.  One camera:
// rig = false, cam = nullptr and V = 1, for which the rig's limits are the one camera's own.
int check_args(const char* who, bool rig, const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
               const int32_t* nearest, const float* intr, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, int B) {
    SH_REQUIRE(!rig || cam, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(V >= 1 && V <= SH_DEPTH_MAX_VIEWS, SH_ERR_INVALID_ARG, "%s: V = %d views, must lie in [1, %d]", who, V, SH_DEPTH_MAX_VIEWS);
    SH_REQUIRE(x && cls && z && nearest && intr, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(B >= 0 && H >= 0 && W >= 0 && rows >= 0 && n >= 0 && n <= rows, SH_ERR_INVALID_ARG,
               "%s: bad size (B %d, H %d, W %d, rows %d, n %d)", who, B, H, W, rows, n);
    SH_REQUIRE(margin >= 0.f, SH_ERR_INVALID_ARG, "%s: margin must be >= 0 (and not NaN)", who);
    SH_REQUIRE(B <= 1 || x_sb >= 3L * n, SH_ERR_INVALID_ARG, "%s: batch stride %ld shorter than a body", who, (long)x_sb);
    SH_REQUIRE(!v_mask || mask_sb == 0 || mask_sb >= n, SH_ERR_INVALID_ARG, "%s: mask stride %ld shorter than n", who, (long)mask_sb);
    SH_REQUIRE(H <= SH_FIELD_MAX_SIDE && W <= SH_FIELD_MAX_SIDE && B <= 65535, SH_ERR_UNSUPPORTED, "%s: H and W must not exceed %d (B 65535)", who,
               SH_FIELD_MAX_SIDE);
    SH_REQUIRE((n == 0) || (H > 0 && W > 0), SH_ERR_INVALID_ARG, "%s: an empty image (H %d, W %d)", who, H, W);
    SH_REQUIRE((long)B * V <= 65535 && (long)V * H * W <= INT_MAX, SH_ERR_UNSUPPORTED,
               "%s: B * V must not exceed 65535 and V * H * W must fit in 31 bits (B %d, V %d, H %d, W %d)", who, B, V, H, W);
    return SH_OK;
}

// "Camera rays": what the two _rays entry points ask of the calibration (fr null: the pinhole entry points, nothing to ask).
int check_rays(const char* who, const FsRays* fr, int V) {
    if (!fr) return SH_OK;
    SH_REQUIRE(fr->rays && fr->dist && fr->limit, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(fr->stride == 0 || fr->stride == V, SH_ERR_INVALID_ARG, "%s: rays_stride = %d, must be 0 (one table per camera) or %d", who, fr->stride, V);
    return SH_OK;
}

// Every check and the launch of a forward entry point, and below of a backward one.  The launch record is the entry point's name
// without the "sh_", then "_kernel"; only a rig's names V.
int free_space_fwd(const char* who, bool rig, const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                   const int32_t* nearest, const float* intr, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, int B,
                   float* term, uint8_t* kind, float* loss, int32_t* counts, sh_stream_t stream, const FsRays* fr = nullptr) {
    if (const int rc = check_args(who, rig, x, x_sb, rows, n, cam, cls, z, nearest, intr, V, H, W, v_mask, mask_sb, margin, B)) return rc;
    if (const int rc = check_rays(who, fr, V)) return rc;
    SH_REQUIRE(term && kind && loss && counts, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    if (B == 0) return SH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FsArgs a = {x, (long)x_sb, n, cls, z, nearest, intr, H, W, v_mask, (long)mask_sb, margin};
    char views[16] = "";
    if (rig) snprintf(views, sizeof views, " V=%d", V);
    ShProfScope ps(st, "%s_kernel|B=%d%s n=%d H=%d W=%d", who + 3, B, views, n, H, W);
    const FsRays none = {nullptr, nullptr, nullptr, 0};
    if (fr && cam) SH_LAUNCH_PS(ps, (free_space_fwd_kernel<true, true>), dim3((unsigned)B), dim3(VIEWS_NT), 0, st, a, cam, V, term, kind, loss, counts, *fr);
    else if (fr) SH_LAUNCH_PS(ps, (free_space_fwd_kernel<false, true>), dim3((unsigned)B), dim3(VIEWS_NT), 0, st, a, cam, V, term, kind, loss, counts, *fr);
    else if (cam) SH_LAUNCH_PS(ps, (free_space_fwd_kernel<true, false>), dim3((unsigned)B), dim3(VIEWS_NT), 0, st, a, cam, V, term, kind, loss, counts, none);
    else SH_LAUNCH_PS(ps, (free_space_fwd_kernel<false, false>), dim3((unsigned)B), dim3(VIEWS_NT), 0, st, a, cam, V, term, kind, loss, counts, none);
    SH_CHECK_LAUNCH(who + 3);
    return SH_OK;
}

int free_space_bwd(const char* who, bool rig, const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                   const int32_t* nearest, const float* intr, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin,
                   const int32_t* counts, const float* gL, int B, float* g_x, sh_stream_t stream, const FsRays* fr = nullptr) {
    if (const int rc = check_args(who, rig, x, x_sb, rows, n, cam, cls, z, nearest, intr, V, H, W, v_mask, mask_sb, margin, B)) return rc;
    if (const int rc = check_rays(who, fr, V)) return rc;
    SH_REQUIRE(counts && gL && g_x, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    if (B == 0 || rows == 0) return SH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FsArgs a = {x, (long)x_sb, n, cls, z, nearest, intr, H, W, v_mask, (long)mask_sb, margin};
    char views[16] = "";
    if (rig) snprintf(views, sizeof views, " V=%d", V);
    ShProfScope ps(st, "%s_kernel|B=%d%s rows=%d n=%d", who + 3, B, views, rows, n);
    const dim3 grid((unsigned)sh_cdiv(rows, 256), (unsigned)B);
    const FsRays none = {nullptr, nullptr, nullptr, 0};
    if (fr && cam) SH_LAUNCH_PS(ps, (free_space_bwd_kernel<true, true>), grid, dim3(256), 0, st, a, cam, V, rows, counts, gL, g_x, *fr);
    else if (fr) SH_LAUNCH_PS(ps, (free_space_bwd_kernel<false, true>), grid, dim3(256), 0, st, a, cam, V, rows, counts, gL, g_x, *fr);
    else if (cam) SH_LAUNCH_PS(ps, (free_space_bwd_kernel<true, false>), grid, dim3(256), 0, st, a, cam, V, rows, counts, gL, g_x, none);
    else SH_LAUNCH_PS(ps, (free_space_bwd_kernel<false, false>), grid, dim3(256), 0, st, a, cam, V, rows, counts, gL, g_x, none);
    SH_CHECK_LAUNCH(who + 3);
    return SH_OK;
}

}  // namespace

extern "C" {

int sh_free_space_fwd(const float* x, int64_t x_sb, int rows, int n, const uint8_t* cls, const float* z, const int32_t* nearest,
                      const float* intr, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, int B, float* term, uint8_t* kind,
                      float* loss, int32_t* counts, sh_stream_t stream) {
    return free_space_fwd("sh_free_space_fwd", false, x, x_sb, rows, n, nullptr, cls, z, nearest, intr, 1, H, W, v_mask, mask_sb, margin, B, term,
                          kind, loss, counts, stream);
}

int sh_free_space_bwd(const float* x, int64_t x_sb, int rows, int n, const uint8_t* cls, const float* z, const int32_t* nearest,
                      const float* intr, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, const int32_t* counts,
                      const float* gL, int B, float* g_x, sh_stream_t stream) {
    return free_space_bwd("sh_free_space_bwd", false, x, x_sb, rows, n, nullptr, cls, z, nearest, intr, 1, H, W, v_mask, mask_sb, margin, counts,
                          gL, B, g_x, stream);
}

int sh_free_space_cameras(const float* pose, const float* ext, int B, int V, float* cam, sh_stream_t stream) {
    const char* who = "sh_free_space_cameras";
    SH_REQUIRE(ext && cam, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(V >= 1 && V <= SH_DEPTH_MAX_VIEWS, SH_ERR_INVALID_ARG, "%s: V = %d views, must lie in [1, %d]", who, V, SH_DEPTH_MAX_VIEWS);
    SH_REQUIRE(B >= 0, SH_ERR_INVALID_ARG, "%s: bad size (B %d)", who, B);
    SH_REQUIRE(B <= 65535 && (long)B * V <= 65535, SH_ERR_UNSUPPORTED, "%s: B and B * V must not exceed 65535 (B %d, V %d)", who, B, V);
    if (B == 0) return SH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "free_space_cameras_kernel|B=%d V=%d pose=%d", B, V, pose != nullptr);
    SH_LAUNCH_PS(ps, free_space_cameras_kernel, dim3((unsigned)sh_cdiv(B * V, 64)), dim3(64), 0, st, pose, ext, B * V, V, cam);
    SH_CHECK_LAUNCH("free_space_cameras");
    return SH_OK;
}

int sh_free_space_views_fwd(const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                            const int32_t* nearest, const float* intr, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin,
                            int B, float* term, uint8_t* kind, float* loss, int32_t* counts, sh_stream_t stream) {
    return free_space_fwd("sh_free_space_views_fwd", true, x, x_sb, rows, n, cam, cls, z, nearest, intr, V, H, W, v_mask, mask_sb, margin, B, term,
                          kind, loss, counts, stream);
}

int sh_free_space_views_bwd(const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                            const int32_t* nearest, const float* intr, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin,
                            const int32_t* counts, const float* gL, int B, float* g_x, sh_stream_t stream) {
    return free_space_bwd("sh_free_space_views_bwd", true, x, x_sb, rows, n, cam, cls, z, nearest, intr, V, H, W, v_mask, mask_sb, margin, counts,
                          gL, B, g_x, stream);
}

// "Camera rays": the pair above under a lens model.  cam may be NULL: one camera, V = 1, x in its frame.
int sh_free_space_views_rays_fwd(const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                                 const int32_t* nearest, const float* intr, const float* rays, const float* dist, const float* limit,
                                 int rays_stride, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, int B, float* term,
                                 uint8_t* kind, float* loss, int32_t* counts, sh_stream_t stream) {
    const char* who = "sh_free_space_views_rays_fwd";
    SH_REQUIRE(cam || V == 1, SH_ERR_INVALID_ARG, "%s: without cam there is one camera, V = %d", who, V);
    const FsRays fr = {rays, dist, limit, rays_stride};
    return free_space_fwd(who, cam != nullptr, x, x_sb, rows, n, cam, cls, z, nearest, intr, V, H, W, v_mask, mask_sb, margin, B, term, kind, loss, counts,
                          stream, &fr);
}

int sh_free_space_views_rays_bwd(const float* x, int64_t x_sb, int rows, int n, const float* cam, const uint8_t* cls, const float* z,
                                 const int32_t* nearest, const float* intr, const float* rays, const float* dist, const float* limit,
                                 int rays_stride, int V, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin,
                                 const int32_t* counts, const float* gL, int B, float* g_x, sh_stream_t stream) {
    const char* who = "sh_free_space_views_rays_bwd";
    SH_REQUIRE(cam || V == 1, SH_ERR_INVALID_ARG, "%s: without cam there is one camera, V = %d", who, V);
    const FsRays fr = {rays, dist, limit, rays_stride};
    return free_space_bwd(who, cam != nullptr, x, x_sb, rows, n, cam, cls, z, nearest, intr, V, H, W, v_mask, mask_sb, margin, counts, gL, B, g_x, stream,
                          &fr);
}

}  // extern "C"
