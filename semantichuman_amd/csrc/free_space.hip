// Free space and silhouette from a depth field (include/sh_kernels.h, "Depth field"): every model vertex is projected into its
// body's image, one pixel is read, and the vertex is charged for standing in front of the surface the sensor measured (kind 1)
// or for projecting onto a pixel the sensor saw through (kind 2: its offset from the ray of the nearest pixel that is not
// empty).  The reference has no counterpart.  No search, no atomics, every output element one plain store; the per-vertex
// expressions are the header's, each operation rounded on its own.
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

// The header's case list for the active vertex i of body b.
__device__ __forceinline__ FsTerm fs_term(const FsArgs& a, int b, int i) {
    const float* p = a.x + (long)b * a.x_sb + 3L * i;
    const float X = p[0], Y = p[1], Z = p[2];
    const float* k = a.intr + 4L * b;
    const float fx = k[0], fy = k[1], cx = k[2], cy = k[3];
    FsTerm r = {SH_FS_OUTSIDE, 0.f, 0.f, 0.f, 0.f};
    if (!(Z > 0.f)) return r;                                            // a NaN included
    const float uf = (X * fx) / Z + cx, vf = (Y * fy) / Z + cy;
    const bool inside = uf >= -0.5f && uf < (float)a.W - 0.5f && vf >= -0.5f && vf < (float)a.H - 0.5f;   // a NaN is outside
    if (!inside) return r;
    const int u = min((int)floorf(uf + 0.5f), a.W - 1), v = min((int)floorf(vf + 0.5f), a.H - 1);        // the min never binds: no read beyond the image whatever the rounding
    const long px = ((long)b * a.H + v) * a.W + u;
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
            const float ra = ((float)uq - cx) / fx, rb = ((float)vq - cy) / fy;
            const float rx = X - ra * Z, ry = Y - rb * Z;
            r.kind = SH_FS_SILHOUETTE;
            r.term = rx * rx + ry * ry;
            r.gx = 2.f * rx;
            r.gy = 2.f * ry;
            r.gz = -2.f * (ra * rx + rb * ry);
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

// grid (body).  Thread t takes the vertices t, t + 256, ... in order: term and kind are stored, the two sums kept in fp64; then
// the wave butterfly and the four wave sums in order - the order of chamfer_fwd_kernel.
__global__ __launch_bounds__(256) void free_space_fwd_kernel(FsArgs a, float* __restrict__ term, uint8_t* __restrict__ kind,
                                                            float* __restrict__ loss, int32_t* __restrict__ counts) {
    __shared__ double red[2][4];
    __shared__ int redi[4][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t* mb = a.v_mask ? a.v_mask + (long)b * a.mask_sb : nullptr;
    double s1 = 0.0, s2 = 0.0;
    int na = 0, k1 = 0, k2 = 0, k4 = 0;
    for (int i = tid; i < a.n; i += 256) {
        FsTerm r = {SH_FS_NONE, 0.f, 0.f, 0.f, 0.f};
        if (!mb || mb[i] != 0) {
            ++na;
            r = fs_term(a, b, i);
        }
        term[(long)b * a.n + i] = r.term;
        kind[(long)b * a.n + i] = (uint8_t)r.kind;
        if (r.kind == SH_FS_FREE) { s1 += (double)r.term; ++k1; }
        if (r.kind == SH_FS_SILHOUETTE) { s2 += (double)r.term; ++k2; }
        k4 += r.kind == SH_FS_OUTSIDE;
    }
    s1 = wave_sum_d(s1); s2 = wave_sum_d(s2);
    na = wave_sum_i(na); k1 = wave_sum_i(k1); k2 = wave_sum_i(k2); k4 = wave_sum_i(k4);
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        red[0][w] = s1; red[1][w] = s2;
        redi[0][w] = na; redi[1][w] = k1; redi[2][w] = k2; redi[3][w] = k4;
    }
    __syncthreads();
    if (tid == 0) {
        double t1 = 0.0, t2 = 0.0;
        int c[4] = {0, 0, 0, 0};
        for (int w = 0; w < 4; ++w) {
            t1 += red[0][w]; t2 += red[1][w];
            for (int j = 0; j < 4; ++j) c[j] += redi[j][w];
        }
        loss[2 * b] = c[0] > 0 ? (float)(t1 / (double)c[0]) : 0.f;
        loss[2 * b + 1] = c[0] > 0 ? (float)(t2 / (double)c[0]) : 0.f;
        for (int j = 0; j < 4; ++j) counts[4 * b + j] = c[j];
    }
}

// grid (row tile of 256, body), thread = one row of g_x: the vertex's case list once more, its gradient times
// fl(gL[b][k] * fl(1 / n_act)); zeros for every row without a term.
__global__ __launch_bounds__(256) void free_space_bwd_kernel(FsArgs a, int rows, const int32_t* __restrict__ counts, const float* __restrict__ gL,
                                                            float* __restrict__ g_x) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (i < a.n && (!a.v_mask || a.v_mask[(long)b * a.mask_sb + i] != 0)) {
        const FsTerm r = fs_term(a, b, i);
        if (r.kind == SH_FS_FREE || r.kind == SH_FS_SILHOUETTE) {
            const float inv = 1.f / (float)counts[4 * b];                // n_act >= 1: this vertex is active
            const float s = gL[2 * b + (r.kind == SH_FS_SILHOUETTE)] * inv;
            g0 = s * r.gx; g1 = s * r.gy; g2 = s * r.gz;
        }
    }
    float* o = g_x + ((long)b * rows + i) * 3;
    o[0] = g0; o[1] = g1; o[2] = g2;
}

// What both entry points ask of the arguments they share.
int check_args(const char* who, const float* x, int64_t x_sb, int rows, int n, const uint8_t* cls, const float* z, const int32_t* nearest,
               const float* intr, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, int B) {
    SH_REQUIRE(x && cls && z && nearest && intr, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(B >= 0 && H >= 0 && W >= 0 && rows >= 0 && n >= 0 && n <= rows, SH_ERR_INVALID_ARG,
               "%s: bad size (B %d, H %d, W %d, rows %d, n %d)", who, B, H, W, rows, n);
    SH_REQUIRE(margin >= 0.f, SH_ERR_INVALID_ARG, "%s: margin must be >= 0 (and not NaN)", who);
    SH_REQUIRE(B <= 1 || x_sb >= 3L * n, SH_ERR_INVALID_ARG, "%s: batch stride %ld shorter than a body", who, (long)x_sb);
    SH_REQUIRE(!v_mask || mask_sb == 0 || mask_sb >= n, SH_ERR_INVALID_ARG, "%s: mask stride %ld shorter than n", who, (long)mask_sb);
    SH_REQUIRE(H <= SH_FIELD_MAX_SIDE && W <= SH_FIELD_MAX_SIDE && B <= 65535, SH_ERR_UNSUPPORTED, "%s: H and W must not exceed %d (B 65535)", who,
               SH_FIELD_MAX_SIDE);
    SH_REQUIRE((n == 0) || (H > 0 && W > 0), SH_ERR_INVALID_ARG, "%s: an empty image (H %d, W %d)", who, H, W);
    return SH_OK;
}

}  // namespace

extern "C" {

int sh_free_space_fwd(const float* x, int64_t x_sb, int rows, int n, const uint8_t* cls, const float* z, const int32_t* nearest,
                      const float* intr, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, int B, float* term, uint8_t* kind,
                      float* loss, int32_t* counts, sh_stream_t stream) {
    if (const int rc = check_args("sh_free_space_fwd", x, x_sb, rows, n, cls, z, nearest, intr, H, W, v_mask, mask_sb, margin, B)) return rc;
    SH_REQUIRE(term && kind && loss && counts, SH_ERR_INVALID_ARG, "sh_free_space_fwd: null pointer");
    if (B == 0) return SH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FsArgs a = {x, (long)x_sb, n, cls, z, nearest, intr, H, W, v_mask, (long)mask_sb, margin};
    ShProfScope ps(st, "free_space_fwd_kernel|B=%d n=%d H=%d W=%d", B, n, H, W);
    SH_LAUNCH_PS(ps, free_space_fwd_kernel, dim3((unsigned)B), dim3(256), 0, st, a, term, kind, loss, counts);
    SH_CHECK_LAUNCH("free_space_fwd");
    return SH_OK;
}

int sh_free_space_bwd(const float* x, int64_t x_sb, int rows, int n, const uint8_t* cls, const float* z, const int32_t* nearest,
                      const float* intr, int H, int W, const uint8_t* v_mask, int64_t mask_sb, float margin, const int32_t* counts,
                      const float* gL, int B, float* g_x, sh_stream_t stream) {
    if (const int rc = check_args("sh_free_space_bwd", x, x_sb, rows, n, cls, z, nearest, intr, H, W, v_mask, mask_sb, margin, B)) return rc;
    SH_REQUIRE(counts && gL && g_x, SH_ERR_INVALID_ARG, "sh_free_space_bwd: null pointer");
    if (B == 0 || rows == 0) return SH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FsArgs a = {x, (long)x_sb, n, cls, z, nearest, intr, H, W, v_mask, (long)mask_sb, margin};
    ShProfScope ps(st, "free_space_bwd_kernel|B=%d rows=%d n=%d", B, rows, n);
    SH_LAUNCH_PS(ps, free_space_bwd_kernel, dim3((unsigned)sh_cdiv(rows, 256), (unsigned)B), dim3(256), 0, st, a, rows, counts, gL, g_x);
    SH_CHECK_LAUNCH("free_space_bwd");
    return SH_OK;
}

}  // extern "C"
