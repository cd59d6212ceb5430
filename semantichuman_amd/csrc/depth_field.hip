// The depth field (include/sh_kernels.h, "Depth field"): per pixel of a depth image its class (EMPTY / UNKNOWN / SURFACE), the
// surface depth, and the exact feature transform of the pixels that are not EMPTY - what the free-space and silhouette terms of
// free_space.hip read.  The reference has no counterpart.  Two passes, no atomics, every output element one plain store: a column
// pass that classifies and leaves one candidate per (pixel, column), and a row pass that takes the lexicographic minimum of
// (d2, v', u') over a row's candidates from LDS.
#include "sh_depth.h"

namespace {

constexpr int COL_NT = 64;              // column pass: one wave, thread = one column, coalesced across u
constexpr int ROW_NT = 256;             // row pass: one workgroup per image row

struct FieldArgs {
    const void* depth; const uint8_t* mask;
    int H, W;
    float depth_scale, z_near, z_far;
};

// grid (columns / 64, body).  Down the column: the pixel's class and z, and the row of the nearest allowed (cls != 0) pixel at or
// above it.  Up again: the nearest at or below, and of the two the closer one - a tie goes to the upper, the smaller index.
// cand[b][v][u] = that row, -1 when the column has no allowed pixel.  One candidate per column is enough for the lexicographic
// rule: within a column d2 and the index both grow with |v - v'| and, at equal |v - v'|, the upper row has the smaller index.
template <typename T>
__global__ __launch_bounds__(COL_NT) void depth_field_column_kernel(FieldArgs a, uint8_t* __restrict__ cls, float* __restrict__ zout,
                                                                    int16_t* __restrict__ cand) {
    const int u = blockIdx.x * COL_NT + threadIdx.x, b = blockIdx.y;
    if (u >= a.W) return;
    const long body = (long)b * a.H * a.W;
    const T* d = static_cast<const T*>(a.depth) + body;
    const uint8_t* m = a.mask ? a.mask + body : nullptr;
    int up = -1;
    for (int v = 0; v < a.H; ++v) {
        const long p = (long)v * a.W + u;
        const T raw = d[p];
        const float z = depth_z(raw, a.depth_scale);
        const bool valid = depth_valid(raw, z, a.z_near, a.z_far, m, p);
        const bool empty = !valid && depth_reading(raw, z) && z >= a.z_near;
        cls[body + p] = valid ? SH_FIELD_SURFACE : empty ? SH_FIELD_EMPTY : SH_FIELD_UNKNOWN;
        zout[body + p] = valid ? z : 0.f;
        up = empty ? up : v;
        cand[body + p] = (int16_t)up;
    }
    int down = -1;
    for (int v = a.H - 1; v >= 0; --v) {
        const long p = body + (long)v * a.W + u;
        const int above = cand[p];                                       // this thread's own store
        down = above == v ? v : down;                                    // allowed here: its own nearest
        const bool take_up = above >= 0 && (down < 0 || v - above <= down - v);
        cand[p] = (int16_t)(take_up ? above : down);
    }
}

// grid (row, body), dynamic LDS = W int16: the row's candidates.  Pixel (u, v) walks outward from its own column, k = 0, 1, ...,
// looks at columns u - k and u + k, keeps the smallest key (d2 << 32 | v' * W + u') and leaves once k * k exceeds the best d2: a
// column at distance k cannot hold anything closer, and at k * k == best it can still hold a tie of smaller index.
__global__ __launch_bounds__(ROW_NT) void depth_field_row_kernel(const int16_t* __restrict__ cand, int H, int W, int32_t* __restrict__ nearest) {
    extern __shared__ int16_t rows[];
    const int v = blockIdx.x, b = blockIdx.y;
    const long base = ((long)b * H + v) * W;
    for (int u = threadIdx.x; u < W; u += ROW_NT) rows[u] = cand[base + u];
    __syncthreads();
    for (int u = threadIdx.x; u < W; u += ROW_NT) {
        unsigned long long best = ~0ull;
        auto look = [&](int c, int k) {
            const int r = rows[c];
            if (r < 0) return;
            const int dy = v - r;
            const unsigned long long key = ((unsigned long long)(unsigned)(dy * dy + k * k) << 32) | (unsigned)(r * W + c);
            best = key < best ? key : best;
        };
        for (int k = 0; (unsigned)(k * k) <= (unsigned)(best >> 32); ++k) {
            const int lo = u - k, hi = u + k;
            if (lo < 0 && hi >= W) break;
            if (lo >= 0) look(lo, k);
            if (k > 0 && hi < W) look(hi, k);
        }
        nearest[base + u] = best == ~0ull ? -1 : (int32_t)(best & 0xffffffffull);
    }
}

}  // namespace

extern "C" {

size_t sh_depth_field_workspace(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * H * W * sizeof(int16_t);
}

int sh_depth_field(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W, float z_near,
                   float z_far, uint8_t* cls, float* z, int32_t* nearest, void* workspace, size_t workspace_bytes, sh_stream_t stream) {
    if (const int rc = depth_check_inputs("sh_depth_field", depth, dtype, intr, B, H, W)) return rc;
    SH_REQUIRE(cls && z && nearest, SH_ERR_INVALID_ARG, "sh_depth_field: null pointer");
    SH_REQUIRE(H <= SH_FIELD_MAX_SIDE && W <= SH_FIELD_MAX_SIDE && B <= 65535, SH_ERR_UNSUPPORTED,
               "sh_depth_field: H and W must not exceed %d (B 65535): got B %d, H %d, W %d", SH_FIELD_MAX_SIDE, B, H, W);
    if (B == 0 || H == 0 || W == 0) return SH_OK;
    const size_t need = sh_depth_field_workspace(B, H, W);
    SH_REQUIRE(workspace && workspace_bytes >= need, SH_ERR_INVALID_ARG, "sh_depth_field: the workspace holds the column candidates (%zu bytes needed)",
               need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const FieldArgs a = {depth, mask, H, W, depth_scale, z_near, z_far};
    int16_t* cand = static_cast<int16_t*>(workspace);
    {
        ShProfScope ps(st, "depth_field_column_kernel|B=%d H=%d W=%d u16=%d", B, H, W, dtype == SH_DEPTH_U16);
        const dim3 grid((unsigned)sh_cdiv(W, COL_NT), (unsigned)B);
        if (dtype == SH_DEPTH_U16) SH_LAUNCH_PS(ps, depth_field_column_kernel<uint16_t>, grid, dim3(COL_NT), 0, st, a, cls, z, cand);
        else SH_LAUNCH_PS(ps, depth_field_column_kernel<float>, grid, dim3(COL_NT), 0, st, a, cls, z, cand);
    }
    {
        ShProfScope ps(st, "depth_field_row_kernel|B=%d H=%d W=%d", B, H, W);
        const size_t lds = ((size_t)W * sizeof(int16_t) + 15) & ~(size_t)15;          // at most 32 KiB
        SH_LAUNCH_PS(ps, depth_field_row_kernel, dim3((unsigned)H, (unsigned)B), dim3(ROW_NT), lds, st, cand, H, W, nearest);
    }
    SH_CHECK_LAUNCH("depth_field");
    return SH_OK;
}

}  // extern "C"
