// Depth images as scans (include/sh_kernels.h, "Depth images"): per pixel the camera-frame point, the normal from the grid
// neighbours, and the kept pixels packed per body in tile / Z-order.  The reference has no counterpart.  One workgroup per
// 16 x 16 tile, thread = Z-rank inside the tile, so the ballot prefix of "kept" IS the rank among the tile's rows: a count pass,
// a per-body scan of the tile counts and an emit pass that recomputes the pixel - no atomics, every output element one plain
// store, nothing that depends on the batch, the padding or the launch shape.
// Also what follows the rig form of it: "Depth views: overlap" - per packed row, which other cameras measure the same surface point
// and whether one of them is better placed - and "Scan compaction", the same three passes over 256-row chunks under a keep plane.
#include "sh_depth.h"

#pragma clang fp contract(off)          // the header's expressions: every operation rounded on its own, in the whole file

namespace {

constexpr int TILE = SH_DEPTH_TILE;
constexpr int NT = TILE * TILE;         // threads per workgroup: one per pixel of the tile
constexpr int HALO = TILE + 2;          // the tile with one pixel around it
// LDS row stride in floats.  The 32 lanes of one ds_read_b32 group are ranks 32 g .. 32 g + 31 = 8 columns x 4 rows of the tile:
// with 24 the four rows start at banks 0, 24, 16, 8 - no two lanes on one bank, for the centre and for every neighbour (a
// uniform shift).  With 18 rows 0 / 2 and 1 / 3 would share four banks each.
constexpr int LROW = 24;
static_assert(TILE == 16, "the Z-rank below is 4 + 4 bits");

struct DepthArgs {
    const void* depth; const float* intr; const uint8_t* mask;
    int H, W, tiles_x, tiles;
    float depth_scale, z_near, z_far, max_step;
    int drop_isolated, stride;
};
// The rig form ("Depth views"): V images per body, each with its camera -> rig transform; ext == nullptr: one camera, its own frame.
struct ViewArgs {
    const float* ext;                   // [B][V][12], R row-major then t; a NaN anywhere in a row: the view is absent
    int V;
    uint8_t* view;                      // [B][M], the view a row came from, 255 in the padding
    int32_t* view_first;                // [B][V + 1]
};
// "Camera rays": the pixel -> ray table of a calibrated camera, fp32 [images][H][W][2]; image (b, view) is table image
// b * stride + view, or with stride == 0 just view - one table per camera, shared by all bodies.
struct RayArgs { const float* rays; int stride; };
struct P3 { float x, y, z; };

// bits 0, 2, 4, 6 of r -> a 4-bit number: the u of a Z-rank (its v: the same of r >> 1)
__device__ __forceinline__ int even_bits(int r) {
    r &= 0x55;
    r = (r | (r >> 1)) & 0x33;
    return (r | (r >> 2)) & 0x0f;
}

// The tile at (u0, v0) with its halo -> zt[HALO][LROW]: z where the pixel is valid, NaN where it is not or lies outside the
// image.  Consecutive threads read consecutive pixels of a row.
template <typename T>
__device__ __forceinline__ void load_tile(const DepthArgs& a, int b, int u0, int v0, float* zt) {
    const long body = (long)b * a.H * a.W;
    const T* d = static_cast<const T*>(a.depth) + body;
    const uint8_t* m = a.mask ? a.mask + body : nullptr;
    for (int i = threadIdx.x; i < HALO * HALO; i += NT) {
        const int r = i / HALO, c = i - r * HALO;
        const int u = u0 - 1 + c, v = v0 - 1 + r;
        float z = NAN;
        if (u >= 0 && u < a.W && v >= 0 && v < a.H) {
            const long p = (long)v * a.W + u;
            const T raw = d[p];
            const float zz = depth_z(raw, a.depth_scale);
            z = depth_valid(raw, zz, a.z_near, a.z_far, m, p) ? zz : NAN;
        }
        zt[r * LROW + c] = z;
    }
}

__device__ __forceinline__ P3 unproject(int u, int v, float z, float fx, float fy, float cx, float cy) {
    return {(((float)u - cx) * z) / fx, (((float)v - cy) * z) / fy, z};
}

// The rays of the tile at (u0, v0) with its halo -> ra, rb [HALO][LROW], in the layout of zt: the same 32 lanes read the same
// offsets of each plane, so LROW's bank reasoning holds for both.  One 8-byte read per pixel, consecutive threads consecutive
// pixels of a row; NaN outside the image, where zt holds a NaN too and no tangent is taken.
__device__ __forceinline__ void load_rays(const float* table, int H, int W, int u0, int v0, float* ra, float* rb) {
    const float2* t = reinterpret_cast<const float2*>(table);
    for (int i = threadIdx.x; i < HALO * HALO; i += NT) {
        const int r = i / HALO, c = i - r * HALO;
        const int u = u0 - 1 + c, v = v0 - 1 + r;
        float2 q = {NAN, NAN};
        if (u >= 0 && u < W && v >= 0 && v < H) q = t[(long)v * W + u];
        ra[r * LROW + c] = q.x;
        rb[r * LROW + c] = q.y;
    }
}

// "Camera rays": the point of a pixel with ray (a, b) at depth z.
__device__ __forceinline__ P3 unproject_ray(float a, float b, float z) { return {a * z, b * z, z}; }

// The header's tangent rule over the lower and upper neighbour of c: hi - lo, else hi - c, else c - lo; false: none.
__device__ __forceinline__ bool tangent(const P3& lo, bool has_lo, const P3& c, const P3& hi, bool has_hi, P3& t) {
    const P3 a = has_hi ? hi : c, b = has_lo ? lo : c;
    t = {a.x - b.x, a.y - b.y, a.z - b.z};
    return has_lo || has_hi;
}

// grid (tile, image).  EMIT = false, the count pass: tile_row[image][tile] = the tile's kept pixels.  EMIT = true: tile_row holds the
// tile's first row (depth_scan_kernel), and the kept pixels and the body's padding are written.  VIEWS = false: an image is a
// body.  VIEWS = true: image = body * V + view, a body's rows are its views' in turn - tile_row [B][V][tiles] is scanned per body -
// and the emit pass moves point and normal into the rig's frame; an absent view enters as a tile of NaN: nothing kept, nothing
// of it read.  RAYS: the five points come from the camera's ray table (ry), staged in LDS next to zt with the same halo, not
// from the intrinsics, which are then not read; everything after the points is the same text.
template <typename T, bool EMIT, bool VIEWS, bool RAYS>
__global__ __launch_bounds__(NT) void depth_kernel(DepthArgs a, ViewArgs va, int32_t* __restrict__ tile_row, const int32_t* __restrict__ counts,
                                                  int M, float* __restrict__ points, float* __restrict__ normals, int32_t* __restrict__ pixel,
                                                  RayArgs ry) {
    __shared__ float zt[HALO * LROW];
    __shared__ float rt[RAYS ? 2 * HALO * LROW : 1];
    __shared__ int wsum[NT / 64];
    const int tile = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const int b = VIEWS ? img / va.V : img, view = VIEWS ? img - b * va.V : 0;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    float e[12] = {};
    bool present = true;                                                 // uniform
    if (VIEWS) {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            e[k] = va.ext[12L * img + k];
            present = present && e[k] == e[k];
        }
    }
    if (present) load_tile<T>(a, img, tx * TILE, ty * TILE, zt);
    else for (int i = tid; i < HALO * LROW; i += NT) zt[i] = NAN;
    if constexpr (RAYS) {
        if ((EMIT || a.drop_isolated) && present)                        // uniform; the condition under which the points are formed
            load_rays(ry.rays + 2L * a.H * a.W * (ry.stride ? (long)b * ry.stride + view : (long)view), a.H, a.W, tx * TILE, ty * TILE, rt,
                      rt + HALO * LROW);
    }
    __syncthreads();
    const int lu = even_bits(tid), lv = even_bits(tid >> 1);
    const int u = tx * TILE + lu, v = ty * TILE + lv;
    const float* zc = zt + (lv + 1) * LROW + (lu + 1);
    const float z = zc[0];
    const bool valid = z == z;                                           // NaN: not valid, or outside the image
    bool kept = valid && u % a.stride == 0 && v % a.stride == 0;
    P3 p = {0.f, 0.f, 0.f};
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if ((EMIT || a.drop_isolated) && present) {                          // uniform
        const float zl = zc[-1], zr = zc[1], zu = zc[-LROW], zd = zc[LROW];
        P3 pl, pr, pu, pd;
        if constexpr (RAYS) {
            const float* ac = rt + (lv + 1) * LROW + (lu + 1);
            const float* bc = ac + HALO * LROW;
            p = unproject_ray(ac[0], bc[0], z);
            pl = unproject_ray(ac[-1], bc[-1], zl); pr = unproject_ray(ac[1], bc[1], zr);
            pu = unproject_ray(ac[-LROW], bc[-LROW], zu); pd = unproject_ray(ac[LROW], bc[LROW], zd);
        } else {
            const float* k = a.intr + 4L * img;
            const float fx = k[0], fy = k[1], cx = k[2], cy = k[3];
            p = unproject(u, v, z, fx, fy, cx, cy);
            pl = unproject(u - 1, v, zl, fx, fy, cx, cy); pr = unproject(u + 1, v, zr, fx, fy, cx, cy);
            pu = unproject(u, v - 1, zu, fx, fy, cx, cy); pd = unproject(u, v + 1, zd, fx, fy, cx, cy);
        }
        P3 dx, dy;                                                       // usable: the compare is false for a NaN on either side
        const bool has_dx = tangent(pl, fabsf(zl - z) <= a.max_step, p, pr, fabsf(zr - z) <= a.max_step, dx);
        const bool has_dy = tangent(pu, fabsf(zu - z) <= a.max_step, p, pd, fabsf(zd - z) <= a.max_step, dy);
        const double ax = dx.x, ay = dx.y, az = dx.z, bx = dy.x, by = dy.y, bz = dy.z;
        const double c0 = ay * bz - az * by, c1 = az * bx - ax * bz, c2 = ax * by - ay * bx;
        const double len2 = (c0 * c0 + c1 * c1) + c2 * c2;
        const bool known = valid && has_dx && has_dy && len2 > 0.0;      // a NaN compares false
        const double len = sqrt(len2);
        const bool away = (c0 * (double)p.x + c1 * (double)p.y) + c2 * (double)p.z > 0.0;
        const double n0 = c0 / len, n1 = c1 / len, n2 = c2 / len;
        const double m0 = away ? -n0 : n0, m1 = away ? -n1 : n1, m2 = away ? -n2 : n2;
        if (VIEWS && EMIT) {                                             // "Depth views": the point in fp32, the normal in fp64 from the unrounded n
            nx = known ? (float)(((double)e[0] * m0 + (double)e[1] * m1) + (double)e[2] * m2) : 0.f;
            ny = known ? (float)(((double)e[3] * m0 + (double)e[4] * m1) + (double)e[5] * m2) : 0.f;
            nz = known ? (float)(((double)e[6] * m0 + (double)e[7] * m1) + (double)e[8] * m2) : 0.f;
            const P3 c = p;
            p.x = ((e[0] * c.x + e[1] * c.y) + e[2] * c.z) + e[9];
            p.y = ((e[3] * c.x + e[4] * c.y) + e[5] * c.z) + e[10];
            p.z = ((e[6] * c.x + e[7] * c.y) + e[8] * c.z) + e[11];
        } else {
            nx = known ? (float)m0 : 0.f;
            ny = known ? (float)m1 : 0.f;
            nz = known ? (float)m2 : 0.f;
        }
        if (a.drop_isolated) kept = kept && known;
    }
    // rank among the tile's kept pixels: lanes below in the wave (ballot), waves below in the workgroup (LDS)
    const int lane = tid & 63, w = sh_wave_id();
    const unsigned long long bal = __ballot(kept);
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const int s = wsum[i];
        before += i < w ? s : 0;
        total += s;
    }
    const long slot = (long)img * a.tiles + tile;
    if (!EMIT) {
        if (tid == 0) tile_row[slot] = total;
        return;
    }
    const long body = (long)b * M;
    if (VIEWS && tile == 0 && tid == 0) {                                // the view's first row; the last view also closes the list
        va.view_first[(long)b * (va.V + 1) + view] = tile_row[slot];
        if (view == va.V - 1) va.view_first[(long)b * (va.V + 1) + va.V] = counts[b];
    }
    if (kept) {
        const int row = tile_row[slot] + before + __popcll(bal & ((1ull << lane) - 1ull));
        if (row < M) {                                                   // holds whenever M >= the count; never a store beyond the body
            const long o = body + row;
            points[3 * o] = p.x; points[3 * o + 1] = p.y; points[3 * o + 2] = p.z;
            normals[3 * o] = nx; normals[3 * o + 1] = ny; normals[3 * o + 2] = nz;
            pixel[o] = v * a.W + u;
            if (VIEWS) va.view[o] = (uint8_t)view;
        }
    }
    // the padding rows of the body, shared out over its workgroups
    const long wg = VIEWS ? (long)view * a.tiles + tile : tile, wgs = VIEWS ? (long)va.V * a.tiles : a.tiles;
    for (long j = (long)max(counts[b], 0) + wg * NT + tid; j < M; j += wgs * NT) {
        const long o = body + j;
        points[3 * o] = 0.f; points[3 * o + 1] = 0.f; points[3 * o + 2] = 0.f;
        normals[3 * o] = 0.f; normals[3 * o + 1] = 0.f; normals[3 * o + 2] = 0.f;
        pixel[o] = -1;
        if (VIEWS) va.view[o] = 255;
    }
}

// grid (body).  tile_row[b][0 .. tiles): counts -> their exclusive prefix sums, in place; counts[b] = the total.  256 tiles per
// round: an inclusive wave scan by shuffles, the wave totals through LDS, the carry in a register.  Integer sums: no order.
__global__ __launch_bounds__(NT) void depth_scan_kernel(int32_t* __restrict__ tile_row, int tiles, int32_t* __restrict__ counts) {
    __shared__ int wsum[NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = sh_wave_id();
    int32_t* t = tile_row + (long)b * tiles;
    int carry = 0;
    for (int base = 0; base < tiles; base += NT) {                       // uniform
        const int i = base + tid;
        const int own = i < tiles ? t[i] : 0;
        int s = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int below = __shfl_up(s, o, 64);
            s += lane >= o ? below : 0;
        }
        if (lane == 63) wsum[w] = s;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) {
            const int ws = wsum[k];
            before += k < w ? ws : 0;
            total += ws;
        }
        if (i < tiles) t[i] = carry + before + s - own;
        carry += total;
        __syncthreads();                                                 // wsum is rewritten in the next round
    }
    if (tid == 0) counts[b] = carry;
}

// ---------------------------------------------------------------------------------------------- "Depth views: overlap"
struct OverlapArgs {
    const void* depth; const float* intr; const uint8_t* mask; const float* ext;
    int V, H, W;
    float depth_scale, z_near, z_far, tol;
    const float* points; const float* normals; const uint8_t* view; const int32_t* counts;
    int M;
};
// "Camera rays": the distortion coefficients [images][8] and fold-back limits [images] of the cameras, images as in RayArgs.
struct DistArgs { const float* dist; const float* limit; int stride; };
constexpr int DIST_WORDS = 9;           // a view's record in LDS: the 8 coefficients, then the limit

// The header's q of a row (point P, normal n) under the camera centre t: cos^2 / d^4 with the sign of the cosine.
__device__ __forceinline__ float view_quality(const P3& P, const P3& n, const float* t) {
    const float ex = t[0] - P.x, ey = t[1] - P.y, ez = t[2] - P.z;
    const float len2 = (ex * ex + ey * ey) + ez * ez;
    const float dot = (n.x * ex + n.y * ey) + n.z * ez;
    return len2 == 0.f ? 0.f : (dot * fabsf(dot)) / ((len2 * len2) * len2);
}

// grid (256-row chunk, body), thread = one row.  The body's V extrinsics and intrinsics are staged in LDS once per workgroup
// (an absent view: its intrinsics are not read); every view is then a uniform loop step whose LDS reads are broadcasts.  One
// scattered depth (and mask) read per row and other view that has the point in front of it and inside its image.  RAYS: the
// projection is the distorted one of "Camera rays"; a present view's coefficients and limit are staged next to sk.
template <typename T, bool RAYS>
__global__ __launch_bounds__(NT) void depth_views_overlap_kernel(OverlapArgs a, uint32_t* __restrict__ seen, uint8_t* __restrict__ keep, DistArgs da) {
    __shared__ float se[SH_DEPTH_MAX_VIEWS * 12];
    __shared__ float sk[SH_DEPTH_MAX_VIEWS * 4];
    __shared__ float sd[RAYS ? SH_DEPTH_MAX_VIEWS * DIST_WORDS : 1];
    __shared__ int present[SH_DEPTH_MAX_VIEWS];
    const int b = blockIdx.y, tid = threadIdx.x;
    for (int i = tid; i < a.V * 12; i += NT) se[i] = a.ext[12L * b * a.V + i];
    __syncthreads();
    if (tid < a.V) {
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 12; ++k) ok = ok && se[12 * tid + k] == se[12 * tid + k];
        present[tid] = ok;
#pragma unroll
        for (int k = 0; k < 4; ++k) sk[4 * tid + k] = ok ? a.intr[4L * ((long)b * a.V + tid) + k] : 0.f;
        if constexpr (RAYS) {
            const long cam = da.stride ? (long)b * da.stride + tid : (long)tid;
#pragma unroll
            for (int k = 0; k < 8; ++k) sd[DIST_WORDS * tid + k] = ok ? da.dist[8 * cam + k] : 0.f;
            sd[DIST_WORDS * tid + 8] = ok ? da.limit[cam] : 0.f;
        }
    }
    __syncthreads();
    const long j = (long)blockIdx.x * NT + tid;
    if (j >= a.M) return;
    const long o = (long)b * a.M + j;
    uint32_t bits = 0;
    bool kp = false;
    if (j < a.counts[b]) {
        const P3 P = {a.points[3 * o], a.points[3 * o + 1], a.points[3 * o + 2]};
        const P3 n = {a.normals[3 * o], a.normals[3 * o + 1], a.normals[3 * o + 2]};
        const int own = a.view[o];
        const float q_own = own < a.V ? view_quality(P, n, se + 12 * own + 9) : 0.f;   // an absent own view (no live row has one): NaN, every compare false
        bits = own < 32 ? 1u << own : 0u;
        kp = true;
        const long image = (long)a.H * a.W;
        for (int c = 0; c < a.V; ++c) {                                  // uniform
            if (!present[c] || c == own) continue;
            const float* e = se + 12 * c;
            const float d0 = P.x - e[9], d1 = P.y - e[10], d2 = P.z - e[11];
            const float X = (e[0] * d0 + e[3] * d1) + e[6] * d2;
            const float Y = (e[1] * d0 + e[4] * d1) + e[7] * d2;
            const float Z = (e[2] * d0 + e[5] * d1) + e[8] * d2;
            if (!(Z > 0.f)) continue;                                    // a NaN included
            float uf, vf;                                                // sh_free_space_fwd's projection, inside test and rounding
            if constexpr (RAYS) {
                if (!camera_project(X, Y, Z, sk + 4 * c, sd + DIST_WORDS * c, sd[DIST_WORDS * c + 8], uf, vf)) continue;
            } else {
                const float fx = sk[4 * c], fy = sk[4 * c + 1], cx = sk[4 * c + 2], cy = sk[4 * c + 3];
                uf = (X * fx) / Z + cx; vf = (Y * fy) / Z + cy;
            }
            const bool inside = uf >= -0.5f && uf < (float)a.W - 0.5f && vf >= -0.5f && vf < (float)a.H - 0.5f;   // a NaN is outside
            if (!inside) continue;
            const int u = min((int)floorf(uf + 0.5f), a.W - 1), v = min((int)floorf(vf + 0.5f), a.H - 1);        // no read beyond the image whatever the rounding
            const long p = ((long)b * a.V + c) * image + (long)v * a.W + u;
            const T raw = static_cast<const T*>(a.depth)[p];
            const float zc = depth_z(raw, a.depth_scale);
            if (!(depth_valid(raw, zc, a.z_near, a.z_far, a.mask, p) && fabsf(zc - Z) <= a.tol)) continue;
            bits |= 1u << c;
            const float q = view_quality(P, n, e + 9);
            if (q > q_own || (q == q_own && c < own)) kp = false;
        }
    }
    seen[o] = bits;
    keep[o] = kp ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- "Scan compaction"
struct CompactArgs {
    const float* points; const float* normals; const int32_t* pixel; const uint8_t* view; const uint32_t* seen; const uint8_t* keep;
    const int32_t* counts;
    int V, M, chunks, M_out;
};
struct CompactOut { float* points; float* normals; int32_t* pixel; uint8_t* view; uint32_t* seen; int32_t* view_first; };

// grid (256-row chunk, body), thread = one row: the three passes of depth_kernel with a chunk of rows for a tile.  EMIT = false:
// chunk_row[body][chunk] = the chunk's kept rows.  EMIT = true: chunk_row holds the chunk's first output row and counts_out the
// body's total (depth_scan_kernel); a kept row moves to that plus its ballot rank - the old order -, the body's workgroups
// share out its padding, and view_first_out comes from the rows where `view` steps (the input is view-major): the kept rows
// before that row are the first row of every view in the step, and the last live row closes the list.
template <bool EMIT>
__global__ __launch_bounds__(NT) void scan_compact_kernel(CompactArgs a, CompactOut out, int32_t* __restrict__ chunk_row,
                                                         const int32_t* __restrict__ counts_out) {
    __shared__ int wsum[NT / 64];
    const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long j = (long)chunk * NT + tid;
    const int live_n = min(max(a.counts[b], 0), a.M);
    const bool live = j < live_n;
    const long in = (long)b * a.M + j;
    const bool kept = live && a.keep[in] != 0;
    const int lane = tid & 63, w = sh_wave_id();
    const unsigned long long bal = __ballot(kept);
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const int s = wsum[i];
        before += i < w ? s : 0;
        total += s;
    }
    const long slot = (long)b * a.chunks + chunk;
    if (!EMIT) {
        if (tid == 0) chunk_row[slot] = total;
        return;
    }
    const int row = chunk_row[slot] + before + __popcll(bal & ((1ull << lane) - 1ull));   // the kept rows before this one
    const int kept_n = counts_out[b];
    int32_t* first = out.view_first + (long)b * (a.V + 1);
    if (live) {
        const int own = a.view[in], prev = j == 0 ? -1 : (int)a.view[in - 1];
        for (int v = prev + 1; v <= own && v < a.V; ++v) first[v] = row;
        if (j == live_n - 1)
            for (int v = min(own + 1, a.V); v <= a.V; ++v) first[v] = kept_n;
    }
    if (live_n == 0 && chunk == 0 && tid <= a.V) first[tid] = 0;         // V + 1 <= 33 threads
    const long body = (long)b * a.M_out;
    if (kept && row < a.M_out) {                                         // holds whenever M_out >= the kept count; never a store beyond the body
        const long o = body + row;
        out.points[3 * o] = a.points[3 * in]; out.points[3 * o + 1] = a.points[3 * in + 1]; out.points[3 * o + 2] = a.points[3 * in + 2];
        out.normals[3 * o] = a.normals[3 * in]; out.normals[3 * o + 1] = a.normals[3 * in + 1]; out.normals[3 * o + 2] = a.normals[3 * in + 2];
        out.pixel[o] = a.pixel[in];
        out.view[o] = a.view[in];
        if (out.seen) out.seen[o] = a.seen[in];
    }
    for (long r = (long)max(kept_n, 0) + (long)chunk * NT + tid; r < a.M_out; r += (long)a.chunks * NT) {
        const long o = body + r;
        out.points[3 * o] = 0.f; out.points[3 * o + 1] = 0.f; out.points[3 * o + 2] = 0.f;
        out.normals[3 * o] = 0.f; out.normals[3 * o + 1] = 0.f; out.normals[3 * o + 2] = 0.f;
        out.pixel[o] = -1;
        out.view[o] = 255;
        if (out.seen) out.seen[o] = 0u;
    }
}

int compact_chunks(int M) { return M <= 0 ? 1 : (int)(((long)M + NT - 1) / NT); }   // at least one workgroup per body: it writes the padding

int tiles_of(int H, int W) { return sh_cdiv(H, TILE) * sh_cdiv(W, TILE); }

// What both entry points ask of the inputs they share; `who` names the caller in the message.
int check_inputs(const char* who, const void* depth, int dtype, const float* intr, int B, int H, int W, int stride) {
    if (const int rc = depth_check_inputs(who, depth, dtype, intr, B, H, W)) return rc;
    SH_REQUIRE(stride >= 1, SH_ERR_INVALID_ARG, "%s: stride = %d, must be at least 1", who, stride);
    SH_REQUIRE(B <= 65535 && (long)H * W <= INT_MAX, SH_ERR_UNSUPPORTED, "%s: B or H * W too large", who);
    return SH_OK;
}

// The same for the rig form: V images per body with their extrinsics.  int32 rows per body: V * H * W must fit.
int check_views(const char* who, const void* depth, int dtype, const float* intr, const float* ext, int B, int V, int H, int W, int stride) {
    SH_REQUIRE(ext, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(V >= 1 && V <= SH_DEPTH_MAX_VIEWS, SH_ERR_INVALID_ARG, "%s: V = %d views, must lie in [1, %d]", who, V, SH_DEPTH_MAX_VIEWS);
    if (const int rc = check_inputs(who, depth, dtype, intr, B, H, W, stride)) return rc;
    SH_REQUIRE((long)B * V <= 65535 && (long)V * H * W <= INT_MAX, SH_ERR_UNSUPPORTED, "%s: B * V or V * H * W too large", who);
    return SH_OK;
}

// One pass over the tiles of B bodies: of one image each (va.ext == nullptr, the record reads as before), or of va.V views each.
// With a ray table (RAYS) the record's name says so - "depth_rays_emit_kernel" - and carries the table's stride.
template <bool EMIT, bool VIEWS, bool RAYS>
void launch_tiles(hipStream_t st, int dtype, const DepthArgs& a, const ViewArgs& va, int B, int32_t* tile_row, const int32_t* counts, int M,
                  float* points, float* normals, int32_t* pixel, const RayArgs& ry) {
    char name[112];
    if (RAYS && VIEWS) snprintf(name, sizeof name, "%s|B=%d V=%d H=%d W=%d u16=%d tables=%d", EMIT ? "depth_views_rays_emit_kernel" : "depth_views_rays_count_kernel", B, va.V, a.H, a.W, dtype == SH_DEPTH_U16, ry.stride);
    else if (RAYS) snprintf(name, sizeof name, "%s|B=%d H=%d W=%d u16=%d tables=%d", EMIT ? "depth_rays_emit_kernel" : "depth_rays_count_kernel", B, a.H, a.W, dtype == SH_DEPTH_U16, ry.stride);
    else if (VIEWS) snprintf(name, sizeof name, "%s|B=%d V=%d H=%d W=%d u16=%d", EMIT ? "depth_views_emit_kernel" : "depth_views_count_kernel", B, va.V, a.H, a.W, dtype == SH_DEPTH_U16);
    else snprintf(name, sizeof name, "%s|B=%d H=%d W=%d u16=%d", EMIT ? "depth_emit_kernel" : "depth_count_kernel", B, a.H, a.W, dtype == SH_DEPTH_U16);
    ShProfScope ps(st, "%s", name);
    const dim3 grid((unsigned)a.tiles, (unsigned)(VIEWS ? B * va.V : B));
    if (dtype == SH_DEPTH_U16) SH_LAUNCH_PS(ps, (depth_kernel<uint16_t, EMIT, VIEWS, RAYS>), grid, dim3(NT), 0, st, a, va, tile_row, counts, M, points, normals, pixel, ry);
    else SH_LAUNCH_PS(ps, (depth_kernel<float, EMIT, VIEWS, RAYS>), grid, dim3(NT), 0, st, a, va, tile_row, counts, M, points, normals, pixel, ry);
}

// The tile rows of B bodies of `images` images each, in bytes: the workspace of both passes.
size_t tile_rows_bytes(int B, int images, int H, int W) { return (size_t)B * images * tiles_of(H, W) * sizeof(int32_t); }

// Everything behind the four entry points: the checks, the workspace need, the tiles and - for the count pass - the per-body scan.
// EMIT: the points pass, which reads counts and the workspace the count pass wrote.  VIEWS: a rig of V images per body with the
// extrinsics ext and the outputs view and view_first; else one camera: ext, view and view_first are null and V counts as 1.
// RAYS: the "Camera rays" form with the table `rays` of rays_stride images per body (0: one table per camera for all bodies);
// else both are null and 0.
template <bool EMIT, bool VIEWS, bool RAYS = false>
int depth_pass(const char* who, const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext, int B, int V,
               int H, int W, float z_near, float z_far, float max_step, int drop_isolated, int stride, int32_t* counts, int max_count, int M,
               void* workspace, size_t workspace_bytes, float* points, float* normals, int32_t* pixel, uint8_t* view, int32_t* view_first,
               sh_stream_t stream, const float* rays = nullptr, int rays_stride = 0) {
    if (RAYS) {
        SH_REQUIRE(rays, SH_ERR_INVALID_ARG, "%s: null pointer", who);
        SH_REQUIRE(rays_stride == 0 || rays_stride == (VIEWS ? V : 1), SH_ERR_INVALID_ARG, "%s: rays_stride = %d, must be 0 (one table per camera) or %d",
                   who, rays_stride, VIEWS ? V : 1);
    }
    if (const int rc = VIEWS ? check_views(who, depth, dtype, intr, ext, B, V, H, W, stride) : check_inputs(who, depth, dtype, intr, B, H, W, stride))
        return rc;
    SH_REQUIRE(counts && (!EMIT || (points && normals && pixel && (!VIEWS || (view && view_first)))), SH_ERR_INVALID_ARG, "%s: null pointer", who);
    if (EMIT) {
        SH_REQUIRE(M >= 0 && max_count >= 0, SH_ERR_INVALID_ARG, "%s: negative size (M %d, max_count %d)", who, M, max_count);
        SH_REQUIRE(M >= max_count, SH_ERR_INVALID_ARG, "%s: M = %d rows cannot hold the largest body's %d", who, M, max_count);
    }
    if (B == 0 || H == 0 || W == 0) return SH_OK;
    const int images = VIEWS ? V : 1;
    const size_t need = tile_rows_bytes(B, images, H, W);
    if (EMIT) {
        SH_REQUIRE(workspace && workspace_bytes >= need, SH_ERR_WORKSPACE, "%s: the workspace of %s is needed (%zu bytes)", who,
                   VIEWS ? "sh_depth_views_count" : "sh_depth_count", need);
    } else {
        SH_REQUIRE(workspace && workspace_bytes >= need, SH_ERR_WORKSPACE, "%s: the workspace holds the tile rows (%zu bytes needed)", who, need);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DepthArgs a = {depth, intr, mask, H, W, sh_cdiv(W, TILE), tiles_of(H, W), depth_scale, z_near, z_far, max_step, drop_isolated, stride};
    int32_t* tile_row = static_cast<int32_t*>(workspace);
    launch_tiles<EMIT, VIEWS, RAYS>(st, dtype, a, ViewArgs{ext, V, view, view_first}, B, tile_row, EMIT ? counts : nullptr, M, points, normals, pixel,
                                    RayArgs{rays, rays_stride});
    if (!EMIT) {
        ShProfScope ps(st, "depth_scan_kernel|B=%d tiles=%d", B, images * a.tiles);
        SH_LAUNCH_PS(ps, depth_scan_kernel, dim3((unsigned)B), dim3(NT), 0, st, tile_row, images * a.tiles, counts);
    }
    SH_CHECK_LAUNCH(who + 3);                                            // named without the "sh_", as ever
    return SH_OK;
}

// Everything behind the two overlap entry points.  RAYS: the projection of "Camera rays" under da.
template <bool RAYS>
int views_overlap(const char* who, const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext, int B, int V,
                  int H, int W, float z_near, float z_far, const DistArgs& da, const float* points, const float* normals, const uint8_t* view,
                  const int32_t* counts, int M, float tol, uint32_t* seen, uint8_t* keep, sh_stream_t stream) {
    if (RAYS) {
        SH_REQUIRE(da.dist && da.limit, SH_ERR_INVALID_ARG, "%s: null pointer", who);
        SH_REQUIRE(da.stride == 0 || da.stride == V, SH_ERR_INVALID_ARG, "%s: rays_stride = %d, must be 0 (one record per camera) or %d", who, da.stride, V);
    }
    if (const int rc = check_views(who, depth, dtype, intr, ext, B, V, H, W, 1)) return rc;
    SH_REQUIRE(points && normals && view && counts && seen && keep, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(M >= 0, SH_ERR_INVALID_ARG, "%s: negative size (M %d)", who, M);
    SH_REQUIRE(tol >= 0.f, SH_ERR_INVALID_ARG, "%s: tol must be >= 0 (and not NaN)", who);
    if (B == 0 || M == 0) return SH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const OverlapArgs a = {depth, intr, mask, ext, V, H, W, depth_scale, z_near, z_far, tol, points, normals, view, counts, M};
    ShProfScope ps(st, "%s_kernel|B=%d V=%d H=%d W=%d M=%d u16=%d", who + 3, B, V, H, W, M, dtype == SH_DEPTH_U16);
    const dim3 grid((unsigned)compact_chunks(M), (unsigned)B);
    if (dtype == SH_DEPTH_U16) SH_LAUNCH_PS(ps, (depth_views_overlap_kernel<uint16_t, RAYS>), grid, dim3(NT), 0, st, a, seen, keep, da);
    else SH_LAUNCH_PS(ps, (depth_views_overlap_kernel<float, RAYS>), grid, dim3(NT), 0, st, a, seen, keep, da);
    SH_CHECK_LAUNCH(who + 3);
    return SH_OK;
}

}  // namespace

extern "C" {

size_t sh_depth_workspace(int B, int H, int W) { return B <= 0 || H <= 0 || W <= 0 ? 0 : tile_rows_bytes(B, 1, H, W); }

int sh_depth_count(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W, float z_near,
                   float z_far, float max_step, int drop_isolated, int stride, int32_t* counts, void* workspace, size_t workspace_bytes,
                   sh_stream_t stream) {
    return depth_pass<false, false>("sh_depth_count", depth, dtype, depth_scale, intr, mask, nullptr, B, 0, H, W, z_near, z_far, max_step, drop_isolated,
                                    stride, counts, 0, 0, workspace, workspace_bytes, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int sh_depth_points(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W, float z_near,
                    float z_far, float max_step, int drop_isolated, int stride, const int32_t* counts, int max_count, int M,
                    const void* workspace, size_t workspace_bytes, float* points, float* normals, int32_t* pixel, sh_stream_t stream) {
    return depth_pass<true, false>("sh_depth_points", depth, dtype, depth_scale, intr, mask, nullptr, B, 0, H, W, z_near, z_far, max_step, drop_isolated,
                                   stride, const_cast<int32_t*>(counts), max_count, M, const_cast<void*>(workspace), workspace_bytes, points, normals,
                                   pixel, nullptr, nullptr, stream);
}

size_t sh_depth_views_workspace(int B, int V, int H, int W) {
    return B <= 0 || V < 1 || V > SH_DEPTH_MAX_VIEWS || H <= 0 || W <= 0 ? 0 : tile_rows_bytes(B, V, H, W);
}

int sh_depth_views_count(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext, int B, int V,
                         int H, int W, float z_near, float z_far, float max_step, int drop_isolated, int stride, int32_t* counts,
                         void* workspace, size_t workspace_bytes, sh_stream_t stream) {
    return depth_pass<false, true>("sh_depth_views_count", depth, dtype, depth_scale, intr, mask, ext, B, V, H, W, z_near, z_far, max_step, drop_isolated,
                                   stride, counts, 0, 0, workspace, workspace_bytes, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int sh_depth_views_points(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext, int B, int V,
                          int H, int W, float z_near, float z_far, float max_step, int drop_isolated, int stride, const int32_t* counts,
                          int max_count, int M, const void* workspace, size_t workspace_bytes, float* points, float* normals, int32_t* pixel,
                          uint8_t* view, int32_t* view_first, sh_stream_t stream) {
    return depth_pass<true, true>("sh_depth_views_points", depth, dtype, depth_scale, intr, mask, ext, B, V, H, W, z_near, z_far, max_step, drop_isolated,
                                  stride, const_cast<int32_t*>(counts), max_count, M, const_cast<void*>(workspace), workspace_bytes, points, normals,
                                  pixel, view, view_first, stream);
}

int sh_depth_views_overlap(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext, int B, int V,
                           int H, int W, float z_near, float z_far, const float* points, const float* normals, const uint8_t* view,
                           const int32_t* counts, int M, float tol, uint32_t* seen, uint8_t* keep, sh_stream_t stream) {
    return views_overlap<false>("sh_depth_views_overlap", depth, dtype, depth_scale, intr, mask, ext, B, V, H, W, z_near, z_far, DistArgs{nullptr, nullptr, 0},
                                points, normals, view, counts, M, tol, seen, keep, stream);
}

int sh_depth_views_rays_overlap(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext, int B, int V,
                                int H, int W, float z_near, float z_far, const float* dist, const float* limit, int rays_stride, const float* points,
                                const float* normals, const uint8_t* view, const int32_t* counts, int M, float tol, uint32_t* seen, uint8_t* keep,
                                sh_stream_t stream) {
    return views_overlap<true>("sh_depth_views_rays_overlap", depth, dtype, depth_scale, intr, mask, ext, B, V, H, W, z_near, z_far,
                               DistArgs{dist, limit, rays_stride}, points, normals, view, counts, M, tol, seen, keep, stream);
}

int sh_depth_rays_count(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W, float z_near,
                        float z_far, float max_step, int drop_isolated, int stride, const float* rays, int rays_stride, int32_t* counts,
                        void* workspace, size_t workspace_bytes, sh_stream_t stream) {
    return depth_pass<false, false, true>("sh_depth_rays_count", depth, dtype, depth_scale, intr, mask, nullptr, B, 0, H, W, z_near, z_far, max_step,
                                          drop_isolated, stride, counts, 0, 0, workspace, workspace_bytes, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          stream, rays, rays_stride);
}

int sh_depth_rays_points(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, int B, int H, int W, float z_near,
                         float z_far, float max_step, int drop_isolated, int stride, const float* rays, int rays_stride, const int32_t* counts,
                         int max_count, int M, const void* workspace, size_t workspace_bytes, float* points, float* normals, int32_t* pixel,
                         sh_stream_t stream) {
    return depth_pass<true, false, true>("sh_depth_rays_points", depth, dtype, depth_scale, intr, mask, nullptr, B, 0, H, W, z_near, z_far, max_step,
                                         drop_isolated, stride, const_cast<int32_t*>(counts), max_count, M, const_cast<void*>(workspace), workspace_bytes,
                                         points, normals, pixel, nullptr, nullptr, stream, rays, rays_stride);
}

int sh_depth_views_rays_count(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext, int B, int V,
                              int H, int W, float z_near, float z_far, float max_step, int drop_isolated, int stride, const float* rays,
                              int rays_stride, int32_t* counts, void* workspace, size_t workspace_bytes, sh_stream_t stream) {
    return depth_pass<false, true, true>("sh_depth_views_rays_count", depth, dtype, depth_scale, intr, mask, ext, B, V, H, W, z_near, z_far, max_step,
                                         drop_isolated, stride, counts, 0, 0, workspace, workspace_bytes, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         stream, rays, rays_stride);
}

int sh_depth_views_rays_points(const void* depth, int dtype, float depth_scale, const float* intr, const uint8_t* mask, const float* ext, int B, int V,
                               int H, int W, float z_near, float z_far, float max_step, int drop_isolated, int stride, const float* rays,
                               int rays_stride, const int32_t* counts, int max_count, int M, const void* workspace, size_t workspace_bytes,
                               float* points, float* normals, int32_t* pixel, uint8_t* view, int32_t* view_first, sh_stream_t stream) {
    return depth_pass<true, true, true>("sh_depth_views_rays_points", depth, dtype, depth_scale, intr, mask, ext, B, V, H, W, z_near, z_far, max_step,
                                        drop_isolated, stride, const_cast<int32_t*>(counts), max_count, M, const_cast<void*>(workspace), workspace_bytes,
                                        points, normals, pixel, view, view_first, stream, rays, rays_stride);
}


size_t sh_scan_compact_workspace(int B, int M) { return B <= 0 || M < 0 ? 0 : (size_t)B * compact_chunks(M) * sizeof(int32_t); }

int sh_scan_compact(const float* points, const float* normals, const int32_t* pixel, const uint8_t* view, const uint32_t* seen, const uint8_t* keep,
                    const int32_t* counts, int B, int V, int M, int max_kept, int M_out, void* workspace, size_t workspace_bytes,
                    float* points_out, float* normals_out, int32_t* pixel_out, uint8_t* view_out, uint32_t* seen_out, int32_t* counts_out,
                    int32_t* view_first_out, sh_stream_t stream) {
    const char* who = "sh_scan_compact";
    SH_REQUIRE(points && normals && pixel && view && keep && counts && points_out && normals_out && pixel_out && view_out && counts_out && view_first_out
               && !seen == !seen_out, SH_ERR_INVALID_ARG, "%s: null pointer (seen and seen_out: both or neither)", who);
    SH_REQUIRE(V >= 1 && V <= SH_DEPTH_MAX_VIEWS, SH_ERR_INVALID_ARG, "%s: V = %d views, must lie in [1, %d]", who, V, SH_DEPTH_MAX_VIEWS);
    SH_REQUIRE(B >= 0 && M >= 0 && M_out >= 0 && max_kept >= 0, SH_ERR_INVALID_ARG, "%s: negative size (B %d, M %d, M_out %d, max_kept %d)", who, B, M,
               M_out, max_kept);
    SH_REQUIRE(M_out >= max_kept, SH_ERR_INVALID_ARG, "%s: M_out = %d rows cannot hold the largest body's %d", who, M_out, max_kept);
    SH_REQUIRE(points_out != points && normals_out != normals && pixel_out != pixel && view_out != view && (!seen || seen_out != seen),
               SH_ERR_INVALID_ARG, "%s: out of place only - an output is its input", who);
    SH_REQUIRE(B <= 65535, SH_ERR_UNSUPPORTED, "%s: B too large", who);
    if (B == 0) return SH_OK;
    const int chunks = compact_chunks(M);
    const size_t need = sh_scan_compact_workspace(B, M);
    SH_REQUIRE(workspace && workspace_bytes >= need, SH_ERR_WORKSPACE, "%s: the workspace holds the chunk rows (%zu bytes needed)", who, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CompactArgs a = {points, normals, pixel, view, seen, keep, counts, V, M, chunks, M_out};
    const CompactOut out = {points_out, normals_out, pixel_out, view_out, seen_out, view_first_out};
    int32_t* chunk_row = static_cast<int32_t*>(workspace);
    const dim3 grid((unsigned)chunks, (unsigned)B);
    {
        ShProfScope ps(st, "scan_compact_count_kernel|B=%d M=%d", B, M);
        SH_LAUNCH_PS(ps, scan_compact_kernel<false>, grid, dim3(NT), 0, st, a, out, chunk_row, static_cast<const int32_t*>(nullptr));
    }
    {
        ShProfScope ps(st, "depth_scan_kernel|B=%d tiles=%d", B, chunks);
        SH_LAUNCH_PS(ps, depth_scan_kernel, dim3((unsigned)B), dim3(NT), 0, st, chunk_row, chunks, counts_out);
    }
    {
        ShProfScope ps(st, "scan_compact_emit_kernel|B=%d M=%d M_out=%d", B, M, M_out);
        SH_LAUNCH_PS(ps, scan_compact_kernel<true>, grid, dim3(NT), 0, st, a, out, chunk_row, counts_out);
    }
    SH_CHECK_LAUNCH("scan_compact");
    return SH_OK;
}

}  // extern "C"
