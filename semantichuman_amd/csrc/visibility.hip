// Which model vertices a sensor sees (include/sh_kernels.h, "Vertex visibility"): per vertex the segment to the body's viewpoint
// against every triangle of the table.  The reference has no counterpart.  The sweep has the form of scan.hip's
// nearest_search_kernel - one vertex per thread in registers, the faces streamed through double-buffered LDS tiles, every lane
// reading the same LDS address (broadcast) - but it is an any-hit search: a lane that has been hit is done, and a wave whose
// lanes are all done stops testing.  No atomics, no scratch: the face range may be split into chunks whose flags a second
// launch ORs, and an OR does not depend on order.  One camera and a rig share the face gathering, the fold kernel and the host
// routine; the two sweeps stay apart: every shared form tried cost one camera 7 - 10 % (DESIGN 4v,
// profiles/rig_of_one_shared_sweep.json).
#include "sh_nn.h"

namespace {

constexpr int NT = 256;          // threads per workgroup = vertices per workgroup
constexpr int TF = 256;          // faces per LDS tile: one face gathered per thread and tile

// The header's products, each in its one fixed form.
__device__ __forceinline__ float vis_dot(float ux, float uy, float uz, float vx, float vy, float vz) {
#pragma clang fp contract(off)
    return __builtin_fmaf(uz, vz, __builtin_fmaf(uy, vy, ux * vx));
}
__device__ __forceinline__ void vis_cross(float ux, float uy, float uz, float vx, float vy, float vz, float& cx, float& cy, float& cz) {
#pragma clang fp contract(off)
    cx = __builtin_fmaf(uy, vz, -(uz * vy));
    cy = __builtin_fmaf(uz, vx, -(ux * vz));
    cz = __builtin_fmaf(ux, vy, -(uy * vx));
}

// Face f as its three 16-byte LDS records - (a, e1.x) (e1.y, e1.z, e2.x, e2.y) (e2.z, i0, i1, i2); a face beyond the table, or with a
// corner outside [0, n), as NaN with indices -1: its det is NaN and no compare of the hit test holds.
__device__ __forceinline__ void gather_face(const float* __restrict__ xb, const int32_t* __restrict__ faces, int f, int nF, int n, f32x4& r0,
                                            f32x4& r1, f32x4& r2) {
#pragma clang fp contract(off)
    int i0 = -1, i1 = -1, i2 = -1;
    const bool ok = f < nF && face_corners(faces, f, n, i0, i1, i2);
    float ax = NAN, ay = NAN, az = NAN, bx = NAN, by = NAN, bz = NAN, cx = NAN, cy = NAN, cz = NAN;
    if (ok) {
        ax = xb[3L * i0]; ay = xb[3L * i0 + 1]; az = xb[3L * i0 + 2];
        bx = xb[3L * i1]; by = xb[3L * i1 + 1]; bz = xb[3L * i1 + 2];
        cx = xb[3L * i2]; cy = xb[3L * i2 + 1]; cz = xb[3L * i2 + 2];
    } else {
        i0 = i1 = i2 = -1;
    }
    r0 = f32x4{ax, ay, az, bx - ax};
    r1 = f32x4{by - ay, bz - az, cx - ax, cy - ay};
    r2 = f32x4{cz - az, __int_as_float(i0), __int_as_float(i1), __int_as_float(i2)};
}

// grid (vertex tile, face chunk, body).  final != 0: the one chunk's answer is the answer, flag = vis [B][n], 1 = visible;
// otherwise flag = the workspace [chunks][B][n], 1 = NOT visible on this chunk's evidence, for visibility_fold_kernel<false>.
// A face enters LDS as the three records of gather_face, written by the thread that gathered its corners.  A lane is `done` when nothing a face could do would change its answer: beyond n, masked,
// turned away from the sensor, or already hit.  The inner loop asks the wave every four faces whether any lane is still open;
// the tile loop asks the workgroup once per tile, through two LDS words per wave written before the tile's one barrier.
__global__ __launch_bounds__(NT) void vertex_visibility_kernel(const float* __restrict__ x, long x_sb, int n, const int32_t* __restrict__ faces,
                                                              int nF, const float* __restrict__ tn, const float* __restrict__ view,
                                                              float cos_g, const unsigned char* __restrict__ mask, long mask_sb, int B,
                                                              int tiles_per_chunk, int final, unsigned char* __restrict__ flag) {
#pragma clang fp contract(off)
    __shared__ f32x4 sf[2][3 * TF];
    __shared__ int sopen[2][NT / 64];
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
    const int i = blockIdx.x * NT + tid;
    const bool inside = i < n;
    const float* xb = x + (long)b * x_sb;
    const float vx = view[3L * b], vy = view[3L * b + 1], vz = view[3L * b + 2];
    const bool known = vx == vx && vy == vy && vz == vz;                 // uniform: a NaN row = no viewpoint, nothing is hidden
    const bool active = inside && (!mask || mask[(long)b * mask_sb + i] != 0);
    const float ox = inside ? xb[3L * i] : 0.f, oy = inside ? xb[3L * i + 1] : 0.f, oz = inside ? xb[3L * i + 2] : 0.f;
    const float dx = vx - ox, dy = vy - oy, dz = vz - oz;
    bool hidden = !active;
    if (known && active && tn) {                                         // the facing test; tn is uniform
        const float* t = tn + ((long)b * n + i) * 3;
        const float along = vis_dot(t[0], t[1], t[2], dx, dy, dz);
        const float len = sqrtf(vis_dot(dx, dy, dz, dx, dy, dz));
        hidden = !(along >= cos_g * len);                                // a NaN compares false: hidden
    }
    const int tiles = (nF + TF - 1) / TF;
    const int tile_lo = c * tiles_per_chunk;
    const int tile_hi = min(tile_lo + tiles_per_chunk, tiles);
    if (known && tile_lo < tile_hi) {                                    // uniform
        bool done = hidden;
        const int wave = sh_wave_id();
        f32x4 r0, r1, r2;
        auto fetch = [&](int tile) { gather_face(xb, faces, tile * TF + tid, nF, n, r0, r1, r2); };
        auto stage = [&](int buf) { sf[buf][3 * tid] = r0; sf[buf][3 * tid + 1] = r1; sf[buf][3 * tid + 2] = r2; };
        fetch(tile_lo);
        stage(0);
        int open = __ballot(!done) != 0ull;                               // uniform over the wave
        if ((tid & 63) == 0) sopen[0][wave] = open;
        __syncthreads();
        for (int tile = tile_lo; tile < tile_hi; ++tile) {
            const int cur = (tile - tile_lo) & 1;
            if ((sopen[cur][0] | sopen[cur][1] | sopen[cur][2] | sopen[cur][3]) == 0) break;   // uniform over the workgroup: every lane is done
            const bool more = tile + 1 < tile_hi;
            if (more) fetch(tile + 1);                                   // in flight under this tile's arithmetic
            for (int u = 0; u < TF; u += 4) {
                if (__ballot(!done) == 0ull) break;                      // uniform over the wave
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const f32x4 R0 = sf[cur][3 * (u + e)], R1 = sf[cur][3 * (u + e) + 1], R2 = sf[cur][3 * (u + e) + 2];
                    const float ax = R0[0], ay = R0[1], az = R0[2], e1x = R0[3], e1y = R1[0], e1z = R1[1];
                    const float e2x = R1[2], e2y = R1[3], e2z = R2[0];
                    const bool names = __float_as_int(R2[1]) == i || __float_as_int(R2[2]) == i || __float_as_int(R2[3]) == i;
                    float px, py, pz, qx, qy, qz;
                    vis_cross(dx, dy, dz, e2x, e2y, e2z, px, py, pz);
                    const float det = vis_dot(e1x, e1y, e1z, px, py, pz);
                    const float sx = ox - ax, sy = oy - ay, sz = oz - az;
                    const float uu = vis_dot(sx, sy, sz, px, py, pz);
                    vis_cross(sx, sy, sz, e1x, e1y, e1z, qx, qy, qz);
                    const float ww = vis_dot(dx, dy, dz, qx, qy, qz);
                    const float tt = vis_dot(e2x, e2y, e2z, qx, qy, qz);
                    const bool neg = det < 0.f;
                    const float ad = fabsf(det), su = neg ? -uu : uu, sw = neg ? -ww : ww, st = neg ? -tt : tt;
                    const bool hit = det != 0.f && su >= 0.f && sw >= 0.f && su + sw <= ad && st > 0.f && st < ad;   // a NaN compares false
                    done = done || (hit && !names);
                }
            }
            if (more) {
                stage(cur ^ 1);
                open = __ballot(!done) != 0ull;
                if ((tid & 63) == 0) sopen[cur ^ 1][wave] = open;
            }
            __syncthreads();                                             // one barrier per tile, as in nearest_search_kernel
        }
        hidden = done;
    }
    if (!inside) return;
    if (final) flag[(long)b * n + i] = hidden ? 0 : 1;
    else flag[((long)c * B + b) * n + i] = hidden ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ any-view form
constexpr int VMAX = SH_VISIBILITY_MAX_VIEWS;
static_assert(VMAX == 32, "one bit of a 32-bit word per view");

// The views a vertex at o can be seen from before any face is looked at: bit v = the view's row holds no NaN (-> `live`, uniform)
// and the vertex is active and - with a normal row t - faces it, by the single-view kernel's own expressions.  view: the body's
// [V][3]; its addresses are uniform, so the rows arrive by scalar loads.
__device__ __forceinline__ uint32_t view_candidates(const float* __restrict__ view, int V, bool active, float ox, float oy, float oz,
                                                    const float* __restrict__ t, float cos_g, uint32_t& live) {
#pragma clang fp contract(off)
    uint32_t cand = 0;
    live = 0;
    for (int v = 0; v < V; ++v) {
        const float vx = view[3 * v], vy = view[3 * v + 1], vz = view[3 * v + 2];
        if (!(vx == vx && vy == vy && vz == vz)) continue;               // uniform: an absent camera
        live |= 1u << v;
        bool ok = active;
        if (ok && t) {
            const float dx = vx - ox, dy = vy - oy, dz = vz - oz;
            const float along = vis_dot(t[0], t[1], t[2], dx, dy, dz);
            const float len = sqrtf(vis_dot(dx, dy, dz, dx, dy, dz));
            ok = along >= cos_g * len;                                   // a NaN compares false: not facing
        }
        cand |= ok ? 1u << v : 0u;
    }
    return cand;
}

// grid (vertex tile, face chunk, body): vertex_visibility_kernel with `open`, the views from which the vertex is still unoccluded,
// in place of `done`.  A face's s = o - a, q = s x e1 and t = e2 . q do not depend on the view and are formed once; a lane then walks
// the set bits of `open` (none for a face that names it), reads that view's position from LDS - one 16-byte read, a broadcast
// where the lanes agree - and forms d, p, det, u, w.  The early exits are the single-view kernel's: a ballot of "any view open"
// every four faces, the workgroup's through two LDS words per wave.  final != 0: out = seen [B][n] (may be null) and vis is
// written; otherwise out = the workspace [chunks][B][n], the views this chunk's faces hide, for visibility_fold_kernel<true>.
__global__ __launch_bounds__(NT) void vertex_visibility_views_kernel(const float* __restrict__ x, long x_sb, int n, const int32_t* __restrict__ faces,
                                                                    int nF, const float* __restrict__ tn, const float* __restrict__ view, int V,
                                                                    float cos_g, const unsigned char* __restrict__ mask, long mask_sb, int B,
                                                                    int tiles_per_chunk, int final, uint32_t* __restrict__ out,
                                                                    unsigned char* __restrict__ vis) {
#pragma clang fp contract(off)
    __shared__ f32x4 sf[2][3 * TF];
    __shared__ f32x4 sview[VMAX];
    __shared__ int sopen[2][NT / 64];
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
    const int i = blockIdx.x * NT + tid;
    const bool inside = i < n;
    const float* xb = x + (long)b * x_sb;
    const float* vb = view + 3L * b * V;
    if (tid < V) sview[tid] = f32x4{vb[3 * tid], vb[3 * tid + 1], vb[3 * tid + 2], 0.f};
    const bool active = inside && (!mask || mask[(long)b * mask_sb + i] != 0);
    const float ox = inside ? xb[3L * i] : 0.f, oy = inside ? xb[3L * i + 1] : 0.f, oz = inside ? xb[3L * i + 2] : 0.f;
    uint32_t live;
    const uint32_t cand = view_candidates(vb, V, active, ox, oy, oz, tn ? tn + ((long)b * n + i) * 3 : nullptr, cos_g, live);   // tn is read where active
    uint32_t open = cand;
    const int tiles = (nF + TF - 1) / TF;
    const int tile_lo = c * tiles_per_chunk;
    const int tile_hi = min(tile_lo + tiles_per_chunk, tiles);
    if (live != 0u && tile_lo < tile_hi) {                               // uniform
        const int wave = sh_wave_id();
        f32x4 r0, r1, r2;
        auto fetch = [&](int tile) { gather_face(xb, faces, tile * TF + tid, nF, n, r0, r1, r2); };
        auto stage = [&](int buf) { sf[buf][3 * tid] = r0; sf[buf][3 * tid + 1] = r1; sf[buf][3 * tid + 2] = r2; };
        fetch(tile_lo);
        stage(0);
        int any = __ballot(open != 0u) != 0ull;                          // uniform over the wave
        if ((tid & 63) == 0) sopen[0][wave] = any;
        __syncthreads();                                                 // sview as well
        for (int tile = tile_lo; tile < tile_hi; ++tile) {
            const int cur = (tile - tile_lo) & 1;
            if ((sopen[cur][0] | sopen[cur][1] | sopen[cur][2] | sopen[cur][3]) == 0) break;   // uniform over the workgroup
            const bool more = tile + 1 < tile_hi;
            if (more) fetch(tile + 1);
            for (int u = 0; u < TF; u += 4) {
                if (__ballot(open != 0u) == 0ull) break;                 // uniform over the wave
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const f32x4 R0 = sf[cur][3 * (u + e)], R1 = sf[cur][3 * (u + e) + 1], R2 = sf[cur][3 * (u + e) + 2];
                    const float ax = R0[0], ay = R0[1], az = R0[2], e1x = R0[3], e1y = R1[0], e1z = R1[1];
                    const float e2x = R1[2], e2y = R1[3], e2z = R2[0];
                    const bool names = __float_as_int(R2[1]) == i || __float_as_int(R2[2]) == i || __float_as_int(R2[3]) == i;
                    float qx, qy, qz;
                    const float sx = ox - ax, sy = oy - ay, sz = oz - az;
                    vis_cross(sx, sy, sz, e1x, e1y, e1z, qx, qy, qz);
                    const float tt = vis_dot(e2x, e2y, e2z, qx, qy, qz);
                    for (uint32_t m = names ? 0u : open; m != 0u; m &= m - 1u) {
                        const int v = __builtin_ctz(m);
                        const f32x4 vw = sview[v];
                        const float dx = vw[0] - ox, dy = vw[1] - oy, dz = vw[2] - oz;
                        float px, py, pz;
                        vis_cross(dx, dy, dz, e2x, e2y, e2z, px, py, pz);
                        const float det = vis_dot(e1x, e1y, e1z, px, py, pz);
                        const float uu = vis_dot(sx, sy, sz, px, py, pz);
                        const float ww = vis_dot(dx, dy, dz, qx, qy, qz);
                        const bool neg = det < 0.f;
                        const float ad = fabsf(det), su = neg ? -uu : uu, sw = neg ? -ww : ww, st = neg ? -tt : tt;
                        const bool hit = det != 0.f && su >= 0.f && sw >= 0.f && su + sw <= ad && st > 0.f && st < ad;   // a NaN compares false
                        open &= hit ? ~(1u << v) : ~0u;
                    }
                }
            }
            if (more) {
                stage(cur ^ 1);
                any = __ballot(open != 0u) != 0ull;
                if ((tid & 63) == 0) sopen[cur ^ 1][wave] = any;
            }
            __syncthreads();
        }
    }
    if (!inside) return;
    const long o = (long)b * n + i;
    if (final) {
        if (out) out[o] = open;
        vis[o] = (live == 0u ? active : open != 0u) ? 1 : 0;             // no camera at all: a full scan
    } else {
        out[((long)c * B + b) * n + i] = cand & ~open;
    }
}

// The workspace element of a chunk: one camera - 1 = NOT visible on this chunk's evidence; a rig - the views this chunk's faces hide.
template <bool RIG> using Part = std::conditional_t<RIG, uint32_t, unsigned char>;

// grid (vertex tile, body).  The OR of the chunks' elements -> vis; for a rig seen (may be null) = the candidate views of the vertex
// (formed again: V dot products) minus what any chunk hides, and the arguments before `B` are read.
template <bool RIG>
__global__ __launch_bounds__(256) void visibility_fold_kernel(const float* __restrict__ x, long x_sb, int n, const float* __restrict__ tn,
                                                             const float* __restrict__ view, int V, float cos_g,
                                                             const unsigned char* __restrict__ mask, long mask_sb, int B,
                                                             const Part<RIG>* __restrict__ part, int chunks, uint32_t* __restrict__ seen,
                                                             unsigned char* __restrict__ vis) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long o = (long)b * n + i;
    Part<RIG> hits = 0;
    for (int c = 0; c < chunks; ++c) hits |= part[(long)c * B * n + o];
    if constexpr (RIG) {
        const float* xb = x + (long)b * x_sb;
        const bool active = !mask || mask[(long)b * mask_sb + i] != 0;
        uint32_t live;
        const uint32_t cand = view_candidates(view + 3L * b * V, V, active, xb[3L * i], xb[3L * i + 1], xb[3L * i + 2],
                                              tn ? tn + ((long)b * n + i) * 3 : nullptr, cos_g, live);
        const uint32_t s = cand & ~hits;
        if (seen) seen[o] = s;
        vis[o] = (live == 0u ? active : s != 0u) ? 1 : 0;
    } else {
        vis[o] = hits ? 0 : 1;
    }
}

// The face split taken for `chunks` (0 = the library's) -> the workspace it needs in bytes, 0 for one chunk: no fold.
size_t workspace_need(int B, int n, int nF, int chunks, size_t part_bytes, int* c, int* tpc) {
    *c = nn_resolve_chunks(B, n, nF, TF, NT, chunks, tpc);
    return *c <= 1 ? 0 : (size_t)*c * B * n * part_bytes;
}

// Every check and both launches of the two entry points; `who` names the one that was called in every error text.  One camera:
// RIG = false, V = 0 and seen = nullptr.
template <bool RIG>
int vertex_visibility(const char* who, const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, const float* tn, const float* view, int V,
                      float cos_g, const uint8_t* mask, int64_t mask_sb, int B, int chunks, void* workspace, size_t workspace_bytes, uint8_t* vis,
                      uint32_t* seen, sh_stream_t stream) {
    SH_REQUIRE(x && view && vis && (faces || nF == 0), SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(!RIG || (V >= 1 && V <= VMAX), SH_ERR_INVALID_ARG, "%s: V = %d views, must lie in [1, %d]", who, V, VMAX);
    SH_REQUIRE(B >= 0 && n >= 0 && nF >= 0 && chunks >= 0, SH_ERR_INVALID_ARG, "%s: negative size (B %d, n %d, nF %d, chunks %d)", who, B, n, nF,
               chunks);
    SH_REQUIRE(!tn || (cos_g >= 0.f && cos_g < 1.f), SH_ERR_INVALID_ARG, "%s: cos_g must lie in [0, 1) (and not be NaN)", who);
    if (B == 0 || n == 0) return SH_OK;
    SH_REQUIRE(x_sb >= 3L * n && (!mask || mask_sb == 0 || mask_sb >= n), SH_ERR_INVALID_ARG,
               "%s: batch stride shorter than a body (x_sb %ld, mask_sb %ld)", who, (long)x_sb, (long)mask_sb);
    SH_REQUIRE(B <= 65535 && (long)B * n < (1L << 30) && nF < (1 << 29), SH_ERR_UNSUPPORTED, "%s: B, B*n or nF too large", who);
    int c, tpc;
    const size_t need = workspace_need(B, n, nF, chunks, sizeof(Part<RIG>), &c, &tpc);
    SH_REQUIRE(c <= 65535, SH_ERR_UNSUPPORTED, "%s: %d face chunks", who, c);
    SH_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), SH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes needed for %d chunks)", who,
               need, c);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int final = c <= 1;
    Part<RIG>* part = static_cast<Part<RIG>*>(workspace);
    const dim3 grid((unsigned)sh_cdiv(n, NT), (unsigned)c, (unsigned)B);
    if constexpr (RIG) {
        ShProfScope ps(st, "vertex_visibility_views_kernel|B=%d n=%d nF=%d V=%d chunks=%d", B, n, nF, V, c);
        SH_LAUNCH_PS(ps, vertex_visibility_views_kernel, grid, dim3(NT), 0, st, x, (long)x_sb, n, faces, nF, tn, view, V, cos_g, mask, (long)mask_sb, B,
                     tpc, final, final ? seen : part, vis);
    } else {
        ShProfScope ps(st, "vertex_visibility_kernel|B=%d n=%d nF=%d chunks=%d", B, n, nF, c);
        SH_LAUNCH_PS(ps, vertex_visibility_kernel, grid, dim3(NT), 0, st, x, (long)x_sb, n, faces, nF, tn, view, cos_g, mask, (long)mask_sb, B, tpc,
                     final, final ? vis : part);
    }
    if (!final) {
        const dim3 fold_grid((unsigned)sh_cdiv(n, 256), (unsigned)B);
        if constexpr (RIG) {
            ShProfScope ps(st, "visibility_views_fold_kernel|B=%d n=%d V=%d chunks=%d", B, n, V, c);
            SH_LAUNCH_PS(ps, visibility_fold_kernel<true>, fold_grid, dim3(256), 0, st, x, (long)x_sb, n, tn, view, V, cos_g, mask, (long)mask_sb, B, part,
                         c, seen, vis);
        } else {
            ShProfScope ps(st, "visibility_fold_kernel|B=%d n=%d chunks=%d", B, n, c);
            SH_LAUNCH_PS(ps, visibility_fold_kernel<false>, fold_grid, dim3(256), 0, st, x, (long)x_sb, n, tn, view, V, cos_g, mask, (long)mask_sb, B, part,
                         c, seen, vis);
        }
    }
    SH_CHECK_LAUNCH(who + 3);                                            // named without the "sh_", as ever
    return SH_OK;
}

}  // namespace

extern "C" {

size_t sh_vertex_visibility_workspace(int B, int n, int nF, int chunks) {
    int c, tpc;
    return B <= 0 || n <= 0 || nF < 0 || chunks < 0 ? 0 : workspace_need(B, n, nF, chunks, sizeof(Part<false>), &c, &tpc);
}

int sh_vertex_visibility(const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, const float* tn, const float* view, float cos_g,
                         const uint8_t* mask, int64_t mask_sb, int B, int chunks, void* workspace, size_t workspace_bytes, uint8_t* vis,
                         sh_stream_t stream) {
    return vertex_visibility<false>("sh_vertex_visibility", x, x_sb, n, faces, nF, tn, view, 0, cos_g, mask, mask_sb, B, chunks, workspace,
                                    workspace_bytes, vis, nullptr, stream);
}

size_t sh_vertex_visibility_views_workspace(int B, int n, int nF, int V, int chunks) {
    int c, tpc;
    return B <= 0 || n <= 0 || nF < 0 || V < 1 || V > VMAX || chunks < 0 ? 0 : workspace_need(B, n, nF, chunks, sizeof(Part<true>), &c, &tpc);
}

int sh_vertex_visibility_views(const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, const float* tn, const float* view, int V,
                               float cos_g, const uint8_t* mask, int64_t mask_sb, int B, int chunks, void* workspace, size_t workspace_bytes,
                               uint8_t* vis, uint32_t* seen, sh_stream_t stream) {
    return vertex_visibility<true>("sh_vertex_visibility_views", x, x_sb, n, faces, nF, tn, view, V, cos_g, mask, mask_sb, B, chunks, workspace,
                                   workspace_bytes, vis, seen, stream);
}

}  // extern "C"
