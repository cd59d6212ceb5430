// Point-to-surface distance for scan fitting: the exact closest point of a triangle mesh to every scan point
// (include/sh_kernels.h, "Nearest surface points"; the gradient of the Chamfer term built on it is scan.hip's
// surface_bwd_kernel, beside the vertex form it follows).  The reference has no counterpart.  The
// sweep follows nearest_search_kernel of scan.hip: queries in registers, one record per triangle streamed through LDS, every
// lane reading the same LDS address (broadcast).  What is streamed is the triangle's bounding sphere; the region test of the
// header runs for a triangle only when the wave's ballot says that some lane cannot rule it out.  The cull only ever skips a
// triangle whose fp32 distance is provably larger than the query's best so far, so the result equals the unculled sweep's bit
// for bit; the unculled sweep is kept (cull = 0) as its yardstick.  No atomics of any kind in the kernels a fit runs (the
// only atomics are two counters of the diagnostic instantiation the benchmark asks for with `stats`): (d2, face) is kept under the lexicographic minimum.
#include "sh_nn.h"

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int QPT = 4;           // queries a thread keeps in registers
constexpr int QT = NT * QPT;     // queries per workgroup; a wave owns 256 CONSECUTIVE ones (a spatially sorted scan keeps them close)
constexpr int FT = 256;          // triangles per LDS tile: one global load per thread and tile
constexpr int TRI = 12;          // floats per triangle record: a, ab, ac, |ab|^2, ab.ac, |ac|^2
// Safety factor of the cull, applied to sqrt(best) and to the sphere's radius.  The rounding it has to cover is about 30 units
// of 2^-24 (include/sh_kernels.h derives it); 2^-10 is 500 times that and costs no measurable number of extra region tests.
constexpr float MARGIN = SH_SURFACE_MARGIN;

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

struct Foot { float v, w, d2; };

// The header's expression, in its one fixed form: no contraction beyond the fused multiply-adds written out, so that every
// kernel that inlines it (sweep, finish) and the numpy transcription of tests/surface_ref.py round alike.
__device__ __forceinline__ Foot surf_foot(const float* __restrict__ T, float sx, float sy, float sz) {
#pragma clang fp contract(off)
    const float ax = T[0], ay = T[1], az = T[2], abx = T[3], aby = T[4], abz = T[5], acx = T[6], acy = T[7], acz = T[8];
    const float e11 = T[9], e12 = T[10], e22 = T[11];
    const float apx = sx - ax, apy = sy - ay, apz = sz - az;
    const float d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    const float d3 = d1 - e11, d4 = d2 - e12, d5 = d1 - e12, d6 = d2 - e22;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    // interior first, then the regions in REVERSE order of the header's list, so that the first region that applies wins
    const float sum = (va + vb) + vc;
    const float den = sum > 0.f ? 1.0f / sum : 0.f;                       // degenerate triangle: falls to vertex a
    float v = vb * den, w = vc * den;
    const float den_bc = e43 + e56, den_ac = d2 - d6, den_ab = d1 - d3;
    if (va <= 0.f && e43 >= 0.f && e56 >= 0.f && den_bc > 0.f) { w = e43 / den_bc; v = 1.0f - w; }          // edge bc
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f && den_ac > 0.f) { v = 0.f; w = d2 / den_ac; }                  // edge ca
    if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; }                                                       // vertex c
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f && den_ab > 0.f) { v = d1 / den_ab; w = 0.f; }                  // edge ab
    if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; }                                                       // vertex b
    if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; }                                                      // vertex a
    v = fminf(fmaxf(v, 0.f), 1.f);                                        // a valid convex combination whatever the rounding did
    w = fminf(fmaxf(w, 0.f), 1.0f - v);
    const float rx = apx - __builtin_fmaf(w, acx, v * abx), ry = apy - __builtin_fmaf(w, acy, v * aby),
                rz = apz - __builtin_fmaf(w, acz, v * abz);
    Foot o;
    o.v = v; o.w = w;
    o.d2 = __builtin_fmaf(rz, rz, __builtin_fmaf(ry, ry, rx * rx));
    return o;
}

// One thread per (body, triangle): the triangle's record and bounding sphere for this step's vertices.  A triangle that is
// not a target (a masked corner, or an index outside [0, n)) gets the centre (+inf, +inf, +inf): the sweep never tests it.
// GATED: the centre is also written on its own, contiguous [B][nF][3], with a flag [B][nF] that is 1 for a target whose centre
// is finite - the targets and the mask of the gated search that bounds the sweep (header, "Nearest surface points under a
// normal gate").  Without GATED neither pointer is read.
template <bool GATED>
__global__ __launch_bounds__(256) void surface_prep_kernel(const float* __restrict__ x, long x_sb, int n, const int32_t* __restrict__ faces,
                                                          int nF, const unsigned char* __restrict__ v_mask, long mask_sb, int B,
                                                          float* __restrict__ tri, f32x4* __restrict__ sphere, float* __restrict__ cen,
                                                          unsigned char* __restrict__ fvalid) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * nF) return;
    const int b = (int)(t / nF), f = (int)(t - (long)b * nF);
    const int i0 = faces[3L * f], i1 = faces[3L * f + 1], i2 = faces[3L * f + 2];
    bool ok = (unsigned)i0 < (unsigned)n && (unsigned)i1 < (unsigned)n && (unsigned)i2 < (unsigned)n;
    if (ok && v_mask) {
        const unsigned char* mb = v_mask + (long)b * mask_sb;
        ok = mb[i0] != 0 && mb[i1] != 0 && mb[i2] != 0;
    }
    float* T = tri + t * TRI;
    if (!ok) {
#pragma unroll
        for (int k = 0; k < TRI; ++k) T[k] = 0.f;
        sphere[t] = f32x4{INFINITY, INFINITY, INFINITY, 0.f};
        if constexpr (GATED) { cen[3 * t] = 0.f; cen[3 * t + 1] = 0.f; cen[3 * t + 2] = 0.f; fvalid[t] = 0; }
        return;
    }
    const float* xb = x + (long)b * x_sb;
    const float ax = xb[3L * i0], ay = xb[3L * i0 + 1], az = xb[3L * i0 + 2];
    const float bx = xb[3L * i1], by = xb[3L * i1 + 1], bz = xb[3L * i1 + 2];
    const float cx = xb[3L * i2], cy = xb[3L * i2 + 1], cz = xb[3L * i2 + 2];
    const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    T[0] = ax; T[1] = ay; T[2] = az; T[3] = abx; T[4] = aby; T[5] = abz; T[6] = acx; T[7] = acy; T[8] = acz;
    T[9] = dot3(abx, aby, abz, abx, aby, abz); T[10] = dot3(abx, aby, abz, acx, acy, acz); T[11] = dot3(acx, acy, acz, acx, acy, acz);
    const float third = 1.0f / 3.0f;
    float mx = ax + (abx + acx) * third, my = ay + (aby + acy) * third, mz = az + (abz + acz) * third;
    const float ra = dot3(ax - mx, ay - my, az - mz, ax - mx, ay - my, az - mz);
    const float rb = dot3(bx - mx, by - my, bz - mz, bx - mx, by - my, bz - mz);
    const float rc = dot3(cx - mx, cy - my, cz - mz, cx - mx, cy - my, cz - mz);
    float r = sqrtf(fmaxf(ra, fmaxf(rb, rc))) * MARGIN;
    if constexpr (GATED) {
        const bool fin = mx < INFINITY && mx > -INFINITY && my < INFINITY && my > -INFINITY && mz < INFINITY && mz > -INFINITY;
        cen[3 * t] = fin ? mx : 0.f; cen[3 * t + 1] = fin ? my : 0.f; cen[3 * t + 2] = fin ? mz : 0.f; fvalid[t] = fin ? 1 : 0;
    }
    if (!(mx < INFINITY && mx > -INFINITY && my < INFINITY && my > -INFINITY && mz < INFINITY && mz > -INFINITY && r < INFINITY)) {
        mx = my = mz = 0.f; r = INFINITY;                                 // overflow or NaN in the vertices: never culled
    }
    sphere[t] = f32x4{mx, my, mz, r};
}

struct SurfParams {
    const float* q; long q_sb; int nq; const int32_t* q_count;
    const float* tri; const f32x4* sphere; int nF;
    const float* bound;
    int tiles_per_chunk, chunks, cull;
    unsigned long long* stats;
};

// The face-normal gate of the header ("Nearest surface points under a normal gate"): the queries' normals, the faces' normals
// (contiguous [B][nF][3]) and the smallest cosine that pairs them.
struct SurfGate {
    const float* qn; long qn_sb;
    const float* fn;
    float cos_min;
};

__device__ __forceinline__ bool surf_compatible(float qu, float qv, float qw, const float* __restrict__ N, float cos_min) {
    return __builtin_fmaf(qw, N[2], __builtin_fmaf(qv, N[1], qu * N[0])) >= cos_min;   // a NaN compares false: not compatible
}

// grid (query tile, triangle chunk, body).  The chunk's (d2, face) go to part_d2 / part_idx [B][chunks][nq] for
// surface_finish_kernel.  Triangles are visited in ascending order and a candidate replaces the best only when strictly
// closer: the lowest face wins an exact tie.  A triangle is skipped for a query when
//     d2(s, centre) > (rb + r)^2,      rb = MARGIN * sqrt(the query's bound),  r = MARGIN * the sphere's radius
// where the bound is the smaller of the caller's upper bound and the best distance found so far (cull = 0: rb = +inf, nothing is
// skipped).  The region test runs, for the lanes that need it, when any lane of the wave does.
// GATED: inside that branch, a lane that needs the triangle runs the region test only when the triangle's normal (one record
// per triangle, the address uniform over the wave like the triangle's own) is compatible with its query's - three more query
// registers, one dot product and one compare per lane and tested triangle; the sphere loop is untouched.  An incompatible pair
// therefore neither becomes `best` nor shrinks rb, and what the sphere test skips is still farther than the bound in force.
// Without GATED, g is not read and the gate's registers do not exist.
template <bool STATS, bool GATED>
__global__ __launch_bounds__(NT) void surface_search_kernel(const SurfParams p, int32_t* __restrict__ part_idx, float* __restrict__ part_d2,
                                                           const SurfGate g) {
    __shared__ __attribute__((aligned(16))) float sx[2][FT];
    __shared__ __attribute__((aligned(16))) float sy[2][FT];
    __shared__ __attribute__((aligned(16))) float sz[2][FT];
    __shared__ __attribute__((aligned(16))) float sr[2][FT];
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int nqb = clamp_count(p.q_count, b, p.nq);
    const int j0 = blockIdx.x * QT;
    if (j0 >= nqb) return;                                               // uniform: no query of this tile is live (finish writes them)
    const float* qb = p.q + (long)b * p.q_sb;
    const f32x4* sph = p.sphere + (long)b * p.nF;
    const float* trib = p.tri + (long)b * p.nF * TRI;
    const float* qnb = GATED ? g.qn + (long)b * g.qn_sb : nullptr;
    const float* fnb = GATED ? g.fn + (long)b * p.nF * 3 : nullptr;
    const float cos_min = g.cos_min;
    float qx[QPT], qy[QPT], qz[QPT], qu[QPT], qv[QPT], qw[QPT], best[QPT], rb[QPT];
    int bi[QPT];
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int j = j0 + wv * (64 * QPT) + k * 64 + lane;
        const bool live = j < nqb;
        // a dead query sits at +inf with a bound of 0: infinitely far from every sphere, it never asks for a region test
        qx[k] = live ? qb[3L * j] : INFINITY; qy[k] = live ? qb[3L * j + 1] : INFINITY; qz[k] = live ? qb[3L * j + 2] : INFINITY;
        if constexpr (GATED) { qu[k] = live ? qnb[3L * j] : 0.f; qv[k] = live ? qnb[3L * j + 1] : 0.f; qw[k] = live ? qnb[3L * j + 2] : 0.f; }
        best[k] = INFINITY; bi[k] = -1;
        const float bnd = (p.cull && p.bound && live) ? p.bound[(long)b * p.nq + j] : INFINITY;
        rb[k] = live ? sqrtf(fmaxf(bnd, 0.f)) * MARGIN : 0.f;
        if (!(rb[k] == rb[k])) rb[k] = INFINITY;                         // NaN bound: no bound
    }
    const int tiles = (p.nF + FT - 1) / FT;
    const int tile_lo = c * p.tiles_per_chunk;
    const int tile_hi = min(tile_lo + p.tiles_per_chunk, tiles);
    unsigned long long tested = 0;                                       // STATS only: the shipped instantiation has no counter
    if (tile_lo < tile_hi) {                                             // uniform
        f32x4 ld;
        auto fetch = [&](int tile) {
            const int f = tile * FT + tid;
            ld = f < p.nF ? sph[f] : f32x4{INFINITY, INFINITY, INFINITY, 0.f};
        };
        fetch(tile_lo);
        sx[0][tid] = ld[0]; sy[0][tid] = ld[1]; sz[0][tid] = ld[2]; sr[0][tid] = ld[3];
        __syncthreads();
        for (int tile = tile_lo; tile < tile_hi; ++tile) {
            const int cur = (tile - tile_lo) & 1;
            const bool more = tile + 1 < tile_hi;
            if (more) fetch(tile + 1);                                   // in flight under this tile's arithmetic
            const int base = tile * FT;
            for (int u = 0; u < FT; u += 4) {
                const f32x4 X = *reinterpret_cast<const f32x4*>(&sx[cur][u]);
                const f32x4 Y = *reinterpret_cast<const f32x4*>(&sy[cur][u]);
                const f32x4 Z = *reinterpret_cast<const f32x4*>(&sz[cur][u]);
                const f32x4 R = *reinterpret_cast<const f32x4*>(&sr[cur][u]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    bool need[QPT];
                    bool any = false;
#pragma unroll
                    for (int k = 0; k < QPT; ++k) {
                        const float d = nn_d2(qx[k], qy[k], qz[k], X[e], Y[e], Z[e]);
                        const float t = rb[k] + R[e];
                        need[k] = !(d > t * t);                          // written so that a NaN asks for the test
                        any = any || need[k];
                    }
                    if (X[e] < INFINITY && __ballot(any) != 0ull) {      // uniform: the triangle is a target and some lane needs it
                        const int f = base + u + e;
                        const float* T = trib + (long)f * TRI;
                        const float* N = GATED ? fnb + 3L * f : nullptr;
#pragma unroll
                        for (int k = 0; k < QPT; ++k) {
                            if constexpr (GATED) need[k] = need[k] && surf_compatible(qu[k], qv[k], qw[k], N, cos_min);
                            if (need[k]) {
                                const Foot ft = surf_foot(T, qx[k], qy[k], qz[k]);
                                if (ft.d2 < best[k]) {
                                    best[k] = ft.d2; bi[k] = f;
                                    if (p.cull) rb[k] = fminf(rb[k], sqrtf(ft.d2) * MARGIN);
                                }
                                if (STATS) ++tested;
                            }
                        }
                    }
                }
            }
            if (more) { sx[cur ^ 1][tid] = ld[0]; sy[cur ^ 1][tid] = ld[1]; sz[cur ^ 1][tid] = ld[2]; sr[cur ^ 1][tid] = ld[3]; }
            __syncthreads();                                             // one barrier per tile: the other buffer was last read before the previous one
        }
    }
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int j = j0 + wv * (64 * QPT) + k * 64 + lane;
        if (j < nqb) {
            const long o = ((long)b * p.chunks + c) * p.nq + j;
            part_idx[o] = bi[k]; part_d2[o] = best[k];
        }
    }
    if (STATS) {                                                         // diagnostic instantiation only (tools/bench_surface.py)
        for (int o = 32; o > 0; o >>= 1) tested += __shfl_xor(tested, o, 64);
        if (lane == 0) atomicAdd(p.stats, tested);
    }
}

// One thread per (body, query).  (d2, face) = lexicographic minimum over the chunks: chunk c holds lower faces than chunk
// c + 1, so walking the chunks in order with a strict `<` is that minimum.  With the cull on, the result is the unculled
// sweep's whenever it does not exceed MARGIN times the caller's bound (every skipped triangle is farther than that, or than a
// distance found; the factor lets a foot point ON the nearest vertex pass, whose distance differs from the vertex search's by
// rounding).  When it does - the bound was no upper bound of the fp32 surface distance, which a vertex mask can cause - the
// query is swept again here without a bound.  Then the weights of the chosen face are formed once more.
// GATED: the sweep here tests the compatible targets only (the same expression), and a query without a face is NOT swept again
// when its bound was +inf: nothing was culled by the bound then, so "no compatible target" is the sweep's exact answer (a scan
// whose normals all point inward would otherwise walk every triangle here, one thread per point).  With a finite bound and no
// face the comparison below fails (+inf is not <= it) and the query is swept again, as without the gate.
template <bool GATED>
__global__ __launch_bounds__(256) void surface_finish_kernel(const SurfParams p, int B, const int32_t* __restrict__ part_idx,
                                                            const float* __restrict__ part_d2, int32_t* __restrict__ face,
                                                            float* __restrict__ d2, float* __restrict__ uv, const SurfGate g) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * p.nq) return;
    const int b = (int)(t / p.nq), j = (int)(t - (long)b * p.nq);
    if (j >= clamp_count(p.q_count, b, p.nq)) { face[t] = -1; d2[t] = 0.f; uv[2 * t] = 0.f; uv[2 * t + 1] = 0.f; return; }
    float best = INFINITY;
    int bi = -1;
    for (int c = 0; c < p.chunks; ++c) {
        const long o = ((long)b * p.chunks + c) * p.nq + j;
        const float d = part_d2[o];
        if (d < best) { best = d; bi = part_idx[o]; }
    }
    const float* qb = p.q + (long)b * p.q_sb;
    const float sx = qb[3L * j], sy = qb[3L * j + 1], sz = qb[3L * j + 2];
    const float* trib = p.tri + (long)b * p.nF * TRI;
    if (p.cull) {
        const float bnd = p.bound ? p.bound[t] : INFINITY;
        if ((!GATED && bi < 0) || !(best <= bnd * MARGIN)) {              // a skipped triangle is farther than MARGIN^2 * bnd
            const f32x4* sph = p.sphere + (long)b * p.nF;
            best = INFINITY; bi = -1;
            if (p.stats) atomicAdd(p.stats + 1, 1ull);                   // diagnostic: points that took this path
            float qu = 0.f, qv = 0.f, qw = 0.f;
            if constexpr (GATED) {
                const float* qnb = g.qn + (long)b * g.qn_sb;
                qu = qnb[3L * j]; qv = qnb[3L * j + 1]; qw = qnb[3L * j + 2];
            }
            for (int f = 0; f < p.nF; ++f) {
                if (!(sph[f][0] < INFINITY)) continue;
                if constexpr (GATED)
                    if (!surf_compatible(qu, qv, qw, g.fn + ((long)b * p.nF + f) * 3, g.cos_min)) continue;
                const Foot ft = surf_foot(trib + (long)f * TRI, sx, sy, sz);
                if (ft.d2 < best) { best = ft.d2; bi = f; }
            }
        }
    }
    float v = 0.f, w = 0.f;
    if (bi >= 0) {
        const Foot ft = surf_foot(trib + (long)bi * TRI, sx, sy, sz);
        v = ft.v; w = ft.w;
    }
    face[t] = bi; d2[t] = best; uv[2 * t] = v; uv[2 * t + 1] = w;
}

// One thread per (body, face): the unit normal of the header ("Face normals"), in its one fixed form - the cross product as
// vertex_normals_kernel forms a face's contribution, no contraction beyond the fused multiply-adds written out, so the numpy
// transcription of tests/surface_gated_ref.py rounds alike.  A face with a corner outside [0, n), no area or an overflow gets
// the zero vector.  No LDS, no atomics; every element stored.
__global__ __launch_bounds__(256) void face_normals_kernel(const float* __restrict__ x, long x_sb, int n, const int32_t* __restrict__ faces,
                                                          int nF, int B, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * nF) return;
    const int b = (int)(t / nF), f = (int)(t - (long)b * nF);
    int i0, i1, i2;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (face_corners(faces, f, n, i0, i1, i2)) {
        const float* xb = x + (long)b * x_sb;
        float cx, cy, cz;
        face_cross(xb + 3L * i0, xb + 3L * i1, xb + 3L * i2, cx, cy, cz);
        const float len2 = __builtin_fmaf(cz, cz, __builtin_fmaf(cy, cy, cx * cx));
        if (len2 > 0.f && len2 < INFINITY) {
            const float len = sqrtf(len2);
            nx = cx / len; ny = cy / len; nz = cz / len;
        }
    }
    float* o = out + t * 3;
    o[0] = nx; o[1] = ny; o[2] = nz;
}

size_t sf_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// Where the pieces of the workspace lie.  Ungated: spheres, records, the chunks' partial results - the layout it has always had.
// Gated: after the records come the centres [B][nF][3], their flags [B][nF], the bound [B][nq] and the index [B][nq] the bounding
// search writes, and that search's own workspace; the partial results stay last.
struct SurfLayout {
    size_t sphere, tri, cen, fvalid, bound, bidx, nn, nn_bytes, part, total;
};

SurfLayout surf_layout(int B, int nq, int nF, int chunks, bool gated) {
    SurfLayout L{};
    size_t o = 0;
    L.sphere = o; o += sf_align16((size_t)B * nF * sizeof(f32x4));
    L.tri = o; o += sf_align16((size_t)B * nF * TRI * sizeof(float));
    if (gated) {
        L.cen = o; o += sf_align16((size_t)B * nF * 3 * sizeof(float));
        L.fvalid = o; o += sf_align16((size_t)B * nF);
        L.bound = o; o += sf_align16((size_t)B * nq * sizeof(float));
        L.bidx = o; o += sf_align16((size_t)B * nq * sizeof(int32_t));
        L.nn_bytes = sh_nearest_points_workspace(B, nq, nF, 0);
        L.nn = o; o += sf_align16(L.nn_bytes);
    }
    L.part = o; o += (size_t)B * chunks * nq * (sizeof(float) + sizeof(int32_t));
    L.total = o;
    return L;
}

// sh_nearest_surface (g == nullptr) and sh_nearest_surface_gated: the checks both make, the split, the workspace and the
// launches.  `who` is the entry point's name in every error text.
int surf_search(const char* who, const float* q, int64_t q_sb, int nq, const int32_t* q_count, const float* x, int64_t x_sb, int n,
                const int32_t* faces, int nF, const uint8_t* v_mask, int64_t mask_sb, const float* bound, const SurfGate* g, int B, int chunks,
                int cull, int32_t* face, float* d2, float* uv, uint64_t* stats, void* workspace, size_t workspace_bytes, sh_stream_t stream) {
    SH_REQUIRE(q && x && face && d2 && uv && (faces || nF == 0) && (!g || (g->qn && (g->fn || nF == 0))), SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(B >= 0 && nq >= 0 && n >= 0 && nF >= 0 && chunks >= 0, SH_ERR_INVALID_ARG, "%s: negative size (B %d, nq %d, n %d, nF %d, chunks %d)", who,
               B, nq, n, nF, chunks);
    SH_REQUIRE(!g || g->cos_min == g->cos_min, SH_ERR_INVALID_ARG, "%s: cos_min is NaN", who);
    if (B == 0 || nq == 0) return SH_OK;
    SH_REQUIRE(q_sb >= 3L * nq && x_sb >= 3L * n && (!v_mask || mask_sb == 0 || mask_sb >= n), SH_ERR_INVALID_ARG,
               "%s: batch stride shorter than a body (q_sb %ld, x_sb %ld, mask_sb %ld)", who, (long)q_sb, (long)x_sb, (long)mask_sb);
    SH_REQUIRE(!g || g->qn_sb >= 3L * nq, SH_ERR_INVALID_ARG, "%s: batch stride shorter than a body (qn_sb %ld)", who, g ? g->qn_sb : 0L);
    SH_REQUIRE(B <= 65535 && (long)B * nq < (1L << 30) && (long)B * nF < (1L << 27), SH_ERR_UNSUPPORTED, "%s: B, B*nq or B*nF too large", who);
    SurfParams p{};
    p.chunks = nn_resolve_chunks(B, nq, nF, FT, QT, chunks, &p.tiles_per_chunk);
    SH_REQUIRE(p.chunks <= 65535, SH_ERR_UNSUPPORTED, "%s: %d triangle chunks", who, p.chunks);
    const SurfLayout L = surf_layout(B, nq, nF, p.chunks, g != nullptr);
    SH_REQUIRE(workspace && workspace_bytes >= L.total && ((uintptr_t)workspace & 15) == 0, SH_ERR_WORKSPACE,
               "%s: workspace too small or not 16-byte aligned (%zu bytes needed for %d chunks)", who, L.total, p.chunks);
    char* wsb = static_cast<char*>(workspace);
    f32x4* sphere = reinterpret_cast<f32x4*>(wsb + L.sphere);
    float* tri = reinterpret_cast<float*>(wsb + L.tri);
    float* part_d2 = reinterpret_cast<float*>(wsb + L.part);
    int32_t* part_idx = reinterpret_cast<int32_t*>(part_d2 + (size_t)B * p.chunks * nq);
    p.q = q; p.q_sb = (long)q_sb; p.nq = nq; p.q_count = q_count;
    p.tri = tri; p.sphere = sphere; p.nF = nF; p.bound = bound; p.cull = cull ? 1 : 0;
    p.stats = reinterpret_cast<unsigned long long*>(stats);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 prep_grid((unsigned)(((long)B * nF + 255) / 256));
    if (nF > 0 && !g) {
        ShProfScope ps(st, "surface_prep_kernel|B=%d nF=%d", B, nF);
        SH_LAUNCH_PS(ps, surface_prep_kernel<false>, prep_grid, dim3(256), 0, st, x, (long)x_sb, n, faces, nF, v_mask, (long)mask_sb, B, tri, sphere,
                     (float*)nullptr, (unsigned char*)nullptr);
    }
    if (g) {
        float* cen = reinterpret_cast<float*>(wsb + L.cen);
        unsigned char* fvalid = reinterpret_cast<unsigned char*>(wsb + L.fvalid);
        if (nF > 0) {
            ShProfScope ps(st, "surface_prep_gated_kernel|B=%d nF=%d", B, nF);
            SH_LAUNCH_PS(ps, surface_prep_kernel<true>, prep_grid, dim3(256), 0, st, x, (long)x_sb, n, faces, nF, v_mask, (long)mask_sb, B, tri, sphere,
                         cen, fvalid);
        }
        if (p.cull && !bound && nF > 0) {
            // The bound that holds under the gate: the gated nearest search over the targets' centres, the faces' normals as the
            // targets' normals.  A centre lies on its face, so its distance bounds that face's; no compatible target: +inf.
            float* bnd = reinterpret_cast<float*>(wsb + L.bound);
            const int rc = sh_nearest_points_gated(q, q_sb, nq, q_count, g->qn, g->qn_sb, cen, 3L * nF, nF, nullptr, g->fn, 3L * nF, fvalid, nF,
                                                   g->cos_min, B, 0, reinterpret_cast<int32_t*>(wsb + L.bidx), bnd, L.nn_bytes ? wsb + L.nn : nullptr,
                                                   L.nn_bytes, stream);
            if (rc != SH_OK) return rc;
            p.bound = bnd;
        }
    }
    const SurfGate gate = g ? *g : SurfGate{};
    {
        ShProfScope ps(st, "%s|B=%d nq=%d nF=%d chunks=%d cull=%d", g ? "surface_search_gated_kernel" : "surface_search_kernel", B, nq, nF, p.chunks,
                       p.cull);
        const dim3 grid((unsigned)sh_cdiv(nq, QT), (unsigned)p.chunks, (unsigned)B);
        auto kern = g ? (p.stats ? surface_search_kernel<true, true> : surface_search_kernel<false, true>)
                      : (p.stats ? surface_search_kernel<true, false> : surface_search_kernel<false, false>);
        SH_LAUNCH_PS(ps, kern, grid, dim3(NT), 0, st, p, part_idx, part_d2, gate);
    }
    {
        ShProfScope ps(st, "%s|B=%d nq=%d chunks=%d", g ? "surface_finish_gated_kernel" : "surface_finish_kernel", B, nq, p.chunks);
        auto kern = g ? surface_finish_kernel<true> : surface_finish_kernel<false>;
        SH_LAUNCH_PS(ps, kern, dim3((unsigned)(((long)B * nq + 255) / 256)), dim3(256), 0, st, p, B, part_idx, part_d2, face, d2, uv, gate);
    }
    SH_CHECK_LAUNCH(who + 3);                                            // named without the "sh_", as ever
    return SH_OK;
}

}  // namespace

extern "C" {

int sh_nearest_surface_chunks(int B, int nq, int nF) {
    int tpc;
    return nn_resolve_chunks(B, nq, nF, FT, QT, 0, &tpc);
}

size_t sh_nearest_surface_workspace(int B, int nq, int nF, int chunks) {
    if (B <= 0 || nq <= 0 || nF < 0 || chunks < 0) return 0;
    int tpc;
    return surf_layout(B, nq, nF, nn_resolve_chunks(B, nq, nF, FT, QT, chunks, &tpc), false).total;
}

size_t sh_nearest_surface_gated_workspace(int B, int nq, int nF, int chunks) {
    if (B <= 0 || nq <= 0 || nF < 0 || chunks < 0) return 0;
    int tpc;
    return surf_layout(B, nq, nF, nn_resolve_chunks(B, nq, nF, FT, QT, chunks, &tpc), true).total;
}

int sh_nearest_surface(const float* q, int64_t q_sb, int nq, const int32_t* q_count, const float* x, int64_t x_sb, int n,
                       const int32_t* faces, int nF, const uint8_t* v_mask, int64_t mask_sb, const float* bound, int B, int chunks,
                       int cull, int32_t* face, float* d2, float* uv, uint64_t* stats, void* workspace, size_t workspace_bytes,
                       sh_stream_t stream) {
    return surf_search("sh_nearest_surface", q, q_sb, nq, q_count, x, x_sb, n, faces, nF, v_mask, mask_sb, bound, nullptr, B, chunks, cull, face, d2,
                       uv, stats, workspace, workspace_bytes, stream);
}

int sh_nearest_surface_gated(const float* q, int64_t q_sb, int nq, const int32_t* q_count, const float* qn, int64_t qn_sb, const float* x,
                             int64_t x_sb, int n, const int32_t* faces, int nF, const float* fn, const uint8_t* v_mask, int64_t mask_sb,
                             float cos_min, const float* bound, int B, int chunks, int cull, int32_t* face, float* d2, float* uv,
                             uint64_t* stats, void* workspace, size_t workspace_bytes, sh_stream_t stream) {
    const SurfGate g{qn, (long)qn_sb, fn, cos_min};
    return surf_search("sh_nearest_surface_gated", q, q_sb, nq, q_count, x, x_sb, n, faces, nF, v_mask, mask_sb, bound, &g, B, chunks, cull, face, d2,
                       uv, stats, workspace, workspace_bytes, stream);
}

int sh_face_normals(const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, int B, float* normals, sh_stream_t stream) {
    SH_REQUIRE(x && normals && (faces || nF == 0), SH_ERR_INVALID_ARG, "sh_face_normals: null pointer");
    SH_REQUIRE(B >= 0 && n >= 0 && nF >= 0, SH_ERR_INVALID_ARG, "sh_face_normals: negative size (B %d, n %d, nF %d)", B, n, nF);
    if (B == 0 || nF == 0) return SH_OK;
    SH_REQUIRE(x_sb >= 3L * n, SH_ERR_INVALID_ARG, "sh_face_normals: batch stride %ld shorter than a body", (long)x_sb);
    SH_REQUIRE((long)B * nF < (1L << 27), SH_ERR_UNSUPPORTED, "sh_face_normals: B*nF too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "face_normals_kernel|B=%d n=%d nF=%d", B, n, nF);
    SH_LAUNCH_PS(ps, face_normals_kernel, dim3((unsigned)(((long)B * nF + 255) / 256)), dim3(256), 0, st, x, (long)x_sb, n, faces, nF, B, normals);
    SH_CHECK_LAUNCH("face_normals");
    return SH_OK;
}

}  // extern "C"
