// Fitting to unregistered point clouds: brute-force nearest-point search and the Chamfer loss built on it
// (include/sh_kernels.h, "Nearest points and Chamfer loss").  The reference has no counterpart; the search follows the part
// pair-distance sweep of part_loss.hip: queries in registers, targets streamed through LDS, every lane reading the same LDS
// address (broadcast).  No float atomics: the search keeps (d2, index) under the lexicographic minimum, which is associative and
// commutative, and the loss / gradient sums run in a fixed order - the same bits on every call and for every split of the targets.
#include "sh_nn.h"

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int QPT = 4;           // queries a thread keeps in registers
constexpr int QT = NT * QPT;     // queries per workgroup
constexpr int TT = 256;          // targets per LDS tile: one global load per thread and tile

struct NNParams {
    const float* q; long q_sb; int nq; const int32_t* q_count;
    const float* t; long t_sb; int nt; const int32_t* t_count;
    const unsigned char* mask; long mask_sb;
    int tiles_per_chunk, chunks;
};

// The normal gate of the header ("Vertex normals"): the queries' and the targets' normals and the smallest cosine that pairs them.
struct NNGate {
    const float* qn; long qn_sb;
    const float* tn; long tn_sb;
    float cos_min;
};

// grid (query tile, target chunk, body).  final != 0: the one chunk's result is the result (idx / d2 [B][nq]); otherwise the
// chunk's (d2, idx) go to part_d2 / part_idx [B][chunks][nq] for nearest_merge_kernel.
// A target that is masked, or lies beyond the body's count, enters LDS as (+inf, +inf, +inf): its distance is +inf, which the
// strict `<` never selects, so the inner loop carries no index test.  Targets are visited in ascending order and a candidate
// replaces the best only when strictly closer: the lowest index wins an exact tie.
// GATED: a target is a candidate only when the fp32 dot product of the two normals reaches g.cos_min - three more LDS arrays,
// three more query registers.  The gate is one compare and one select on the candidate distance (d = ok ? d : +inf), so a
// gated-out target loses exactly as a masked one does and the (d2, index) minimum stays the lexicographic one.  Target normals
// of masked / out-of-count targets enter as zeros: their distance is +inf whatever the gate says.  Without GATED, g is not read
// and the gate's arrays and registers do not exist.
template <bool GATED>
__global__ __launch_bounds__(NT) void nearest_search_kernel(const NNParams p, int32_t* __restrict__ idx, float* __restrict__ d2, int final,
                                                           const NNGate g) {
    __shared__ __attribute__((aligned(16))) float sx[2][TT];
    __shared__ __attribute__((aligned(16))) float sy[2][TT];
    __shared__ __attribute__((aligned(16))) float sz[2][TT];
    __shared__ __attribute__((aligned(16))) float su[GATED ? 2 : 1][GATED ? TT : 4];
    __shared__ __attribute__((aligned(16))) float sv[GATED ? 2 : 1][GATED ? TT : 4];
    __shared__ __attribute__((aligned(16))) float sw[GATED ? 2 : 1][GATED ? TT : 4];
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
    const int nqb = clamp_count(p.q_count, b, p.nq), ntb = clamp_count(p.t_count, b, p.nt);
    const int j0 = blockIdx.x * QT;
    if (j0 >= nqb) {                                                     // uniform: no query of this tile is live
        if (final)
            for (int k = 0; k < QPT; ++k) {
                const int j = j0 + k * NT + tid;
                if (j < p.nq) { idx[(long)b * p.nq + j] = -1; d2[(long)b * p.nq + j] = 0.f; }
            }
        return;
    }
    const float* qb = p.q + (long)b * p.q_sb;
    const float* tb = p.t + (long)b * p.t_sb;
    const float* qnb = GATED ? g.qn + (long)b * g.qn_sb : nullptr;
    const float* tnb = GATED ? g.tn + (long)b * g.tn_sb : nullptr;
    const unsigned char* mb = p.mask ? p.mask + (long)b * p.mask_sb : nullptr;
    const float cos_min = g.cos_min;
    float qx[QPT], qy[QPT], qz[QPT], qu[QPT], qv[QPT], qw[QPT], best[QPT];
    int bi[QPT];
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int j = j0 + k * NT + tid;
        const bool live = j < nqb;
        qx[k] = live ? qb[3L * j] : 0.f; qy[k] = live ? qb[3L * j + 1] : 0.f; qz[k] = live ? qb[3L * j + 2] : 0.f;
        if constexpr (GATED) { qu[k] = live ? qnb[3L * j] : 0.f; qv[k] = live ? qnb[3L * j + 1] : 0.f; qw[k] = live ? qnb[3L * j + 2] : 0.f; }
        best[k] = INFINITY; bi[k] = -1;
    }
    const int tiles = (ntb + TT - 1) / TT;
    const int tile_lo = c * p.tiles_per_chunk;
    const int tile_hi = min(tile_lo + p.tiles_per_chunk, tiles);
    if (tile_lo < tile_hi) {                                             // uniform
        float lx, ly, lz, lu, lv, lw;
        auto fetch = [&](int tile) {
            const int i = tile * TT + tid;
            const bool ok = i < ntb && (!mb || mb[i] != 0);
            lx = ok ? tb[3L * i] : INFINITY; ly = ok ? tb[3L * i + 1] : INFINITY; lz = ok ? tb[3L * i + 2] : INFINITY;
            if constexpr (GATED) { lu = ok ? tnb[3L * i] : 0.f; lv = ok ? tnb[3L * i + 1] : 0.f; lw = ok ? tnb[3L * i + 2] : 0.f; }
        };
        auto stage = [&](int buf) {
            sx[buf][tid] = lx; sy[buf][tid] = ly; sz[buf][tid] = lz;
            if constexpr (GATED) { su[buf][tid] = lu; sv[buf][tid] = lv; sw[buf][tid] = lw; }
        };
        fetch(tile_lo);
        stage(0);
        __syncthreads();
        for (int tile = tile_lo; tile < tile_hi; ++tile) {
            const int cur = (tile - tile_lo) & 1;
            const bool more = tile + 1 < tile_hi;
            if (more) fetch(tile + 1);                                   // in flight under this tile's arithmetic
            const int base = tile * TT;
#pragma unroll 2
            for (int u = 0; u < TT; u += 4) {
                const f32x4 X = *reinterpret_cast<const f32x4*>(&sx[cur][u]);
                const f32x4 Y = *reinterpret_cast<const f32x4*>(&sy[cur][u]);
                const f32x4 Z = *reinterpret_cast<const f32x4*>(&sz[cur][u]);
                f32x4 U, V, W;
                if constexpr (GATED) {
                    U = *reinterpret_cast<const f32x4*>(&su[cur][u]);
                    V = *reinterpret_cast<const f32x4*>(&sv[cur][u]);
                    W = *reinterpret_cast<const f32x4*>(&sw[cur][u]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int k = 0; k < QPT; ++k) {
                        float d = nn_d2(qx[k], qy[k], qz[k], X[e], Y[e], Z[e]);
                        if constexpr (GATED) {
                            const float dot = __builtin_fmaf(qw[k], W[e], __builtin_fmaf(qv[k], V[e], qu[k] * U[e]));
                            d = dot >= cos_min ? d : INFINITY;            // a NaN compares false: not compatible
                        }
                        const bool closer = d < best[k];
                        best[k] = closer ? d : best[k];
                        bi[k] = closer ? base + u + e : bi[k];
                    }
                }
            }
            if (more) stage(cur ^ 1);
            __syncthreads();                                             // one barrier per tile: the other buffer was last read before the previous one
        }
    }
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int j = j0 + k * NT + tid;
        if (j >= p.nq) continue;
        if (final) {
            const long o = (long)b * p.nq + j;
            idx[o] = j < nqb ? bi[k] : -1;
            d2[o] = j < nqb ? best[k] : 0.f;
        } else if (j < nqb) {
            const long o = ((long)b * p.chunks + c) * p.nq + j;
            idx[o] = bi[k]; d2[o] = best[k];
        }
    }
}

// (d2, idx) of a query = lexicographic minimum over its chunks.  Chunk c holds lower indices than chunk c + 1, so walking the
// chunks in order with a strict `<` is that minimum.  One thread per (body, query).
__global__ __launch_bounds__(256) void nearest_merge_kernel(const int32_t* __restrict__ part_idx, const float* __restrict__ part_d2,
                                                           const int32_t* __restrict__ q_count, int B, int nq, int chunks,
                                                           int32_t* __restrict__ idx, float* __restrict__ d2) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * nq) return;
    const int b = (int)(t / nq), j = (int)(t - (long)b * nq);
    if (j >= clamp_count(q_count, b, nq)) { idx[t] = -1; d2[t] = 0.f; return; }
    float best = INFINITY;
    int bi = -1;
    for (int c = 0; c < chunks; ++c) {
        const long o = ((long)b * chunks + c) * nq + j;
        const float d = part_d2[o];
        if (d < best) { best = d; bi = part_idx[o]; }
    }
    idx[t] = bi; d2[t] = best;
}

// One workgroup per body.  Stage 1: thread t sums the terms t, t + 256, ... in order (fp64); stage 2: the 256 sums through the
// wave butterfly and the four wave sums in order.  counts[b] = (m_b, n_act).  ROBUST: a term is rho(min(d2, tau2)) of the header's
// "Robust terms"; SH_ROBUST_NONE is the plain sum, scale2 unread.
template <int ROBUST>
__global__ __launch_bounds__(256) void chamfer_fwd_kernel(const float* __restrict__ d2_sm, int M, const int32_t* __restrict__ s_count,
                                                         const float* __restrict__ d2_ms, int rows, int n,
                                                         const unsigned char* __restrict__ v_mask, long mask_sb, float tau2, float w_ms,
                                                         float scale2, float* __restrict__ loss, int32_t* __restrict__ counts) {
    __shared__ double red[3][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int m = clamp_count(s_count, b, M);
    const unsigned char* mb = v_mask ? v_mask + (long)b * mask_sb : nullptr;
    double s1 = 0.0, s2 = 0.0, na = 0.0;
    for (int j = tid; j < m; j += 256) s1 += (double)robust_rho<ROBUST>(fminf(d2_sm[(long)b * M + j], tau2), scale2);
    for (int i = tid; i < n; i += 256) {
        if (mb && mb[i] == 0) continue;
        na += 1.0;
        if (d2_ms) s2 += (double)robust_rho<ROBUST>(fminf(d2_ms[(long)b * rows + i], tau2), scale2);
    }
    s1 = wave_sum_d(s1); s2 = wave_sum_d(s2); na = wave_sum_d(na);
    if ((tid & 63) == 0) { red[0][tid >> 6] = s1; red[1][tid >> 6] = s2; red[2][tid >> 6] = na; }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, c = 0.0, k = 0.0;
        for (int w = 0; w < 4; ++w) { a += red[0][w]; c += red[1][w]; k += red[2][w]; }
        double L = 0.0;
        if (m > 0) {
            L = a / (double)m;
            if (d2_ms && w_ms > 0.f && k > 0.0) L += (double)w_ms * c / k;
        }
        loss[b] = (float)L;
        counts[2 * b] = m; counts[2 * b + 1] = (int)k;
    }
}

// Gradient w.r.t. the model points, gather form.  grid (row tile of 256, body), thread = one row i.  The scan -> model indices are
// swept in tiles of 256: thread t looks at entry j = base + t and keeps it when its (untruncated) index lies in this workgroup's
// row range; the kept entries are compacted into LDS in ascending j (wave ballot, waves in order), and every thread then walks
// that short list and adds the terms whose row is its own - ascending j, the order the header states, whatever the scheduling.
// ROBUST: a kept pair's term carries the weight w(d2) of the header's "Robust terms" - one more LDS list, one fused multiply-add
// per term in place of the addition; SH_ROBUST_NONE has neither the list nor the weight.
template <int ROBUST>
__device__ __forceinline__ float* weight_list() {                       // the list exists in the robust instantiations only
    if constexpr (ROBUST != 0) {
        __shared__ float w[256];
        return w;
    } else {
        return nullptr;
    }
}

template <int ROBUST>
__global__ __launch_bounds__(256) void chamfer_bwd_kernel(const float* __restrict__ x, long x_sb, int rows, int n,
                                                         const float* __restrict__ s, long s_sb, int M, const int32_t* __restrict__ s_count,
                                                         const int32_t* __restrict__ idx_sm, const float* __restrict__ d2_sm,
                                                         const int32_t* __restrict__ idx_ms, const float* __restrict__ d2_ms,
                                                         const unsigned char* __restrict__ v_mask, long mask_sb,
                                                         const int32_t* __restrict__ counts, float tau2, float w_ms, float scale2,
                                                         const float* __restrict__ gL, float* __restrict__ g_x) {
    __shared__ int wave_n[4];
    __shared__ int list_j[256];
    __shared__ int list_r[256];
    float* const list_w = weight_list<ROBUST>();
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i_lo = blockIdx.x * 256, i = i_lo + tid;
    const int m = min(clamp_count(s_count, b, M), counts[2 * b]);
    const int n_act = counts[2 * b + 1];
    const float* xb = x + (long)b * x_sb;
    const float* sb = s + (long)b * s_sb;
    const bool mine = i < n;
    const float xi0 = mine ? xb[3L * i] : 0.f, xi1 = mine ? xb[3L * i + 1] : 0.f, xi2 = mine ? xb[3L * i + 2] : 0.f;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    float wt = 0.f, wt_next = 0.f;                                       // the weights of id / id_next, ROBUST only
    auto fetch = [&](int base, float& w) {
        const int j = base + tid;
        if (j >= m) return -1;
        const float d = d2_sm[(long)b * M + j];
        if (!(d < tau2)) return -1;
        if constexpr (ROBUST != 0) w = robust_weight<ROBUST>(d, scale2);   // kept pairs only: a truncated one costs no division
        return idx_sm[(long)b * M + j];
    };
    int id = m > 0 ? fetch(0, wt) : -1;
    for (int base = 0; base < m; base += 256) {                         // m is uniform over the workgroup
        const int id_next = base + 256 < m ? fetch(base + 256, wt_next) : -1;   // in flight under this tile's compaction
        const bool hit = (unsigned)(id - i_lo) < 256u;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wave_n[wv] = __popcll(bal);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < 4; ++w) { off += w < wv ? wave_n[w] : 0; total += wave_n[w]; }
        if (hit) {
            const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
            list_j[pos] = base + tid; list_r[pos] = id - i_lo;
            if constexpr (ROBUST != 0) list_w[pos] = wt;
        }
        __syncthreads();
        for (int k = 0; k < total; ++k)
            if (list_r[k] == tid && mine) {
                const long j = list_j[k];
                if constexpr (ROBUST != 0) {
                    const float w = list_w[k];
                    a0 = __builtin_fmaf(w, xi0 - sb[3 * j], a0); a1 = __builtin_fmaf(w, xi1 - sb[3 * j + 1], a1);
                    a2 = __builtin_fmaf(w, xi2 - sb[3 * j + 2], a2);
                } else {
                    a0 += xi0 - sb[3 * j]; a1 += xi1 - sb[3 * j + 1]; a2 += xi2 - sb[3 * j + 2];
                }
            }
        __syncthreads();                                                 // the lists are rewritten by the next tile
        id = id_next; wt = wt_next;
    }
    if (i >= rows) return;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    const bool active = mine && !(v_mask && v_mask[(long)b * mask_sb + i] == 0);
    if (active && m > 0) {
        const float g = gL[b];
        const float c1 = 2.f / (float)m;
        g0 = c1 * a0; g1 = c1 * a1; g2 = c1 * a2;
        if (idx_ms && w_ms > 0.f && n_act > 0) {
            const int k = idx_ms[(long)b * rows + i];
            if (k >= 0 && k < m && d2_ms[(long)b * rows + i] < tau2) {
                float c2 = w_ms * 2.f / (float)n_act;
                if constexpr (ROBUST != 0) c2 *= robust_weight<ROBUST>(d2_ms[(long)b * rows + i], scale2);
                g0 += c2 * (xi0 - sb[3L * k]); g1 += c2 * (xi1 - sb[3L * k + 1]); g2 += c2 * (xi2 - sb[3L * k + 2]);
            }
        }
        g0 *= g; g1 *= g; g2 *= g;
    }
    float* o = g_x + ((long)b * rows + i) * 3;
    o[0] = g0; o[1] = g1; o[2] = g2;
}

// The same gradient when the partner of a scan point is the foot point (face, uv) that sh_nearest_surface recorded on the table
// `faces` (header, "Nearest surface points"), the discipline of chamfer_bwd_kernel: whoever changes the kept rule, the order of
// the sums or the epilogue of one changes the other, and tests/test_chamfer_bwd_bits.py holds the bytes of both.  grid (row tile of
// 256, body), thread = one row i.  The recorded faces are swept in tiles of 256 scan points: thread t looks at entry j = base + t and keeps the
// corners of its face that lie in this workgroup's row range; the kept (row, weight, q - s) entries are compacted into LDS in
// ascending j and corner order 0, 1, 2 within a j (wave ballots, waves in order), and every thread then walks that short list
// and adds the terms whose row is its own - the order the header states, whatever the scheduling.  ROBUST: the pair's q - s is
// multiplied by its weight w(d2) once, before the corners' barycentric weights; SH_ROBUST_NONE is the plain walk.
template <int ROBUST>
__global__ __launch_bounds__(256) void surface_bwd_kernel(const float* __restrict__ x, long x_sb, int rows, int n,
                                                         const float* __restrict__ s, long s_sb, int M, const int32_t* __restrict__ s_count,
                                                         const int32_t* __restrict__ faces, int nF, const int32_t* __restrict__ face,
                                                         const float* __restrict__ d2, const float* __restrict__ uv,
                                                         const int32_t* __restrict__ idx_ms, const float* __restrict__ d2_ms,
                                                         const unsigned char* __restrict__ v_mask, long mask_sb,
                                                         const int32_t* __restrict__ counts, float tau2, float w_ms, float scale2,
                                                         const float* __restrict__ gL, float* __restrict__ g_x) {
#pragma clang fp contract(off)
    __shared__ int wave_n[4];
    __shared__ int list_r[768];
    __shared__ float list_l[768];
    __shared__ float list_x[768];
    __shared__ float list_y[768];
    __shared__ float list_z[768];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i_lo = blockIdx.x * 256, i = i_lo + tid;
    const int m = min(clamp_count(s_count, b, M), counts[2 * b]);
    const int n_act = counts[2 * b + 1];
    const float* xb = x + (long)b * x_sb;
    const float* sb = s + (long)b * s_sb;
    const bool mine = i < n;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < m; base += 256) {                         // m is uniform over the workgroup
        const int j = base + tid;
        int r[3] = {-1, -1, -1};
        float l[3] = {0.f, 0.f, 0.f}, ex = 0.f, ey = 0.f, ez = 0.f;
        if (j < m) {
            const long o = (long)b * M + j;
            const int f = face[o];
            if (f >= 0 && f < nF && d2[o] < tau2) {
                const int i0 = faces[3L * f], i1 = faces[3L * f + 1], i2 = faces[3L * f + 2];
                const bool ok = (unsigned)i0 < (unsigned)n && (unsigned)i1 < (unsigned)n && (unsigned)i2 < (unsigned)n;
                const bool h0 = (unsigned)(i0 - i_lo) < 256u, h1 = (unsigned)(i1 - i_lo) < 256u, h2 = (unsigned)(i2 - i_lo) < 256u;
                if (ok && (h0 || h1 || h2)) {
                    const float v = uv[2 * o], w = uv[2 * o + 1];
                    const float ax = xb[3L * i0], ay = xb[3L * i0 + 1], az = xb[3L * i0 + 2];
                    const float abx = xb[3L * i1] - ax, aby = xb[3L * i1 + 1] - ay, abz = xb[3L * i1 + 2] - az;
                    const float acx = xb[3L * i2] - ax, acy = xb[3L * i2 + 1] - ay, acz = xb[3L * i2 + 2] - az;
                    const float apx = sb[3L * j] - ax, apy = sb[3L * j + 1] - ay, apz = sb[3L * j + 2] - az;
                    ex = __builtin_fmaf(w, acx, v * abx) - apx;          // q - s, the exact negative of the forward pass's residual
                    ey = __builtin_fmaf(w, acy, v * aby) - apy;
                    ez = __builtin_fmaf(w, acz, v * abz) - apz;
                    if constexpr (ROBUST != 0) {
                        const float wr = robust_weight<ROBUST>(d2[o], scale2);
                        ex = wr * ex; ey = wr * ey; ez = wr * ez;
                    }
                    l[0] = (1.0f - v) - w; l[1] = v; l[2] = w;
                    r[0] = h0 ? i0 - i_lo : -1; r[1] = h1 ? i1 - i_lo : -1; r[2] = h2 ? i2 - i_lo : -1;
                }
            }
        }
        const unsigned long long b0 = __ballot(r[0] >= 0), b1 = __ballot(r[1] >= 0), b2 = __ballot(r[2] >= 0);
        if (lane == 0) wave_n[wv] = __popcll(b0) + __popcll(b1) + __popcll(b2);
        __syncthreads();
        int off = 0, total = 0;
        for (int w_ = 0; w_ < 4; ++w_) { off += w_ < wv ? wave_n[w_] : 0; total += wave_n[w_]; }
        int pos = off + __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (r[k] >= 0) { list_r[pos] = r[k]; list_l[pos] = l[k]; list_x[pos] = ex; list_y[pos] = ey; list_z[pos] = ez; ++pos; }
        __syncthreads();
        for (int k = 0; k < total; ++k)
            if (list_r[k] == tid && mine) {
                const float lk = list_l[k];
                a0 = a0 + lk * list_x[k]; a1 = a1 + lk * list_y[k]; a2 = a2 + lk * list_z[k];
            }
        __syncthreads();                                                 // the lists are rewritten by the next tile
    }
    if (i >= rows) return;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    const bool active = mine && !(v_mask && v_mask[(long)b * mask_sb + i] == 0);
    if (active && m > 0) {
        const float g = gL[b];
        const float c1 = 2.f / (float)m;
        g0 = c1 * a0; g1 = c1 * a1; g2 = c1 * a2;
        if (idx_ms && w_ms > 0.f && n_act > 0) {
            const int k = idx_ms[(long)b * rows + i];
            if (k >= 0 && k < m && d2_ms[(long)b * rows + i] < tau2) {
                float c2 = w_ms * 2.f / (float)n_act;
                if constexpr (ROBUST != 0) c2 = c2 * robust_weight<ROBUST>(d2_ms[(long)b * rows + i], scale2);
                const float xi0 = xb[3L * i], xi1 = xb[3L * i + 1], xi2 = xb[3L * i + 2];
                g0 = g0 + c2 * (xi0 - sb[3L * k]); g1 = g1 + c2 * (xi1 - sb[3L * k + 1]); g2 = g2 + c2 * (xi2 - sb[3L * k + 2]);
            }
        }
        g0 *= g; g1 *= g; g2 *= g;
    }
    float* o = g_x + ((long)b * rows + i) * 3;
    o[0] = g0; o[1] = g1; o[2] = g2;
}

// ------------------------------------------------------------------------------------------------ normals (header: "Vertex normals")
// Area-weighted vertex normals, gather form: one thread per (body, vertex) walks the vertex's incident faces in the order of the
// incidence table (ascending face) and sums the faces' cross products in fp32 - the header's expression, no contraction beyond
// the fused multiply-adds written out, so the numpy transcription of tests/normals_ref.py rounds alike.  An entry of either table
// outside its range is passed over (scan.FaceTable never builds one).
__global__ __launch_bounds__(256) void vertex_normals_kernel(const float* __restrict__ x, long x_sb, int n, const int32_t* __restrict__ faces,
                                                            int nF, const int32_t* __restrict__ vf_ptr, const int32_t* __restrict__ vf_idx,
                                                            int B, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * n) return;
    const int b = (int)(t / n), v = (int)(t - (long)b * n);
    const float* xb = x + (long)b * x_sb;
    int lo = vf_ptr[v], hi = vf_ptr[v + 1];
    lo = max(lo, 0); hi = min(hi, 3 * nF);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int e = lo; e < hi; ++e) {
        const int f = vf_idx[e];
        if ((unsigned)f >= (unsigned)nF) continue;
        int i0, i1, i2;
        if (!face_corners(faces, f, n, i0, i1, i2)) continue;
        float cx, cy, cz;
        face_cross(xb + 3L * i0, xb + 3L * i1, xb + 3L * i2, cx, cy, cz);
        sx = sx + cx; sy = sy + cy; sz = sz + cz;
    }
    const float len2 = __builtin_fmaf(sz, sz, __builtin_fmaf(sy, sy, sx * sx));
    const bool ok = len2 > 0.f && len2 < INFINITY;
    const float len = sqrtf(len2);
    float* o = out + t * 3;
    o[0] = ok ? sx / len : 0.f; o[1] = ok ? sy / len : 0.f; o[2] = ok ? sz / len : 0.f;
}

// sh_nearest_points (g == nullptr) and sh_nearest_points_gated: the checks both make, in the order the header states, the split,
// the workspace and the launches.  `who` is the entry point's name in every error text.
int nn_search(const char* who, NNParams p, const NNGate* g, int B, int chunks, int32_t* idx, float* d2, void* workspace,
              size_t workspace_bytes, sh_stream_t stream) {
    const int nq = p.nq, nt = p.nt;
    SH_REQUIRE(p.q && p.t && idx && d2, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(B >= 0 && nq >= 0 && nt >= 0 && chunks >= 0, SH_ERR_INVALID_ARG, "%s: negative size (B %d, nq %d, nt %d, chunks %d)", who, B, nq,
               nt, chunks);
    SH_REQUIRE(!g || g->cos_min == g->cos_min, SH_ERR_INVALID_ARG, "%s: cos_min is NaN", who);
    if (B == 0 || nq == 0) return SH_OK;
    SH_REQUIRE(p.q_sb >= 3L * nq && p.t_sb >= 3L * nt && (!p.mask || p.mask_sb == 0 || p.mask_sb >= nt), SH_ERR_INVALID_ARG,
               "%s: batch stride shorter than a body (q_sb %ld, t_sb %ld, mask_sb %ld)", who, p.q_sb, p.t_sb, p.mask_sb);
    SH_REQUIRE(!g || (g->qn_sb >= 3L * nq && g->tn_sb >= 3L * nt), SH_ERR_INVALID_ARG,
               "%s: batch stride shorter than a body (qn_sb %ld, tn_sb %ld)", who, g ? g->qn_sb : 0L, g ? g->tn_sb : 0L);
    SH_REQUIRE(B <= 65535 && (long)B * nq < (1L << 30) && nt < (1 << 30), SH_ERR_UNSUPPORTED, "%s: B, B*nq or nt too large", who);
    p.chunks = nn_resolve_chunks(B, nq, nt, TT, QT, chunks, &p.tiles_per_chunk);
    SH_REQUIRE(p.chunks <= 65535, SH_ERR_UNSUPPORTED, "%s: %d target chunks", who, p.chunks);
    const size_t need = p.chunks <= 1 ? 0 : (size_t)B * p.chunks * nq * (sizeof(float) + sizeof(int32_t));
    SH_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), SH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes needed for %d chunks)",
               who, need, p.chunks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)sh_cdiv(nq, QT), (unsigned)p.chunks, (unsigned)B);
    const int final = p.chunks <= 1;
    float* part_d2 = final ? d2 : static_cast<float*>(workspace);
    int32_t* part_idx = final ? idx : reinterpret_cast<int32_t*>(part_d2 + (size_t)B * p.chunks * nq);
    if (g) {
        ShProfScope ps(st, "nearest_search_gated_kernel|B=%d nq=%d nt=%d chunks=%d", B, nq, nt, p.chunks);
        SH_LAUNCH_PS(ps, nearest_search_kernel<true>, grid, dim3(NT), 0, st, p, part_idx, part_d2, final, *g);
    } else {
        ShProfScope ps(st, "nearest_search_kernel|B=%d nq=%d nt=%d chunks=%d", B, nq, nt, p.chunks);
        SH_LAUNCH_PS(ps, nearest_search_kernel<false>, grid, dim3(NT), 0, st, p, part_idx, part_d2, final, NNGate{});
    }
    if (!final) {
        ShProfScope ps(st, "nearest_merge_kernel|B=%d nq=%d chunks=%d", B, nq, p.chunks);
        SH_LAUNCH_PS(ps, nearest_merge_kernel, dim3((unsigned)(((long)B * nq + 255) / 256)), dim3(256), 0, st, part_idx, part_d2, p.q_count, B, nq,
                     p.chunks, idx, d2);
    }
    SH_CHECK_LAUNCH(who + 3);                                            // named without the "sh_", as ever
    return SH_OK;
}

// What the surface form's partner adds to the vertex form's arguments: the table and the foot points' weights (the recorded
// face and the surface distance take the place of idx_sm and d2_sm).
struct BwdSurface { const int32_t* faces; int nF; const float* uv; };

// sh_chamfer_bwd (sf == nullptr), sh_chamfer_surface_bwd and their _robust twins: the checks all make, then the launch of the
// robust form's instantiation (SH_ROBUST_NONE: the plain kernels under their plain names).  `who` is the entry point's name in
// every error text.
int chamfer_bwd(const char* who, const float* x, int64_t x_sb, int rows, int n, const float* s, int64_t s_sb, int M, const int32_t* s_count,
                const int32_t* idx_sm, const float* d2_sm, const BwdSurface* sf, const int32_t* idx_ms, const float* d2_ms, const uint8_t* v_mask,
                int64_t mask_sb, const int32_t* counts, float tau2, float w_ms, int robust, float scale2, const float* gL, int B, float* g_x,
                sh_stream_t stream) {
    if (const int rc = robust_check(who, robust, scale2)) return rc;
    SH_REQUIRE(x && s && idx_sm && d2_sm && counts && gL && g_x && (!sf || (sf->uv && (sf->faces || sf->nF == 0))), SH_ERR_INVALID_ARG,
               "%s: null pointer", who);
    SH_REQUIRE(B >= 0 && M >= 0 && rows >= 0 && n >= 0 && n <= rows && (!sf || sf->nF >= 0), SH_ERR_INVALID_ARG,       // each its own text
               sf ? "%s: bad size (B %d, M %d, rows %d, n %d, nF %d)" : "%s: bad size (B %d, M %d, rows %d, n %d)", who, B, M, rows, n, sf ? sf->nF : 0);
    SH_REQUIRE(w_ms >= 0.f && tau2 >= 0.f, SH_ERR_INVALID_ARG, "%s: w_ms and tau2 must be >= 0 (and not NaN)", who);
    SH_REQUIRE((idx_ms != nullptr) == (d2_ms != nullptr), SH_ERR_INVALID_ARG, "%s: idx_ms and d2_ms come together", who);
    if (B == 0 || rows == 0) return SH_OK;
    SH_REQUIRE(x_sb >= 3L * rows && s_sb >= 3L * M && (!v_mask || mask_sb == 0 || mask_sb >= n), SH_ERR_INVALID_ARG,
               "%s: batch stride shorter than a body (x_sb %ld, s_sb %ld, mask_sb %ld)", who, (long)x_sb, (long)s_sb, (long)mask_sb);
    SH_REQUIRE(B <= 65535 && (long)B * rows < (1L << 30), SH_ERR_UNSUPPORTED, "%s: B or B*rows too large", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)sh_cdiv(rows, 256), (unsigned)B);
    if (w_ms <= 0.f) idx_ms = nullptr;                                   // the kernels read the model -> scan matches only through idx_ms
    const char* name = sf ? (robust ? "surface_bwd_robust_kernel" : "surface_bwd_kernel") : (robust ? "chamfer_bwd_robust_kernel" : "chamfer_bwd_kernel");
    ShProfScope ps(st, robust ? "%s|B=%d M=%d rows=%d robust=%d" : "%s|B=%d M=%d rows=%d", name, B, M, rows, robust);
    robust_dispatch(robust, [&](auto form) {
        constexpr int R = decltype(form)::value;
        if (sf)
            SH_LAUNCH_PS(ps, surface_bwd_kernel<R>, grid, dim3(256), 0, st, x, (long)x_sb, rows, n, s, (long)s_sb, M, s_count, sf->faces, sf->nF,
                         idx_sm, d2_sm, sf->uv, idx_ms, d2_ms, v_mask, (long)mask_sb, counts, tau2, w_ms, scale2, gL, g_x);
        else
            SH_LAUNCH_PS(ps, chamfer_bwd_kernel<R>, grid, dim3(256), 0, st, x, (long)x_sb, rows, n, s, (long)s_sb, M, s_count, idx_sm, d2_sm,
                         idx_ms, d2_ms, v_mask, (long)mask_sb, counts, tau2, w_ms, scale2, gL, g_x);
    });
    SH_CHECK_LAUNCH(who + 3);                                            // named without the "sh_", as ever
    return SH_OK;
}

// sh_chamfer_fwd and its _robust twin: the checks both make, then the launch of the robust form's instantiation.
int chamfer_fwd(const char* who, const float* d2_sm, int M, const int32_t* s_count, const float* d2_ms, int rows, int n, const uint8_t* v_mask,
                int64_t mask_sb, float tau2, float w_ms, int robust, float scale2, int B, float* loss, int32_t* counts, sh_stream_t stream) {
    if (const int rc = robust_check(who, robust, scale2)) return rc;
    SH_REQUIRE(d2_sm && loss && counts, SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(B >= 0 && M >= 0 && rows >= 0 && n >= 0 && n <= rows, SH_ERR_INVALID_ARG, "%s: bad size (B %d, M %d, rows %d, n %d)", who, B, M, rows,
               n);
    SH_REQUIRE(w_ms >= 0.f && tau2 >= 0.f, SH_ERR_INVALID_ARG, "%s: w_ms and tau2 must be >= 0 (and not NaN)", who);
    SH_REQUIRE(!v_mask || mask_sb == 0 || mask_sb >= n, SH_ERR_INVALID_ARG, "%s: mask stride %ld shorter than n", who, (long)mask_sb);
    if (B == 0) return SH_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, robust ? "chamfer_fwd_robust_kernel|B=%d M=%d n=%d robust=%d" : "chamfer_fwd_kernel|B=%d M=%d n=%d", B, M, n, robust);
    robust_dispatch(robust, [&](auto form) {
        SH_LAUNCH_PS(ps, chamfer_fwd_kernel<decltype(form)::value>, dim3((unsigned)B), dim3(256), 0, st, d2_sm, M, s_count,
                     w_ms > 0.f ? d2_ms : nullptr, rows, n, v_mask, (long)mask_sb, tau2, w_ms, scale2, loss, counts);
    });
    SH_CHECK_LAUNCH("chamfer_fwd");
    return SH_OK;
}

}  // namespace

extern "C" {

int sh_nearest_points_chunks(int B, int nq, int nt) {
    if (B <= 0 || nq <= 0) return 1;                                     // nothing to search: not split
    int tpc;
    return nn_resolve_chunks(B, nq, nt, TT, QT, 0, &tpc);
}

size_t sh_nearest_points_workspace(int B, int nq, int nt, int chunks) {
    if (B <= 0 || nq <= 0 || nt < 0 || chunks < 0) return 0;
    int tpc;
    const int c = nn_resolve_chunks(B, nq, nt, TT, QT, chunks, &tpc);
    return c <= 1 ? 0 : (size_t)B * c * nq * (sizeof(float) + sizeof(int32_t));
}

int sh_nearest_points(const float* q, int64_t q_sb, int nq, const int32_t* q_count, const float* t, int64_t t_sb, int nt,
                      const int32_t* t_count, const uint8_t* t_mask, int64_t mask_sb, int B, int chunks, int32_t* idx, float* d2,
                      void* workspace, size_t workspace_bytes, sh_stream_t stream) {
    const NNParams p{q, (long)q_sb, nq, q_count, t, (long)t_sb, nt, t_count, t_mask, (long)mask_sb, 0, 0};
    return nn_search("sh_nearest_points", p, nullptr, B, chunks, idx, d2, workspace, workspace_bytes, stream);
}

int sh_nearest_points_gated(const float* q, int64_t q_sb, int nq, const int32_t* q_count, const float* qn, int64_t qn_sb, const float* t,
                            int64_t t_sb, int nt, const int32_t* t_count, const float* tn, int64_t tn_sb, const uint8_t* t_mask,
                            int64_t mask_sb, float cos_min, int B, int chunks, int32_t* idx, float* d2, void* workspace,
                            size_t workspace_bytes, sh_stream_t stream) {
    SH_REQUIRE(qn && tn, SH_ERR_INVALID_ARG, "sh_nearest_points_gated: null pointer");
    const NNParams p{q, (long)q_sb, nq, q_count, t, (long)t_sb, nt, t_count, t_mask, (long)mask_sb, 0, 0};
    const NNGate g{qn, (long)qn_sb, tn, (long)tn_sb, cos_min};
    return nn_search("sh_nearest_points_gated", p, &g, B, chunks, idx, d2, workspace, workspace_bytes, stream);
}

int sh_vertex_normals(const float* x, int64_t x_sb, int n, const int32_t* faces, int nF, const int32_t* vf_ptr, const int32_t* vf_idx, int B,
                      float* normals, sh_stream_t stream) {
    SH_REQUIRE(x && normals && vf_ptr && (nF == 0 || (faces && vf_idx)), SH_ERR_INVALID_ARG, "sh_vertex_normals: null pointer");
    SH_REQUIRE(B >= 0 && n >= 0 && nF >= 0, SH_ERR_INVALID_ARG, "sh_vertex_normals: negative size (B %d, n %d, nF %d)", B, n, nF);
    if (B == 0 || n == 0) return SH_OK;
    SH_REQUIRE(x_sb >= 3L * n, SH_ERR_INVALID_ARG, "sh_vertex_normals: batch stride %ld shorter than a body", (long)x_sb);
    SH_REQUIRE((long)B * n < (1L << 30) && nF < (1 << 29), SH_ERR_UNSUPPORTED, "sh_vertex_normals: B*n or nF too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "vertex_normals_kernel|B=%d n=%d nF=%d", B, n, nF);
    SH_LAUNCH_PS(ps, vertex_normals_kernel, dim3((unsigned)(((long)B * n + 255) / 256)), dim3(256), 0, st, x, (long)x_sb, n, faces, nF, vf_ptr,
                 vf_idx, B, normals);
    SH_CHECK_LAUNCH("vertex_normals");
    return SH_OK;
}

int sh_chamfer_fwd(const float* d2_sm, int M, const int32_t* s_count, const float* d2_ms, int rows, int n, const uint8_t* v_mask,
                   int64_t mask_sb, float tau2, float w_ms, int B, float* loss, int32_t* counts, sh_stream_t stream) {
    return chamfer_fwd("sh_chamfer_fwd", d2_sm, M, s_count, d2_ms, rows, n, v_mask, mask_sb, tau2, w_ms, SH_ROBUST_NONE, 0.f, B, loss, counts, stream);
}

int sh_chamfer_fwd_robust(const float* d2_sm, int M, const int32_t* s_count, const float* d2_ms, int rows, int n, const uint8_t* v_mask,
                          int64_t mask_sb, float tau2, float w_ms, int B, float* loss, int32_t* counts, sh_stream_t stream, int robust,
                          float scale2) {
    return chamfer_fwd("sh_chamfer_fwd_robust", d2_sm, M, s_count, d2_ms, rows, n, v_mask, mask_sb, tau2, w_ms, robust, scale2, B, loss, counts,
                       stream);
}

int sh_chamfer_bwd(const float* x, int64_t x_sb, int rows, int n, const float* s, int64_t s_sb, int M, const int32_t* s_count,
                   const int32_t* idx_sm, const float* d2_sm, const int32_t* idx_ms, const float* d2_ms, const uint8_t* v_mask,
                   int64_t mask_sb, const int32_t* counts, float tau2, float w_ms, const float* gL, int B, float* g_x, sh_stream_t stream) {
    return chamfer_bwd("sh_chamfer_bwd", x, x_sb, rows, n, s, s_sb, M, s_count, idx_sm, d2_sm, nullptr, idx_ms, d2_ms, v_mask, mask_sb, counts, tau2,
                       w_ms, SH_ROBUST_NONE, 0.f, gL, B, g_x, stream);
}

int sh_chamfer_bwd_robust(const float* x, int64_t x_sb, int rows, int n, const float* s, int64_t s_sb, int M, const int32_t* s_count,
                          const int32_t* idx_sm, const float* d2_sm, const int32_t* idx_ms, const float* d2_ms, const uint8_t* v_mask,
                          int64_t mask_sb, const int32_t* counts, float tau2, float w_ms, const float* gL, int B, float* g_x, sh_stream_t stream,
                          int robust, float scale2) {
    return chamfer_bwd("sh_chamfer_bwd_robust", x, x_sb, rows, n, s, s_sb, M, s_count, idx_sm, d2_sm, nullptr, idx_ms, d2_ms, v_mask, mask_sb, counts,
                       tau2, w_ms, robust, scale2, gL, B, g_x, stream);
}

int sh_chamfer_surface_bwd(const float* x, int64_t x_sb, int rows, int n, const float* s, int64_t s_sb, int M, const int32_t* s_count,
                           const int32_t* faces, int nF, const int32_t* face, const float* d2, const float* uv, const int32_t* idx_ms,
                           const float* d2_ms, const uint8_t* v_mask, int64_t mask_sb, const int32_t* counts, float tau2, float w_ms,
                           const float* gL, int B, float* g_x, sh_stream_t stream) {
    const BwdSurface sf{faces, nF, uv};
    return chamfer_bwd("sh_chamfer_surface_bwd", x, x_sb, rows, n, s, s_sb, M, s_count, face, d2, &sf, idx_ms, d2_ms, v_mask, mask_sb, counts, tau2,
                       w_ms, SH_ROBUST_NONE, 0.f, gL, B, g_x, stream);
}

int sh_chamfer_surface_bwd_robust(const float* x, int64_t x_sb, int rows, int n, const float* s, int64_t s_sb, int M, const int32_t* s_count,
                                  const int32_t* faces, int nF, const int32_t* face, const float* d2, const float* uv, const int32_t* idx_ms,
                                  const float* d2_ms, const uint8_t* v_mask, int64_t mask_sb, const int32_t* counts, float tau2, float w_ms,
                                  const float* gL, int B, float* g_x, sh_stream_t stream, int robust, float scale2) {
    const BwdSurface sf{faces, nF, uv};
    return chamfer_bwd("sh_chamfer_surface_bwd_robust", x, x_sb, rows, n, s, s_sb, M, s_count, face, d2, &sf, idx_ms, d2_ms, v_mask, mask_sb, counts,
                       tau2, w_ms, robust, scale2, gL, B, g_x, stream);
}

}  // extern "C"
