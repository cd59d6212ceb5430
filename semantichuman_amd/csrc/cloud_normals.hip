// Normals of a bare point cloud (include/sh_kernels.h, "Cloud normals"): per point the k nearest points of its own cloud, the
// covariance of that neighbourhood and the eigenvector of its smallest eigenvalue.  The reference has no counterpart.  Two
// sweeps in the form of scan.hip's nearest_search_kernel - queries in registers, targets streamed through LDS, every lane
// reading the same LDS address (broadcast): the first keeps each query's k smallest squared distances, the second sums the
// moments of every point within the k-th.  No atomics, no scratch, no index kept: the neighbourhood is a distance threshold, so
// ties at the k-th distance are all in and the result depends on neither visiting order nor launch shape.
#include "sh_nn.h"

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int TT = 256;          // targets per LDS tile: one global load per thread and tile

// One insertion into a query's ascending list w[0 .. CAP - 1], the largest value dropped: slot i becomes the median of
// (w[i - 1], d, w[i]) - w[i] when d is no smaller, d when it falls between, w[i - 1] when it is smaller than both.  Fully
// unrolled, every index static: the list lives in registers.  A d that is not below the last slot (+inf, to which a lane that
// has nothing to insert sets it) leaves the list as it is.
template <int CAP>
__device__ __forceinline__ void kth_insert(float (&w)[CAP], float d) {
#pragma unroll
    for (int i = CAP - 1; i > 0; --i) w[i] = __builtin_amdgcn_fmed3f(w[i - 1], d, w[i]);
    w[0] = fminf(w[0], d);
}

// Pass 1.  grid (query tile of NT * QPT, body) -> r2 [B][M]: the k_eff-th smallest nn_d2(s_j, s_i) over the live i (self
// included), k_eff = min(k, m_b); 0 for rows beyond the count.  A list of CAP >= k slots serves every k: CAP - k_eff slots start
// at -inf and stay there, k_eff start at +inf, so the last slot is always the k_eff-th smallest value seen and `d < w[CAP - 1]`
// has a static index.  Targets beyond the count enter LDS as +inf: their distance is +inf (or NaN), never below the last slot.
// The insertion runs under a wave ballot - after the first tiles few candidates pass.  QPT only trades LDS reads per distance
// against workgroups: the k-th smallest of a set does not depend on it.
template <int CAP, int QPT>
__global__ __launch_bounds__(NT) void cloud_kth_kernel(const float* __restrict__ s, long s_sb, int M, const int32_t* __restrict__ count, int k,
                                                      float* __restrict__ r2) {
    __shared__ __attribute__((aligned(16))) float sx[2][TT];
    __shared__ __attribute__((aligned(16))) float sy[2][TT];
    __shared__ __attribute__((aligned(16))) float sz[2][TT];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int m = clamp_count(count, b, M);
    const int j0 = blockIdx.x * (NT * QPT);
    float* out = r2 + (long)b * M;
    if (j0 >= m) {                                                       // uniform: no query of this tile is live
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            const int j = j0 + q * NT + tid;
            if (j < M) out[j] = 0.f;
        }
        return;
    }
    const float* sb = s + (long)b * s_sb;
    const int k_eff = min(k, m);
    float qx[QPT], qy[QPT], qz[QPT], w[QPT][CAP];
#pragma unroll
    for (int q = 0; q < QPT; ++q) {
        const int j = j0 + q * NT + tid;
        const bool live = j < m;
        qx[q] = live ? sb[3L * j] : 0.f; qy[q] = live ? sb[3L * j + 1] : 0.f; qz[q] = live ? sb[3L * j + 2] : 0.f;
#pragma unroll
        for (int i = 0; i < CAP; ++i) w[q][i] = i < CAP - k_eff ? -INFINITY : INFINITY;
    }
    const int tiles = (m + TT - 1) / TT;
    float lx, ly, lz;
    auto fetch = [&](int tile) {
        const int i = tile * TT + tid;
        const bool ok = i < m;
        lx = ok ? sb[3L * i] : INFINITY; ly = ok ? sb[3L * i + 1] : INFINITY; lz = ok ? sb[3L * i + 2] : INFINITY;
    };
    auto stage = [&](int buf) { sx[buf][tid] = lx; sy[buf][tid] = ly; sz[buf][tid] = lz; };
    fetch(0);
    stage(0);
    __syncthreads();
    for (int tile = 0; tile < tiles; ++tile) {
        const int cur = tile & 1;
        const bool more = tile + 1 < tiles;
        if (more) fetch(tile + 1);                                       // in flight under this tile's arithmetic
#pragma unroll 2
        for (int u = 0; u < TT; u += 4) {
            const f32x4 X = *reinterpret_cast<const f32x4*>(&sx[cur][u]);
            const f32x4 Y = *reinterpret_cast<const f32x4*>(&sy[cur][u]);
            const f32x4 Z = *reinterpret_cast<const f32x4*>(&sz[cur][u]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int q = 0; q < QPT; ++q) {
                    const float d = nn_d2(qx[q], qy[q], qz[q], X[e], Y[e], Z[e]);
                    const bool in = d < w[q][CAP - 1];                   // a NaN compares false
                    if (__ballot(in) != 0ull) kth_insert<CAP>(w[q], in ? d : INFINITY);
                }
            }
        }
        if (more) stage(cur ^ 1);
        __syncthreads();                                                 // one barrier per tile, as in nearest_search_kernel
    }
#pragma unroll
    for (int q = 0; q < QPT; ++q) {
        const int j = j0 + q * NT + tid;
        if (j < M) out[j] = j < m ? w[q][CAP - 1] : 0.f;
    }
}

// Pass 2 and the finish.  grid (query tile of NT, body), one query per thread.  The whole body is swept once more, in ascending
// i, never split: candidate i is a member iff nn_d2(s_j, s_i) <= r2[j], and the fp64 moments of d = s_i - s_j (fp32 differences,
// widened; their products are exact in fp64) are added under a wave ballot - about k of M candidates are members.  Targets
// beyond the count enter LDS as NaN here: no compare admits them, even against an r2 that overflowed to +inf.  Then, per point:
// the covariance, the 3 x 3 cyclic Jacobi (SH_CLOUD_JACOBI_SWEEPS sweeps, select form, no convergence test), the eigenvector of
// the smallest eigenvalue, the sign, the surface variation - the header's rules one by one.
__global__ __launch_bounds__(NT) void cloud_normals_kernel(const float* __restrict__ s, long s_sb, int M, const int32_t* __restrict__ count,
                                                          const float* __restrict__ r2, const float* __restrict__ view, long view_sb,
                                                          long view_ps, float* __restrict__ nrm, float* __restrict__ var,
                                                          int32_t* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float sx[2][TT];
    __shared__ __attribute__((aligned(16))) float sy[2][TT];
    __shared__ __attribute__((aligned(16))) float sz[2][TT];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int m = clamp_count(count, b, M);
    const int j0 = blockIdx.x * NT, j = j0 + tid;
    const long o = (long)b * M + j;
    if (j0 >= m) {                                                       // uniform: no query of this tile is live
        if (j < M) {
            nrm[3 * o] = 0.f; nrm[3 * o + 1] = 0.f; nrm[3 * o + 2] = 0.f;
            if (var) var[o] = 0.f;
            if (cnt) cnt[o] = 0;
        }
        return;
    }
    const float* sb = s + (long)b * s_sb;
    const bool live = j < m;
    const float qx = live ? sb[3L * j] : 0.f, qy = live ? sb[3L * j + 1] : 0.f, qz = live ? sb[3L * j + 2] : 0.f;
    const float rr = live ? r2[o] : -1.f;                                // a dead lane admits nothing
    int n = 0;
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    const int tiles = (m + TT - 1) / TT;
    float lx, ly, lz;
    auto fetch = [&](int tile) {
        const int i = tile * TT + tid;
        const bool ok = i < m;
        lx = ok ? sb[3L * i] : NAN; ly = ok ? sb[3L * i + 1] : NAN; lz = ok ? sb[3L * i + 2] : NAN;
    };
    auto stage = [&](int buf) { sx[buf][tid] = lx; sy[buf][tid] = ly; sz[buf][tid] = lz; };
    fetch(0);
    stage(0);
    __syncthreads();
    for (int tile = 0; tile < tiles; ++tile) {
        const int cur = tile & 1;
        const bool more = tile + 1 < tiles;
        if (more) fetch(tile + 1);
#pragma unroll 2
        for (int u = 0; u < TT; u += 4) {
            const f32x4 X = *reinterpret_cast<const f32x4*>(&sx[cur][u]);
            const f32x4 Y = *reinterpret_cast<const f32x4*>(&sy[cur][u]);
            const f32x4 Z = *reinterpret_cast<const f32x4*>(&sz[cur][u]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = nn_d2(qx, qy, qz, X[e], Y[e], Z[e]) <= rr;
                if (__ballot(in) != 0ull && in) {
                    const double dx = (double)(X[e] - qx), dy = (double)(Y[e] - qy), dz = (double)(Z[e] - qz);
                    n += 1;
                    s1x += dx; s1y += dy; s1z += dz;
                    sxx += dx * dx; sxy += dx * dy; sxz += dx * dz; syy += dy * dy; syz += dy * dz; szz += dz * dz;
                }
            }
        }
        if (more) stage(cur ^ 1);
        __syncthreads();
    }
    if (j >= M) return;
    // ---- the finish: fp64, per point
    const double c = (double)n;
    const double mx = s1x / c, my = s1y / c, mz = s1z / c;
    double a[3][3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    a[0][0] = sxx / c - mx * mx; a[0][1] = sxy / c - mx * my; a[0][2] = sxz / c - mx * mz;
    a[1][1] = syy / c - my * my; a[1][2] = syz / c - my * mz; a[2][2] = szz / c - mz * mz;
    a[1][0] = a[0][1]; a[2][0] = a[0][2]; a[2][1] = a[1][2];
    for (int sweep = 0; sweep < SH_CLOUD_JACOBI_SWEEPS; ++sweep) {       // fixed count: no convergence test
        jacobi_rotate<0, 1>(a, v); jacobi_rotate<0, 2>(a, v); jacobi_rotate<1, 2>(a, v);
    }
    const double e0 = a[0][0], e1 = a[1][1], e2 = a[2][2];
    const int i0 = e1 < e0 ? (e2 < e1 ? 2 : 1) : (e2 < e0 ? 2 : 0);      // the smallest: the lowest index on a tie
    const int ia = i0 == 0 ? 1 : 0, ib = i0 == 2 ? 1 : 2;                // the other two, ascending index
    const double ea = ia == 0 ? e0 : e1, eb = ib == 1 ? e1 : e2;
    const double l0 = i0 == 0 ? e0 : (i0 == 1 ? e1 : e2);
    const double l1 = eb < ea ? eb : ea, l2 = eb < ea ? ea : eb;
    double nx = i0 == 0 ? v[0][0] : (i0 == 1 ? v[0][1] : v[0][2]);
    double ny = i0 == 0 ? v[1][0] : (i0 == 1 ? v[1][1] : v[1][2]);
    double nz = i0 == 0 ? v[2][0] : (i0 == 1 ? v[2][1] : v[2][2]);
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx = nx / len; ny = ny / len; nz = nz / len;
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    const double lead = (ay > ax) ? (az > ay ? nz : ny) : (az > ax ? nz : nx);   // the largest magnitude: the lowest index on a tie
    const bool known = live && n >= 3 && l1 > SH_CLOUD_RANK_MIN * l2 && len > 0.0 && len < INFINITY;   // a NaN compares false
    float fx = (float)(lead < 0.0 ? -nx : nx), fy = (float)(lead < 0.0 ? -ny : ny), fz = (float)(lead < 0.0 ? -nz : nz);
    if (view) {                                                          // uniform
        const float* vp = view + (long)b * view_sb + (long)(live ? j : 0) * view_ps;
        const double wx = (double)vp[0] - (double)qx, wy = (double)vp[1] - (double)qy, wz = (double)vp[2] - (double)qz;
        const double dot = ((double)fx * wx + (double)fy * wy) + (double)fz * wz;
        const bool flip = dot < 0.0;                                     // exactly 0, or NaN: the canonical sign stays
        fx = flip ? -fx : fx; fy = flip ? -fy : fy; fz = flip ? -fz : fz;
    }
    const double tr = (l0 + l1) + l2;
    nrm[3 * o] = known ? fx : 0.f; nrm[3 * o + 1] = known ? fy : 0.f; nrm[3 * o + 2] = known ? fz : 0.f;
    if (var) var[o] = known ? (float)((l0 > 0.0 ? l0 : 0.0) / tr) : 0.f;
    if (cnt) cnt[o] = live ? n : 0;
}

template <int CAP, int QPT>
void launch_kth(hipStream_t st, const float* s, long s_sb, int M, const int32_t* count, int B, int k, float* r2) {
    ShProfScope ps(st, "cloud_kth_kernel|B=%d M=%d k=%d cap=%d qpt=%d", B, M, k, CAP, QPT);
    SH_LAUNCH_PS(ps, (cloud_kth_kernel<CAP, QPT>), dim3((unsigned)sh_cdiv(M, NT * QPT), (unsigned)B), dim3(NT), 0, st, s, s_sb, M, count, k, r2);
}

}  // namespace

extern "C" {

int sh_cloud_normals(const float* s, int64_t s_sb, int M, const int32_t* count, int B, int k, const float* view, int64_t view_sb,
                     int64_t view_ps, float* nrm, float* var, float* r2, int32_t* cnt, void* workspace, size_t workspace_bytes,
                     sh_stream_t stream) {
    SH_REQUIRE(k >= SH_CLOUD_K_MIN && k <= SH_CLOUD_K_MAX, SH_ERR_INVALID_ARG, "sh_cloud_normals: k = %d outside [%d, %d]", k, SH_CLOUD_K_MIN,
               SH_CLOUD_K_MAX);
    SH_REQUIRE(s && nrm, SH_ERR_INVALID_ARG, "sh_cloud_normals: null pointer");
    SH_REQUIRE(B >= 0 && M >= 0, SH_ERR_INVALID_ARG, "sh_cloud_normals: negative size (B %d, M %d)", B, M);
    if (B == 0 || M == 0) return SH_OK;
    SH_REQUIRE(s_sb >= 3L * M, SH_ERR_INVALID_ARG, "sh_cloud_normals: batch stride %ld shorter than a body", (long)s_sb);
    SH_REQUIRE(!view || ((view_ps == 0 && view_sb >= 3) || (view_ps == 3 && view_sb >= 3L * M)), SH_ERR_INVALID_ARG,
               "sh_cloud_normals: viewpoint strides (body %ld, point %ld) fit neither one viewpoint per body nor one per point", (long)view_sb,
               (long)view_ps);
    SH_REQUIRE(B <= 65535 && (long)B * M < (1L << 30), SH_ERR_UNSUPPORTED, "sh_cloud_normals: B or B*M too large");
    const size_t need = r2 ? 0 : (size_t)B * M * sizeof(float);
    SH_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), SH_ERR_WORKSPACE,
               "sh_cloud_normals: without r2 the workspace holds it (%zu bytes needed)", need);
    float* rr = r2 ? r2 : static_cast<float*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // The list's capacity is the next of 8 / 16 / 32 / 64 at or above k.  Several queries per thread share each LDS read when that
    // still leaves two workgroups per CU; otherwise one query per thread, four times the workgroups.
    const bool wide = (long)B * sh_cdiv(M, NT * 4) >= NN_WG_SLOTS / 4;
    if (k <= 8) wide ? launch_kth<8, 4>(st, s, (long)s_sb, M, count, B, k, rr) : launch_kth<8, 1>(st, s, (long)s_sb, M, count, B, k, rr);
    else if (k <= 16) wide ? launch_kth<16, 4>(st, s, (long)s_sb, M, count, B, k, rr) : launch_kth<16, 1>(st, s, (long)s_sb, M, count, B, k, rr);
    else if (k <= 32) wide ? launch_kth<32, 2>(st, s, (long)s_sb, M, count, B, k, rr) : launch_kth<32, 1>(st, s, (long)s_sb, M, count, B, k, rr);
    else launch_kth<64, 1>(st, s, (long)s_sb, M, count, B, k, rr);
    {
        ShProfScope ps(st, "cloud_normals_kernel|B=%d M=%d k=%d", B, M, k);
        SH_LAUNCH_PS(ps, cloud_normals_kernel, dim3((unsigned)sh_cdiv(M, NT), (unsigned)B), dim3(NT), 0, st, s, (long)s_sb, M, count, rr, view,
                     (long)view_sb, (long)view_ps, nrm, var, cnt);
    }
    SH_CHECK_LAUNCH("cloud_normals");
    return SH_OK;
}

}  // extern "C"
