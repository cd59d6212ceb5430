// Body measurements on device: closed-polyline girths and bone lengths, batched over meshes
// (reference utils_SH.py:86-98 cal_length, :144-161 measure_body_quick).  Tiny, latency-bound
// work: one wavefront per (mesh, ring), one thread per (mesh, bone).
// Their gradients are gather kernels over host-built transposed lists (measure.py: GirthRings, Bones): one thread per
// (mesh, vertex) or (mesh, joint) sums its terms in list order - no atomics, the same bits on every call.
#include "sh_common.h"

namespace {

__device__ __forceinline__ void ring_point(const float* __restrict__ v, const int32_t* __restrict__ ra,
                                           const int32_t* __restrict__ rb, const float* __restrict__ rf, int i, float* q) {
    const float f = rf[i];
    const float* a = v + 3L * ra[i];
    const float* b = v + 3L * rb[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) q[d] = a[d] * (1.f - f) + b[d] * f;          // utils_SH.py:155
}

// grid = B * P wavefronts (4 per block)
__global__ void girth_kernel(const float* __restrict__ v, long v_sb, const int32_t* __restrict__ ring_ptr,
                             const int32_t* __restrict__ ra, const int32_t* __restrict__ rb, const float* __restrict__ rf,
                             int B, int P, float* __restrict__ girth) {
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (wave >= B * P) return;
    const int b = wave / P, p = wave - b * P;
    const int beg = ring_ptr[p], n = ring_ptr[p + 1] - beg;
    const float* vb = v + (long)b * v_sb;
    float s = 0.f;
    // segment i joins point i and point (i+1) mod n; for n == 1 both are the same point (length 0),
    // for n == 2 the closing segment is counted as well, exactly like utils_SH.py:156-158
    for (int i = lane; i < n; i += 64) {
        const int j = (i + 1 == n) ? 0 : i + 1;
        float q0[3], q1[3];
        ring_point(vb, ra, rb, rf, beg + i, q0);
        ring_point(vb, ra, rb, rf, beg + j, q1);
        const float dx = q0[0] - q1[0], dy = q0[1] - q1[1], dz = q0[2] - q1[2];
        s += sqrtf(dx * dx + dy * dy + dz * dz);
    }
    s = sh_wave_sum(s);
    if (lane == 0) girth[wave] = s;
}

__global__ void bone_length_kernel(const float* __restrict__ kps, const int32_t* __restrict__ bones, int B, int K, int P,
                                   float* __restrict__ length) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * P) return;
    const int b = i / P, p = i - b * P;
    const float* k = kps + (long)b * K * 3;
    const int i0 = bones[3 * p], i1 = bones[3 * p + 1], i2 = bones[3 * p + 2];
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float tail = i2 >= 0 ? (k[3 * i1 + d] + k[3 * i2 + d]) / 2.f : k[3 * i1 + d];
        const float e = k[3 * i0 + d] - tail;
        s += e * e;
    }
    length[i] = sqrtf(s);
}

// The gradients form ring points and segment vectors in fp64: a segment is short next to the coordinates of its ends, and in fp32
// the cancellation in q0 - q1 costs ~|q| / |d| x 2^-24 of its direction (1e-5 relative on the golden rings).  Tiny work; the
// inputs and outputs stay fp32.
__device__ __forceinline__ void ring_point_d(const float* __restrict__ v, const int32_t* __restrict__ ra,
                                             const int32_t* __restrict__ rb, const float* __restrict__ rf, int i, double* q) {
    const double f = rf[i];
    const float* a = v + 3L * ra[i];
    const float* b = v + 3L * rb[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) q[d] = (double)a[d] * (1.0 - f) + (double)b[d] * f;
}
// unit vector of segment q0 -> q1 as the forward measures it (d = q0 - q1); a zero-length segment gives 0 (its subgradient)
__device__ __forceinline__ void seg_unit(const double* q0, const double* q1, double* u) {
    const double dx = q0[0] - q1[0], dy = q0[1] - q1[1], dz = q0[2] - q1[2];
    const double L = sqrt(dx * dx + dy * dy + dz * dz);
    const double r = L > 0.0 ? 1.0 / L : 0.0;
    u[0] = dx * r; u[1] = dy * r; u[2] = dz * r;
}

// g_v[b][r][:] = sum over the entries (ring point k, weight w) of row r of  w * g_girth[b][ring(k)] * (u(k -> k+1) - u(k-1 -> k)),
// segment k joining ring point k to point (k+1) mod n exactly as girth_kernel does (n == 1: the one segment has length 0; n == 2:
// both segments join the same two points).  Rows >= n_vt (and rows with no entry) get 0.  grid: one thread per (mesh, row).
__global__ void girth_bwd_kernel(const float* __restrict__ v, long v_sb, const int32_t* __restrict__ ring_ptr,
                                 const int32_t* __restrict__ ra, const int32_t* __restrict__ rb, const float* __restrict__ rf,
                                 const int32_t* __restrict__ pt_ring, const int32_t* __restrict__ vt_ptr,
                                 const int32_t* __restrict__ vt_pt, const float* __restrict__ vt_w, int n_vt,
                                 const float* __restrict__ g_girth, int B, int P, int rows, float* __restrict__ g_v) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)B * rows) return;
    const int b = (int)(t / rows), r = (int)(t - (long)b * rows);
    const float* vb = v + (long)b * v_sb;
    double acc[3] = {0.0, 0.0, 0.0};
    if (r < n_vt) {
        for (int e = vt_ptr[r]; e < vt_ptr[r + 1]; ++e) {
            const int k = vt_pt[e], p = pt_ring[k];
            const int beg = ring_ptr[p], n = ring_ptr[p + 1] - beg, i = k - beg;
            const int nx = (i + 1 == n) ? 0 : i + 1, pv = (i == 0) ? n - 1 : i - 1;
            double q[3], qn[3], qp[3], u0[3], u1[3];
            ring_point_d(vb, ra, rb, rf, k, q);
            ring_point_d(vb, ra, rb, rf, beg + nx, qn);
            ring_point_d(vb, ra, rb, rf, beg + pv, qp);
            seg_unit(q, qn, u0);                                  // segment i: d/dq_i |q_i - q_next| = +u
            seg_unit(qp, q, u1);                                  // segment i - 1: d/dq_i |q_prev - q_i| = -u
            const double gw = (double)g_girth[(long)b * P + p] * (double)vt_w[e];
#pragma unroll
            for (int d = 0; d < 3; ++d) acc[d] += gw * (u0[d] - u1[d]);
        }
    }
    float* o = g_v + t * 3;
    o[0] = (float)acc[0]; o[1] = (float)acc[1]; o[2] = (float)acc[2];
}

// g_kps[b][j][:] = sum over the entries (bone p, weight w) of joint j of  w * g_len[b][p] * u_p,  u_p the unit vector of bone p as
// bone_length_kernel measures it (w = +1 for the head, -1 for a 2-joint bone's tail, -1/2 for each joint of a 3-joint bone's tail).
// Joints >= n_jt get 0.  grid: one thread per (mesh, joint).
__global__ void bone_length_bwd_kernel(const float* __restrict__ kps, const int32_t* __restrict__ bones,
                                       const int32_t* __restrict__ jt_ptr, const int32_t* __restrict__ jt_bone,
                                       const float* __restrict__ jt_w, int n_jt, const float* __restrict__ g_len, int B, int K,
                                       int P, float* __restrict__ g_kps) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * K) return;
    const int b = t / K, j = t - b * K;
    const float* k = kps + (long)b * K * 3;
    double acc[3] = {0.0, 0.0, 0.0};
    if (j < n_jt) {
        for (int e = jt_ptr[j]; e < jt_ptr[j + 1]; ++e) {                // (fp64 bone vectors, as the girth gradient's segments)
            const int p = jt_bone[e];
            const int i0 = bones[3 * p], i1 = bones[3 * p + 1], i2 = bones[3 * p + 2];
            double ed[3], s = 0.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double tail = i2 >= 0 ? ((double)k[3 * i1 + d] + (double)k[3 * i2 + d]) / 2.0 : (double)k[3 * i1 + d];
                ed[d] = (double)k[3 * i0 + d] - tail;
                s += ed[d] * ed[d];
            }
            const double L = sqrt(s);
            const double gw = L > 0.0 ? (double)g_len[(long)b * P + p] * (double)jt_w[e] / L : 0.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) acc[d] += gw * ed[d];
        }
    }
    float* o = g_kps + (long)t * 3;
    o[0] = (float)acc[0]; o[1] = (float)acc[1]; o[2] = (float)acc[2];
}

// g_x[b][r][:] = sum_{j < K} J[j][r] g_kps[b][j][:] for r < N, 0 for N <= r < rows.  One thread per (mesh, row); J read a
// column at a time (coalesced across the threads of a block), joints summed in order.
__global__ void joint_regress_bwd_kernel(const float* __restrict__ g_kps, const float* __restrict__ J, int B, int N, int K, int rows,
                                         float* __restrict__ g_x) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)B * rows) return;
    const int b = (int)(t / rows), r = (int)(t - (long)b * rows);
    float acc[3] = {0.f, 0.f, 0.f};
    if (r < N) {
        const float* gk = g_kps + (long)b * K * 3;
        for (int j = 0; j < K; ++j) {
            const float w = J[(long)j * N + r];
            acc[0] += w * gk[3 * j]; acc[1] += w * gk[3 * j + 1]; acc[2] += w * gk[3 * j + 2];
        }
    }
    float* o = g_x + t * 3;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
}

}  // namespace

extern "C" {

int sh_measure_girth(const float* v, int64_t v_sb, const int32_t* ring_ptr, const int32_t* ring_a, const int32_t* ring_b,
                     const float* ring_f, int B, int P, float* girth, sh_stream_t stream) {
    SH_REQUIRE(v && ring_ptr && ring_a && ring_b && ring_f && girth, SH_ERR_INVALID_ARG, "sh_measure_girth: null pointer");
    SH_REQUIRE(B > 0 && P > 0 && v_sb > 0, SH_ERR_INVALID_ARG, "sh_measure_girth: non-positive size");
    SH_REQUIRE((long)B * P < (1L << 30), SH_ERR_UNSUPPORTED, "sh_measure_girth: B*P too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "girth_kernel|B=%d P=%d", B, P);
    hipLaunchKernelGGL(girth_kernel, dim3(sh_cdiv(B * P, 4)), dim3(256), 0, st, v, (long)v_sb, ring_ptr, ring_a, ring_b, ring_f,
                       B, P, girth);
    SH_CHECK_LAUNCH("measure_girth");
    return SH_OK;
}

int sh_bone_length(const float* kps, const int32_t* bones, int B, int K, int P, float* length, sh_stream_t stream) {
    SH_REQUIRE(kps && bones && length, SH_ERR_INVALID_ARG, "sh_bone_length: null pointer");
    SH_REQUIRE(B > 0 && K > 0 && P > 0, SH_ERR_INVALID_ARG, "sh_bone_length: non-positive size");
    SH_REQUIRE((long)B * P < (1L << 30), SH_ERR_UNSUPPORTED, "sh_bone_length: B*P too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "bone_length_kernel|B=%d P=%d", B, P);
    hipLaunchKernelGGL(bone_length_kernel, dim3(sh_cdiv(B * P, 256)), dim3(256), 0, st, kps, bones, B, K, P, length);
    SH_CHECK_LAUNCH("bone_length");
    return SH_OK;
}

int sh_measure_girth_bwd(const float* v, int64_t v_sb, const int32_t* ring_ptr, const int32_t* ring_a, const int32_t* ring_b,
                         const float* ring_f, const int32_t* pt_ring, const int32_t* vt_ptr, const int32_t* vt_pt, const float* vt_w,
                         int n_vt, const float* g_girth, int B, int P, int rows, float* g_v, sh_stream_t stream) {
    SH_REQUIRE(v && ring_ptr && ring_a && ring_b && ring_f && pt_ring && vt_ptr && vt_pt && vt_w && g_girth && g_v, SH_ERR_INVALID_ARG,
               "sh_measure_girth_bwd: null pointer");
    SH_REQUIRE(B > 0 && P > 0 && rows > 0 && v_sb >= 3L * rows && n_vt >= 0 && n_vt <= rows, SH_ERR_INVALID_ARG,
               "sh_measure_girth_bwd: bad size (B %d, P %d, rows %d, v_sb %ld, table rows %d)", B, P, rows, (long)v_sb, n_vt);
    SH_REQUIRE((long)B * rows < (1L << 30), SH_ERR_UNSUPPORTED, "sh_measure_girth_bwd: B*rows too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "girth_bwd_kernel|B=%d P=%d rows=%d", B, P, rows);
    SH_LAUNCH_PS(ps, girth_bwd_kernel, dim3(sh_cdiv(B * rows, 256)), dim3(256), 0, st, v, (long)v_sb, ring_ptr, ring_a, ring_b, ring_f,
                 pt_ring, vt_ptr, vt_pt, vt_w, n_vt, g_girth, B, P, rows, g_v);
    SH_CHECK_LAUNCH("measure_girth_bwd");
    return SH_OK;
}

int sh_bone_length_bwd(const float* kps, const int32_t* bones, const int32_t* jt_ptr, const int32_t* jt_bone, const float* jt_w,
                       int n_jt, const float* g_len, int B, int K, int P, float* g_kps, sh_stream_t stream) {
    SH_REQUIRE(kps && bones && jt_ptr && jt_bone && jt_w && g_len && g_kps, SH_ERR_INVALID_ARG, "sh_bone_length_bwd: null pointer");
    SH_REQUIRE(B > 0 && K > 0 && P > 0 && n_jt >= 0 && n_jt <= K, SH_ERR_INVALID_ARG,
               "sh_bone_length_bwd: bad size (B %d, K %d, P %d, table joints %d)", B, K, P, n_jt);
    SH_REQUIRE((long)B * K < (1L << 30), SH_ERR_UNSUPPORTED, "sh_bone_length_bwd: B*K too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "bone_length_bwd_kernel|B=%d P=%d", B, P);
    SH_LAUNCH_PS(ps, bone_length_bwd_kernel, dim3(sh_cdiv(B * K, 256)), dim3(256), 0, st, kps, bones, jt_ptr, jt_bone, jt_w, n_jt, g_len,
                 B, K, P, g_kps);
    SH_CHECK_LAUNCH("bone_length_bwd");
    return SH_OK;
}

int sh_joint_regress_bwd(const float* g_kps, const float* J, int B, int N, int K, int rows, float* g_x, sh_stream_t stream) {
    SH_REQUIRE(g_kps && J && g_x, SH_ERR_INVALID_ARG, "sh_joint_regress_bwd: null pointer");
    SH_REQUIRE(B > 0 && N > 0 && K > 0 && rows >= N, SH_ERR_INVALID_ARG, "sh_joint_regress_bwd: bad size (B %d, N %d, K %d, rows %d)",
               B, N, K, rows);
    SH_REQUIRE((long)B * rows < (1L << 30), SH_ERR_UNSUPPORTED, "sh_joint_regress_bwd: B*rows too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "joint_regress_bwd_kernel|B=%d N=%d K=%d", B, N, K);
    SH_LAUNCH_PS(ps, joint_regress_bwd_kernel, dim3(sh_cdiv(B * rows, 256)), dim3(256), 0, st, g_kps, J, B, N, K, rows, g_x);
    SH_CHECK_LAUNCH("joint_regress_bwd");
    return SH_OK;
}

}  // extern "C"
