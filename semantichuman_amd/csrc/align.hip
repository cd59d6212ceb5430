// Aligning scans to the model: the weighted moments of the matched pairs, the closed-form similarity from them, and the
// transform of the scan (include/sh_kernels.h, "Scan alignment").  The matches are the ones scan.hip's search has recorded for
// the Chamfer loss, so a pose update costs no search.  No atomics of any kind: every sum runs in a fixed order that depends on
// M and n only - the same bits on every call, for every batch size and for a body alone or inside a batch.
#include "sh_nn.h"

namespace {

constexpr int NT = 256;                       // threads per workgroup of the moments kernel
constexpr int RANGE = SH_ALIGN_RANGE;         // pairs per workgroup: thread t takes t, t + 256, ... of its range (8 each)
constexpr int NP = SH_ALIGN_PARTIAL;          // sums per range
constexpr int NM = SH_ALIGN_MOMENTS;          // doubles per body of the finished moments
constexpr int NPP = SH_ALIGN_PLANE_PARTIAL;   // sums per range of the point-to-plane step
constexpr int NPS = SH_ALIGN_PLANE_SYSTEM;    // doubles per body of its joined system

int ranges_of(int rows) { return (rows + RANGE - 1) / RANGE; }

// The scan -> model partner of the surface form: which table the recorded face indexes, and the foot point's weights.  Empty
// (all null) for the vertex form, which never reads it.
struct AlignSurface {
    const int32_t* faces;   // [nF][3]
    int nF;
    const float* uv;        // [B][M][2]
};

// One coordinate of the foot point, the header's expression: fp32 differences from corner a, then fp64 with no contraction.
__device__ __forceinline__ double foot_coord(float a, float b, float c, float v, float w) {
#pragma clang fp contract(off)
    const float ab = b - a, ac = c - a;
    return (double)a + ((double)v * (double)ab + (double)w * (double)ac);
}

// The unit normal of the face (a, b, c), the header's expression: the fp32 cross product of "Vertex normals", normalised in fp64;
// the zero vector when its length is zero or not finite.
__device__ __forceinline__ void face_normal(const float* a, const float* b, const float* c, double& n0, double& n1, double& n2) {
#pragma clang fp contract(off)
    float fx, fy, fz;
    face_cross(a, b, c, fx, fy, fz);
    const double cx = fx, cy = fy, cz = fz;
    const double len = sqrt((cx * cx + cy * cy) + cz * cz);
    const bool ok = len > 0.0 && len < __builtin_inf();
    const double d = ok ? len : 1.0;
    n0 = ok ? cx / d : 0.0; n1 = ok ? cy / d : 0.0; n2 = ok ? cz / d : 0.0;
}

// What a kept pair adds to the sums of its range, in the two forms the walk below is instantiated with.  p: the scan point (fp32
// [3]), q: its partner.  N: sums per range, N_ACT: the slot that counts the active vertices of a model -> scan range, NORMALS:
// whether add() takes the model's normal at the partner as well.  SCOPE: the profile labels of the vertex and the surface form.

// The closed form's sums (header, "Scan alignment").  The compiler's default contraction, as ever.
struct PointSums {
    static constexpr int N = NP, N_ACT = 18;
    static constexpr bool NORMALS = false;
    static constexpr const char* SCOPE = "align_moments_kernel|B=%d M=%d n=%d ranges=%d";
    static constexpr const char* SCOPE_SURFACE = "align_moments_surface_kernel|B=%d M=%d n=%d nF=%d ranges=%d";
    static constexpr const char* SCOPE_ROBUST = "align_moments_robust_kernel|B=%d M=%d n=%d ranges=%d robust=%d";
    static constexpr const char* SCOPE_SURFACE_ROBUST = "align_moments_surface_robust_kernel|B=%d M=%d n=%d nF=%d ranges=%d robust=%d";
    double a[N];
    __device__ __forceinline__ void add(const float* p, double q0, double q1, double q2) {
        const double p0 = p[0], p1 = p[1], p2 = p[2];
        a[0] += 1.0;
        a[1] += p0; a[2] += p1; a[3] += p2;
        a[4] += q0; a[5] += q1; a[6] += q2;
        a[7] += q0 * p0; a[8] += q0 * p1; a[9] += q0 * p2;
        a[10] += q1 * p0; a[11] += q1 * p1; a[12] += q1 * p2;
        a[13] += q2 * p0; a[14] += q2 * p1; a[15] += q2 * p2;
        a[16] += p0 * p0 + p1 * p1 + p2 * p2;
        a[17] += q0 * q0 + q1 * q1 + q2 * q2;
    }
};

// The sums of the header's "Point-to-plane step": per kept pair the Jacobian row J (7) of the residual r along the partner's
// normal, J J^T (upper triangle), J r and r^2.  fp64, contraction off.
struct PlaneSums {
    static constexpr int N = NPP, N_ACT = 37;
    static constexpr bool NORMALS = true;
    static constexpr const char* SCOPE = "align_plane_moments_kernel|B=%d M=%d n=%d ranges=%d";
    static constexpr const char* SCOPE_SURFACE = "align_plane_moments_surface_kernel|B=%d M=%d n=%d nF=%d ranges=%d";
    static constexpr const char* SCOPE_ROBUST = "align_plane_moments_robust_kernel|B=%d M=%d n=%d ranges=%d robust=%d";
    static constexpr const char* SCOPE_SURFACE_ROBUST = "align_plane_moments_surface_robust_kernel|B=%d M=%d n=%d nF=%d ranges=%d robust=%d";
    double a[N];
    __device__ __forceinline__ void add(const float* p, double q0, double q1, double q2, double n0, double n1, double n2) {
#pragma clang fp contract(off)
        const double p0 = p[0], p1 = p[1], p2 = p[2];
        const double res = (n0 * (p0 - q0) + n1 * (p1 - q1)) + n2 * (p2 - q2);
        const double J[7] = {n0, n1, n2, p1 * n2 - p2 * n1, p2 * n0 - p0 * n2, p0 * n1 - p1 * n0, (n0 * p0 + n1 * p1) + n2 * p2};
        a[0] += 1.0;
        int c = 1;
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int j = i; j < 7; ++j) a[c++] += J[i] * J[j];
#pragma unroll
        for (int i = 0; i < 7; ++i) a[29 + i] += J[i] * res;
        a[36] += res * res;
    }
};

// Stage 1 of both pose steps: the one walk over the matched pairs.  grid (range, body).  Ranges [0, r_sm) walk the scan -> model
// pairs j, ranges [r_sm, r_sm + r_ms) the model -> scan pairs i.  The sums are unweighted (the weight of a direction is one factor
// per body, applied by the solve kernel); a range beyond the body's count stores zeros, which change nothing when the second stage
// adds them.  SURFACE: idx_sm / d2_sm are the recorded face and the surface distance, and the partner of s_j is the foot point on
// that face instead of a vertex - with the face's normal, formed from the three corners the foot point needs anyway, where Sums
// takes one; nothing else differs.  A vertex partner's normal is its row of tn, which no other form reads.
// ROBUST (header, "Robust terms"): a kept pair adds w times what it adds otherwise, w = the fp32 weight of its recorded d2 widened
// to fp64 - its terms are formed by the same Sums::add into a zeroed set and each multiplied by w once.  The active-vertex slot
// stays a count.  SH_ROBUST_NONE adds straight into the range's sums, as ever.
template <class Sums, bool SURFACE, int ROBUST>
__global__ __launch_bounds__(NT) void align_pairs_kernel(const float* __restrict__ s, long s_sb, int M, const int32_t* __restrict__ s_count,
                                                         const float* __restrict__ x, long x_sb, int rows, int n,
                                                         const unsigned char* __restrict__ v_mask, long mask_sb, const float* __restrict__ tn,
                                                         const int32_t* __restrict__ idx_sm, const float* __restrict__ d2_sm,
                                                         const int32_t* __restrict__ idx_ms, const float* __restrict__ d2_ms, float tau2,
                                                         float scale2, int r_sm, AlignSurface sf, double* __restrict__ partials) {
    constexpr int N = Sums::N;
    __shared__ double red[N][4];
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int R = gridDim.x;
    const int m = clamp_count(s_count, b, M);
    const float* sb = s + (long)b * s_sb;
    const float* xb = x + (long)b * x_sb;
    const float* tb = Sums::NORMALS && tn ? tn + (long)b * n * 3 : nullptr;
    Sums acc;
#pragma unroll
    for (int c = 0; c < N; ++c) acc.a[c] = 0.0;
    auto add_pair = [&](float d2, auto... pair) {                        // a kept pair with the recorded distance d2
        if constexpr (ROBUST != 0) {
            const double w = robust_weight<ROBUST>(d2, scale2);
            Sums one;
#pragma unroll
            for (int c = 0; c < N; ++c) one.a[c] = 0.0;
            one.add(pair...);
#pragma unroll
            for (int c = 0; c < N; ++c) acc.a[c] += w * one.a[c];
        } else {
            acc.add(pair...);
        }
    };
    auto add_vertex = [&](float d2, long ip, int i) {                    // the partner of scan point ip is vertex i
        const float* q = xb + 3L * i;
        if constexpr (Sums::NORMALS) add_pair(d2, sb + 3 * ip, (double)q[0], (double)q[1], (double)q[2], (double)tb[3L * i], (double)tb[3L * i + 1],
                                              (double)tb[3L * i + 2]);
        else add_pair(d2, sb + 3 * ip, (double)q[0], (double)q[1], (double)q[2]);
    };
    if (r < r_sm) {                                                      // uniform over the workgroup
        const int lo = r * RANGE, hi = min(lo + RANGE, m);
        for (int j = lo + tid; j < hi; j += NT) {
            const int i = idx_sm[(long)b * M + j];
            const float d2 = d2_sm[(long)b * M + j];
            if (!(d2 < tau2)) continue;
            if constexpr (SURFACE) {
                if ((unsigned)i >= (unsigned)sf.nF) continue;
                int i0, i1, i2;
                if (!face_corners(sf.faces, i, n, i0, i1, i2)) continue;
                const float v = sf.uv[2 * ((long)b * M + j)], w = sf.uv[2 * ((long)b * M + j) + 1];
                const float *ca = xb + 3L * i0, *cb = xb + 3L * i1, *cc = xb + 3L * i2;
                double n0, n1, n2;                                       // the face's, only where Sums takes a normal
                if constexpr (Sums::NORMALS) face_normal(ca, cb, cc, n0, n1, n2);
                const double q0 = foot_coord(ca[0], cb[0], cc[0], v, w), q1 = foot_coord(ca[1], cb[1], cc[1], v, w),
                             q2 = foot_coord(ca[2], cb[2], cc[2], v, w);
                if constexpr (Sums::NORMALS) add_pair(d2, sb + 3L * j, q0, q1, q2, n0, n1, n2);
                else add_pair(d2, sb + 3L * j, q0, q1, q2);
            } else {
                if (i >= 0 && i < n) add_vertex(d2, j, i);
            }
        }
    } else {
        const unsigned char* mb = v_mask ? v_mask + (long)b * mask_sb : nullptr;
        const int lo = (r - r_sm) * RANGE, hi = min(lo + RANGE, n);
        for (int i = lo + tid; i < hi; i += NT) {
            if (mb && mb[i] == 0) continue;
            acc.a[Sums::N_ACT] += 1.0;                                   // n_act
            const int k = idx_ms[(long)b * rows + i];
            if (k < 0 || k >= m) continue;
            const float d2 = d2_ms[(long)b * rows + i];
            if (d2 < tau2) add_vertex(d2, k, i);
        }
    }
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const double v = wave_sum_d(acc.a[c]);
        if ((tid & 63) == 0) red[c][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < N) partials[((long)b * R + r) * N + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// The pose so far composed with the increment (c R, t): A_new = c R A_old, t_new = c R t_old + t, scale_new = c scale_old, each
// rounded to fp32 once.  Everything is read before anything is written, so the outputs may alias the inputs.  Both solve kernels
// end here.
__device__ __forceinline__ void compose_pose(double c, const double (&Rm)[3][3], const double (&t)[3], const float* pi, double s0, float* po,
                                             float* so) {
    double A0[3][3], t0[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) A0[i][j] = pi[3 * i + j];
        t0[i] = pi[9 + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) po[3 * i + j] = (float)(c * (Rm[i][0] * A0[0][j] + Rm[i][1] * A0[1][j] + Rm[i][2] * A0[2][j]));
        po[9 + i] = (float)(c * (Rm[i][0] * t0[0] + Rm[i][1] * t0[1] + Rm[i][2] * t0[2]) + t[i]);
    }
    *so = (float)(c * s0);
}

// How both solve kernels open, one wave per body: lane c < Sums::N adds the ranges' partial sums of component c in range order,
// the scan -> model ranges into sum[0][c] and the model -> scan ranges into sum[1][c]; w1 and w2 are the weights the two
// directions are then joined with.
template <class Sums>
__device__ __forceinline__ void sum_ranges(const double* __restrict__ partials, int b, int lane, int r_sm, int r_ms, int M,
                                           const int32_t* __restrict__ s_count, float w_ms, double (&sum)[2][Sums::N], double& w1, double& w2) {
    constexpr int N = Sums::N;
    const int R = r_sm + r_ms;
    if (lane < N) {
        double u = 0.0, w = 0.0;
        for (int r = 0; r < r_sm; ++r) u += partials[((long)b * R + r) * N + lane];
        for (int r = r_sm; r < R; ++r) w += partials[((long)b * R + r) * N + lane];
        sum[0][lane] = u; sum[1][lane] = w;
    }
    __syncthreads();
    const int m = clamp_count(s_count, b, M);
    const double n_act = sum[1][Sums::N_ACT];
    w1 = m > 0 ? 1.0 / (double)m : 0.0;
    w2 = (m > 0 && r_ms > 0 && n_act > 0.0) ? (double)w_ms / n_act : 0.0;
}

// The closed form's stage 2, one wave per body: the ranges' sums (sum_ranges), the two directions joined with their weights - the
// kept count exact, in a slot of its own -, and lane 0 then solves for the pose.
__global__ __launch_bounds__(64) void align_solve_kernel(const double* __restrict__ partials, int M, int n, const int32_t* __restrict__ s_count,
                                                        float w_ms, int r_sm, int r_ms, int mode, const float* __restrict__ pose_in,
                                                        const float* __restrict__ scale_in, float* __restrict__ pose_out,
                                                        float* __restrict__ scale_out, float* __restrict__ inc, double* __restrict__ mom) {
    __shared__ double sum[2][NP];
    __shared__ double mo[NM];
    const int b = blockIdx.x, lane = threadIdx.x;
    double w1, w2;
    sum_ranges<PointSums>(partials, b, lane, r_sm, r_ms, M, s_count, w_ms, sum, w1, w2);
    if (lane < 18) mo[lane] = w1 * sum[0][lane] + w2 * sum[1][lane];
    if (lane == 18) mo[18] = (w1 > 0.0 ? sum[0][0] : 0.0) + (w2 > 0.0 ? sum[1][0] : 0.0);       // kept pairs, exact
    if (lane == 19) mo[19] = 0.0;
    __syncthreads();
    if (mom && lane < NM) mom[(long)b * NM + lane] = mo[lane];
    if (lane != 0 || !pose_out) return;

    const double W = mo[0];
    double Rm[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double c = 1.0, t[3] = {0.0, 0.0, 0.0};
    if (W > 0.0) {
        const double iw = 1.0 / W;
        double pb[3], qb[3], H[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { pb[k] = mo[1 + k] * iw; qb[k] = mo[4 + k] * iw; }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) H[i][j] = mo[7 + 3 * i + j] * iw - qb[i] * pb[j];      // H[i][j] = cov(q_i, p_j)
        if (mode != SH_ALIGN_TRANSLATION) {
            // Horn's matrix: with S_ab = sum p_a q_b = H[b][a], its largest eigenvector is the quaternion (w, x, y, z) of the
            // rotation that maximises trace(R^T H).  Scaled to unit size first: the eigenvectors do not change.
            const double Sxx = H[0][0], Sxy = H[1][0], Sxz = H[2][0], Syx = H[0][1], Syy = H[1][1], Syz = H[2][1], Szx = H[0][2],
                         Szy = H[1][2], Szz = H[2][2];
            double a[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                              {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                              {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                              {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
            double big = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) big = fmax(big, fabs(a[i][j]));
            const double inv = big > 0.0 ? 1.0 / big : 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) a[i][j] *= inv;
            double v[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
            for (int sweep = 0; sweep < SH_ALIGN_JACOBI_SWEEPS; ++sweep) {       // fixed count: no convergence test
                jacobi_rotate<0, 1>(a, v); jacobi_rotate<0, 2>(a, v); jacobi_rotate<0, 3>(a, v);
                jacobi_rotate<1, 2>(a, v); jacobi_rotate<1, 3>(a, v); jacobi_rotate<2, 3>(a, v);
            }
            double best = a[0][0], q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];   // lowest index on a tie
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const bool up = a[k][k] > best;
                best = up ? a[k][k] : best;
                q0 = up ? v[0][k] : q0; q1 = up ? v[1][k] : q1; q2 = up ? v[2][k] : q2; q3 = up ? v[3][k] : q3;
            }
            const double qn = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
            q0 *= qn; q1 *= qn; q2 *= qn; q3 *= qn;
            Rm[0][0] = 1.0 - 2.0 * (q2 * q2 + q3 * q3); Rm[0][1] = 2.0 * (q1 * q2 - q0 * q3); Rm[0][2] = 2.0 * (q1 * q3 + q0 * q2);
            Rm[1][0] = 2.0 * (q1 * q2 + q0 * q3); Rm[1][1] = 1.0 - 2.0 * (q1 * q1 + q3 * q3); Rm[1][2] = 2.0 * (q2 * q3 - q0 * q1);
            Rm[2][0] = 2.0 * (q1 * q3 - q0 * q2); Rm[2][1] = 2.0 * (q2 * q3 + q0 * q1); Rm[2][2] = 1.0 - 2.0 * (q1 * q1 + q2 * q2);
        }
        if (mode == SH_ALIGN_SIMILARITY) {
            const double var_p = mo[16] * iw - (pb[0] * pb[0] + pb[1] * pb[1] + pb[2] * pb[2]);
            double num = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) num += Rm[i][j] * H[i][j];
            c = (var_p > 0.0 && num > 0.0) ? num / var_p : 1.0;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = qb[i] - c * (Rm[i][0] * pb[0] + Rm[i][1] * pb[1] + Rm[i][2] * pb[2]);
    }
    if (inc) {
        float* o = inc + (long)b * 13;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) o[3 * i + j] = (float)(c * Rm[i][j]);
            o[9 + i] = (float)t[i];
        }
        o[12] = (float)c;
    }
    compose_pose(c, Rm, t, pose_in + (long)b * 12, scale_in[b], pose_out + (long)b * 12, scale_out + b);
}

// The point-to-plane step's stage 2, one wave per body: the ranges' sums (sum_ranges), the two directions joined with their
// weights, and lane 0 solves the leading k x k block of
// H delta = -g (diagonal scaling, Cholesky; fixed loop counts, selects instead of branches: the rows and columns >= k are those of
// the identity, so every mode runs the same 7 x 7 code), turns delta into (c R, t) and composes it with the pose so far.
__global__ __launch_bounds__(64) void align_plane_solve_kernel(const double* __restrict__ partials, int M, int n, const int32_t* __restrict__ s_count,
                                                              float w_ms, int r_sm, int r_ms, int k, const float* __restrict__ pose_in,
                                                              const float* __restrict__ scale_in, float* __restrict__ pose_out,
                                                              float* __restrict__ scale_out, double* __restrict__ sys,
                                                              int32_t* __restrict__ solved) {
#pragma clang fp contract(off)
    __shared__ double sum[2][NPP];
    __shared__ double sy[NPS];
    const int b = blockIdx.x, lane = threadIdx.x;
    double w1, w2;
    sum_ranges<PlaneSums>(partials, b, lane, r_sm, r_ms, M, s_count, w_ms, sum, w1, w2);
    if (lane < NPS) sy[lane] = w1 * sum[0][lane] + w2 * sum[1][lane];
    __syncthreads();
    if (sys && lane < NPS) sys[(long)b * NPS + lane] = sy[lane];
    if (lane != 0 || !pose_out) return;

    bool ok = sy[0] > 0.0;
    double H[7][7], sd[7], gs[7];
    {
        int c = 1;
#pragma unroll
        for (int i = 0; i < 7; ++i)
#pragma unroll
            for (int j = i; j < 7; ++j) { H[i][j] = sy[c]; H[j][i] = sy[c]; ++c; }
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const double d = H[i][i];
        const bool good = d > 0.0 && d < __builtin_inf();
        ok = ok && (i >= k || good);
        sd[i] = (i < k && good) ? sqrt(d) : 1.0;
        gs[i] = i < k ? sy[29 + i] / sd[i] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int j = 0; j < 7; ++j) H[i][j] = (i < k && j < k) ? H[i][j] / (sd[i] * sd[j]) : (i == j ? 1.0 : 0.0);
    double L[7][7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < j; ++c) acc += L[j][c] * L[j][c];
        const double piv = H[j][j] - acc;
        const bool pos = piv > SH_ALIGN_PLANE_PIVOT_MIN;                 // false for NaN
        ok = ok && pos;
        L[j][j] = sqrt(pos ? piv : 1.0);
#pragma unroll
        for (int i = j + 1; i < 7; ++i) {
            double dot = 0.0;
#pragma unroll
            for (int c = 0; c < j; ++c) dot += L[i][c] * L[j][c];
            L[i][j] = (H[i][j] - dot) / L[j][j];
        }
    }
    double y[7], z[7], delta[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double dot = 0.0;
#pragma unroll
        for (int c = 0; c < i; ++c) dot += L[i][c] * y[c];
        y[i] = (-gs[i] - dot) / L[i][i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        double dot = 0.0;
#pragma unroll
        for (int c = i + 1; c < 7; ++c) dot += L[c][i] * z[c];
        z[i] = (y[i] - dot) / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        delta[i] = z[i] / sd[i];
        ok = ok && fabs(delta[i]) < __builtin_inf();                     // false for NaN
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) delta[i] = (ok && i < k) ? delta[i] : 0.0;
    const double c = exp(delta[6]);
    const double o0 = delta[3], o1 = delta[4], o2 = delta[5];
    const double th2 = (o0 * o0 + o1 * o1) + o2 * o2;
    const bool tiny = th2 < 1e-8;
    const double th = sqrt(tiny ? 1.0 : th2);
    const double fa = tiny ? 1.0 - th2 / 6.0 : sin(th) / th;
    const double fb = tiny ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / (tiny ? 1.0 : th2);
    const double K[3][3] = {{0.0, -o2, o1}, {o2, 0.0, -o0}, {-o1, o0, 0.0}};
    double Rm[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double k2 = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
            Rm[i][j] = (i == j ? 1.0 : 0.0) + (fa * K[i][j] + fb * k2);
        }
    const double t[3] = {delta[0], delta[1], delta[2]};
    solved[b] = ok ? 1 : 0;
    compose_pose(c, Rm, t, pose_in + (long)b * 12, scale_in[b], pose_out + (long)b * 12, scale_out + b);
}

// grid (tile of 256 points, body); the expression of the header, one fma chain per coordinate.
__global__ __launch_bounds__(256) void transform_points_kernel(const float* __restrict__ src, long src_sb, int M, const int32_t* __restrict__ count,
                                                              const float* __restrict__ pose, float* __restrict__ dst) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    if (j < clamp_count(count, b, M)) {
        const float* A = pose + (long)b * 12;
        const float* p = src + (long)b * src_sb + 3L * j;
        const float px = p[0], py = p[1], pz = p[2];
        o0 = __builtin_fmaf(A[2], pz, __builtin_fmaf(A[1], py, __builtin_fmaf(A[0], px, A[9])));
        o1 = __builtin_fmaf(A[5], pz, __builtin_fmaf(A[4], py, __builtin_fmaf(A[3], px, A[10])));
        o2 = __builtin_fmaf(A[8], pz, __builtin_fmaf(A[7], py, __builtin_fmaf(A[6], px, A[11])));
    }
    float* o = dst + ((long)b * M + j) * 3;
    o[0] = o0; o[1] = o1; o[2] = o2;
}

// The checks every moments entry point makes, and the range arithmetic.  `per_range`: doubles a range stores.  *ranges: the grid's
// first dimension, 0 when there is nothing to launch.  `who` is the entry point's name in every error text.
int align_moments_check(const char* who, const float* s, int64_t s_sb, int M, const float* x, int64_t x_sb, int rows, int n, const uint8_t* v_mask,
                        int64_t mask_sb, const int32_t* idx_sm, const float* d2_sm, const AlignSurface* sf, const int32_t* idx_ms,
                        const float* d2_ms, float tau2, float w_ms, int B, const double* partials, size_t partials_bytes, int per_range,
                        int* ranges) {
    *ranges = 0;
    SH_REQUIRE(s && x && idx_sm && d2_sm && partials && (!sf || sf->uv) && (!sf || sf->faces || sf->nF == 0), SH_ERR_INVALID_ARG,
               "%s: null pointer", who);
    SH_REQUIRE(B >= 0 && M >= 0 && rows >= 0 && n >= 0 && n <= rows && (!sf || sf->nF >= 0), SH_ERR_INVALID_ARG,
               "%s: bad size (B %d, M %d, rows %d, n %d, nF %d)", who, B, M, rows, n, sf ? sf->nF : 0);
    SH_REQUIRE(w_ms >= 0.f && tau2 >= 0.f, SH_ERR_INVALID_ARG, "%s: w_ms and tau2 must be >= 0 (and not NaN)", who);
    SH_REQUIRE(!(w_ms > 0.f) || (idx_ms && d2_ms), SH_ERR_INVALID_ARG, "%s: w_ms > 0 needs idx_ms and d2_ms", who);
    if (B == 0) return SH_OK;
    SH_REQUIRE(s_sb >= 3L * M && x_sb >= 3L * rows && (!v_mask || mask_sb == 0 || mask_sb >= n), SH_ERR_INVALID_ARG,
               "%s: batch stride shorter than a body (s_sb %ld, x_sb %ld, mask_sb %ld)", who, (long)s_sb, (long)x_sb, (long)mask_sb);
    SH_REQUIRE(B <= 65535 && (long)B * M < (1L << 30) && (long)B * rows < (1L << 30) && (!sf || sf->nF < (1 << 30)), SH_ERR_UNSUPPORTED,
               "%s: B, B*M, B*rows or nF too large", who);
    const int R = sh_align_ranges(M, n, w_ms);
    const size_t need = (size_t)B * R * per_range * sizeof(double);
    SH_REQUIRE(partials_bytes >= need, SH_ERR_WORKSPACE, "%s: partials too small (%zu bytes needed)", who, need);
    *ranges = R;
    return SH_OK;
}

// The four moments entry points (sf == nullptr: the vertex forms; Sums: the closed form's or the point-to-plane step's sums): the
// checks, the normals' for the plane step, then the launch.  idx_sm / d2_sm are the surface form's face / d2; tn is read by the
// plane step only.  robust / scale2: the form of the header's "Robust terms" (the _robust twins; SH_ROBUST_NONE for the others, which
// launch the plain kernels under their plain names).
template <class Sums>
int align_moments(const char* who, const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                  const uint8_t* v_mask, int64_t mask_sb, const float* tn, const int32_t* idx_sm, const float* d2_sm, const AlignSurface* sf,
                  const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int robust, float scale2, int B, double* partials,
                  size_t partials_bytes, sh_stream_t stream) {
    int R = 0;
    if (const int rb = robust_check(who, robust, scale2)) return rb;
    const int rc = align_moments_check(who, s, s_sb, M, x, x_sb, rows, n, v_mask, mask_sb, idx_sm, d2_sm, sf, idx_ms, d2_ms, tau2, w_ms, B, partials,
                                       partials_bytes, Sums::N, &R);
    if (rc != SH_OK) return rc;
    if constexpr (Sums::NORMALS)
        SH_REQUIRE(tn || (sf && !(w_ms > 0.f)), SH_ERR_INVALID_ARG,
                   "%s: null pointer (tn: only the surface form with w_ms == 0 needs no vertex normals)", who);
    if (R == 0) return SH_OK;
    if constexpr (Sums::NORMALS) SH_REQUIRE((long)B * n < (1L << 30), SH_ERR_UNSUPPORTED, "%s: B*n too large", who);
    const int r_sm = ranges_of(M);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)R, (unsigned)B);
    robust_dispatch(robust, [&](auto form) {
        constexpr int RB = decltype(form)::value;
        if (sf) {
            ShProfScope ps(st, RB ? Sums::SCOPE_SURFACE_ROBUST : Sums::SCOPE_SURFACE, B, M, n, sf->nF, R, RB);
            SH_LAUNCH_PS(ps, (align_pairs_kernel<Sums, true, RB>), grid, dim3(NT), 0, st, s, (long)s_sb, M, s_count, x, (long)x_sb, rows, n, v_mask,
                         (long)mask_sb, tn, idx_sm, d2_sm, idx_ms, d2_ms, tau2, scale2, r_sm, *sf, partials);
        } else {
            ShProfScope ps(st, RB ? Sums::SCOPE_ROBUST : Sums::SCOPE, B, M, n, R, RB);
            SH_LAUNCH_PS(ps, (align_pairs_kernel<Sums, false, RB>), grid, dim3(NT), 0, st, s, (long)s_sb, M, s_count, x, (long)x_sb, rows, n, v_mask,
                         (long)mask_sb, tn, idx_sm, d2_sm, idx_ms, d2_ms, tau2, scale2, r_sm, AlignSurface{}, partials);
        }
    });
    SH_CHECK_LAUNCH(who + 3);                                            // named without the "sh_", as ever
    return SH_OK;
}

// The checks both solve entry points make.  `joined`: mom or sys; `pose_args`: whether all that pose_out needs is there, and
// `pose_needs` its names.
int align_solve_check(const char* who, const double* partials, const void* joined, const float* pose_out, bool pose_args, const char* pose_needs,
                      int M, int n, float w_ms, int mode, int B) {
    SH_REQUIRE(partials && (joined || pose_out), SH_ERR_INVALID_ARG, "%s: null pointer", who);
    SH_REQUIRE(!pose_out || pose_args, SH_ERR_INVALID_ARG, "%s: pose_out needs %s", who, pose_needs);
    SH_REQUIRE(B >= 0 && M >= 0 && n >= 0, SH_ERR_INVALID_ARG, "%s: bad size (B %d, M %d, n %d)", who, B, M, n);
    SH_REQUIRE(w_ms >= 0.f, SH_ERR_INVALID_ARG, "%s: w_ms must be >= 0 (and not NaN)", who);
    SH_REQUIRE(mode == SH_ALIGN_TRANSLATION || mode == SH_ALIGN_RIGID || mode == SH_ALIGN_SIMILARITY, SH_ERR_INVALID_ARG, "%s: unknown mode %d", who,
               mode);
    return SH_OK;
}

}  // namespace

extern "C" {

int sh_align_ranges(int M, int n, float w_ms) {
    if (M < 0 || n < 0) return 0;
    return ranges_of(M) + (w_ms > 0.f ? ranges_of(n) : 0);
}

size_t sh_align_partials_bytes(int B, int M, int n, float w_ms) {
    if (B <= 0) return 0;
    return (size_t)B * sh_align_ranges(M, n, w_ms) * NP * sizeof(double);
}

int sh_align_moments(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                     const uint8_t* v_mask, int64_t mask_sb, const int32_t* idx_sm, const float* d2_sm, const int32_t* idx_ms,
                     const float* d2_ms, float tau2, float w_ms, int B, double* partials, size_t partials_bytes, sh_stream_t stream) {
    return align_moments<PointSums>("sh_align_moments", s, s_sb, M, s_count, x, x_sb, rows, n, v_mask, mask_sb, nullptr, idx_sm, d2_sm, nullptr,
                                    idx_ms, d2_ms, tau2, w_ms, SH_ROBUST_NONE, 0.f, B, partials, partials_bytes, stream);
}

int sh_align_moments_robust(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                     const uint8_t* v_mask, int64_t mask_sb, const int32_t* idx_sm, const float* d2_sm, const int32_t* idx_ms,
                     const float* d2_ms, float tau2, float w_ms, int B, double* partials, size_t partials_bytes, sh_stream_t stream, int robust, float scale2) {
    return align_moments<PointSums>("sh_align_moments_robust", s, s_sb, M, s_count, x, x_sb, rows, n, v_mask, mask_sb, nullptr, idx_sm, d2_sm, nullptr,
                                    idx_ms, d2_ms, tau2, w_ms, robust, scale2, B, partials, partials_bytes, stream);
}

int sh_align_moments_surface(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                             const uint8_t* v_mask, int64_t mask_sb, const int32_t* faces, int nF, const int32_t* face, const float* uv,
                             const float* d2, const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B, double* partials,
                             size_t partials_bytes, sh_stream_t stream) {
    const AlignSurface sf{faces, nF, uv};
    return align_moments<PointSums>("sh_align_moments_surface", s, s_sb, M, s_count, x, x_sb, rows, n, v_mask, mask_sb, nullptr, face, d2, &sf,
                                    idx_ms, d2_ms, tau2, w_ms, SH_ROBUST_NONE, 0.f, B, partials, partials_bytes, stream);
}

int sh_align_moments_surface_robust(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                             const uint8_t* v_mask, int64_t mask_sb, const int32_t* faces, int nF, const int32_t* face, const float* uv,
                             const float* d2, const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B, double* partials,
                             size_t partials_bytes, sh_stream_t stream, int robust, float scale2) {
    const AlignSurface sf{faces, nF, uv};
    return align_moments<PointSums>("sh_align_moments_surface_robust", s, s_sb, M, s_count, x, x_sb, rows, n, v_mask, mask_sb, nullptr, face, d2, &sf,
                                    idx_ms, d2_ms, tau2, w_ms, robust, scale2, B, partials, partials_bytes, stream);
}

size_t sh_align_plane_partials_bytes(int B, int M, int n, float w_ms) {
    if (B <= 0) return 0;
    return (size_t)B * sh_align_ranges(M, n, w_ms) * NPP * sizeof(double);
}

int sh_align_plane_moments(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                           const uint8_t* v_mask, int64_t mask_sb, const float* tn, const int32_t* idx_sm, const float* d2_sm,
                           const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B, double* partials, size_t partials_bytes,
                           sh_stream_t stream) {
    return align_moments<PlaneSums>("sh_align_plane_moments", s, s_sb, M, s_count, x, x_sb, rows, n, v_mask, mask_sb, tn, idx_sm, d2_sm, nullptr,
                                    idx_ms, d2_ms, tau2, w_ms, SH_ROBUST_NONE, 0.f, B, partials, partials_bytes, stream);
}

int sh_align_plane_moments_robust(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                           const uint8_t* v_mask, int64_t mask_sb, const float* tn, const int32_t* idx_sm, const float* d2_sm,
                           const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B, double* partials, size_t partials_bytes,
                           sh_stream_t stream, int robust, float scale2) {
    return align_moments<PlaneSums>("sh_align_plane_moments_robust", s, s_sb, M, s_count, x, x_sb, rows, n, v_mask, mask_sb, tn, idx_sm, d2_sm, nullptr,
                                    idx_ms, d2_ms, tau2, w_ms, robust, scale2, B, partials, partials_bytes, stream);
}

int sh_align_plane_moments_surface(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                                   const uint8_t* v_mask, int64_t mask_sb, const float* tn, const int32_t* faces, int nF, const int32_t* face,
                                   const float* uv, const float* d2, const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B,
                                   double* partials, size_t partials_bytes, sh_stream_t stream) {
    const AlignSurface sf{faces, nF, uv};
    return align_moments<PlaneSums>("sh_align_plane_moments_surface", s, s_sb, M, s_count, x, x_sb, rows, n, v_mask, mask_sb, tn, face, d2, &sf,
                                    idx_ms, d2_ms, tau2, w_ms, SH_ROBUST_NONE, 0.f, B, partials, partials_bytes, stream);
}

int sh_align_plane_moments_surface_robust(const float* s, int64_t s_sb, int M, const int32_t* s_count, const float* x, int64_t x_sb, int rows, int n,
                                   const uint8_t* v_mask, int64_t mask_sb, const float* tn, const int32_t* faces, int nF, const int32_t* face,
                                   const float* uv, const float* d2, const int32_t* idx_ms, const float* d2_ms, float tau2, float w_ms, int B,
                                   double* partials, size_t partials_bytes, sh_stream_t stream, int robust, float scale2) {
    const AlignSurface sf{faces, nF, uv};
    return align_moments<PlaneSums>("sh_align_plane_moments_surface_robust", s, s_sb, M, s_count, x, x_sb, rows, n, v_mask, mask_sb, tn, face, d2, &sf,
                                    idx_ms, d2_ms, tau2, w_ms, robust, scale2, B, partials, partials_bytes, stream);
}

int sh_align_plane_solve(const double* partials, int M, int n, const int32_t* s_count, float w_ms, int mode, int B, const float* pose_in,
                         const float* scale_in, float* pose_out, float* scale_out, double* sys, int32_t* solved, sh_stream_t stream) {
    const int rc = align_solve_check("sh_align_plane_solve", partials, sys, pose_out, pose_in && scale_in && scale_out && solved,
                                     "pose_in, scale_in, scale_out and solved", M, n, w_ms, mode, B);
    if (rc != SH_OK || B == 0) return rc;
    const int r_sm = ranges_of(M), r_ms = w_ms > 0.f ? ranges_of(n) : 0;
    const int k = mode == SH_ALIGN_TRANSLATION ? 3 : (mode == SH_ALIGN_RIGID ? 6 : 7);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "align_plane_solve_kernel|B=%d ranges=%d mode=%d", B, r_sm + r_ms, mode);
    SH_LAUNCH_PS(ps, align_plane_solve_kernel, dim3((unsigned)B), dim3(64), 0, st, partials, M, n, s_count, w_ms, r_sm, r_ms, k, pose_in, scale_in,
                 pose_out, scale_out, sys, solved);
    SH_CHECK_LAUNCH("align_plane_solve");
    return SH_OK;
}

int sh_align_solve(const double* partials, int M, int n, const int32_t* s_count, float w_ms, int mode, int B, const float* pose_in,
                   const float* scale_in, float* pose_out, float* scale_out, float* inc, double* mom, sh_stream_t stream) {
    const int rc = align_solve_check("sh_align_solve", partials, mom, pose_out, pose_in && scale_in && scale_out, "pose_in, scale_in and scale_out", M,
                                     n, w_ms, mode, B);
    if (rc != SH_OK || B == 0) return rc;
    const int r_sm = ranges_of(M), r_ms = w_ms > 0.f ? ranges_of(n) : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "align_solve_kernel|B=%d ranges=%d mode=%d", B, r_sm + r_ms, mode);
    SH_LAUNCH_PS(ps, align_solve_kernel, dim3((unsigned)B), dim3(64), 0, st, partials, M, n, s_count, w_ms, r_sm, r_ms, mode, pose_in, scale_in, pose_out,
                 scale_out, inc, mom);
    SH_CHECK_LAUNCH("align_solve");
    return SH_OK;
}


int sh_transform_points(const float* src, int64_t src_sb, int M, const int32_t* count, const float* pose, int B, float* dst, sh_stream_t stream) {
    SH_REQUIRE(src && pose && dst, SH_ERR_INVALID_ARG, "sh_transform_points: null pointer");
    SH_REQUIRE(B >= 0 && M >= 0, SH_ERR_INVALID_ARG, "sh_transform_points: negative size (B %d, M %d)", B, M);
    if (B == 0 || M == 0) return SH_OK;
    SH_REQUIRE(src_sb >= 3L * M, SH_ERR_INVALID_ARG, "sh_transform_points: batch stride %ld shorter than a body", (long)src_sb);
    SH_REQUIRE(B <= 65535 && (long)B * M < (1L << 30), SH_ERR_UNSUPPORTED, "sh_transform_points: B or B*M too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ShProfScope ps(st, "transform_points_kernel|B=%d M=%d", B, M);
    SH_LAUNCH_PS(ps, transform_points_kernel, dim3((unsigned)sh_cdiv(M, 256), (unsigned)B), dim3(256), 0, st, src, (long)src_sb, M, count, pose, dst);
    SH_CHECK_LAUNCH("transform_points");
    return SH_OK;
}

}  // extern "C"
