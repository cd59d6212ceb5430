"""Host reference for the cloud-normal tests (numpy only): the definition of include/sh_kernels.h, "Cloud normals" - distances
through scan_ref.d2_f32 (the transcription of the library's one distance expression), the tie-inclusive neighbourhood, fp32
differences widened to float64, float64 moments, numpy.linalg.eigh, the unknown rule, the sign rule and the surface variation -
plus a transcription of the fixed-sweep Jacobi the kernel runs, the inputs the tests share and the float64 study of how good the
estimate is.

`python -m tests.cloud_normals_ref` prints the study's figures; tests/test_cloud_normals_host.py pins them."""
import functools

import numpy as np

from tests.normals_ref import angle, template
from tests.scan_ref import d2_f32
from tests.surface_gated_ref import face_normals_f64, sample_surface_faces

K_MIN, K_MAX = 3, 64            # SH_CLOUD_K_MIN, SH_CLOUD_K_MAX
RANK_MIN = 1e-12                # SH_CLOUD_RANK_MIN
SWEEPS = 8                      # SH_CLOUD_JACOBI_SWEEPS
GAP_MIN = 1e-3                  # a point whose relative gap (l1 - l0) / l2 is below this is left out of the angle comparison
SIGMA = 0.002
KS = (3, 8, 16, 32, 33, 64)     # the issue's five and 32: every list capacity (8, 16, 32, 64) at its upper end, and 33 just above one

# The angle between the kernel's normal and this reference's.  Both round a unit vector to fp32 once: at most 2^-24 each in
# angle, 4 2^-24 with room for the normalisation.  Before that they differ by the eigenvector's response to the difference dC of
# the two covariance matrices, at most 2 |dC| / (l1 - l0) (Davis-Kahan).  Each of the nine sums runs over cnt terms in fp64,
# sequentially in the kernel and pairwise in numpy: error at most (cnt + 16) u sum |term| on either side, u = 2^-53, the 16
# standing for the divisions, the subtraction of the mean's products and the two eigen-solvers' own backward error.  With T =
# trace(S2) / cnt, the mean squared distance of the members from the point, sum |d_a d_b| / cnt <= T and |mean_a mean_b| <= T, so an
# entry of dC is at most 4 (cnt + 16) u T and |dC|_2 <= 12 (cnt + 16) u T.  The angle is therefore at most
#     4 2^-24 + 24 (T / l2) (cnt + 16) 2^-53 / gap,        gap = (l1 - l0) / l2.
# T / l2 compares the neighbourhood's size with its largest spread: 2 for a disc seen from its centre or from its rim; it is
# held below SPREAD_MAX = 16 on every compared point (the tests assert it), which makes c = 24 * 16.
SPREAD_MAX = 16.0
C_BOUND = 24.0 * SPREAD_MAX


def angle_bound(cnt, gap):
    return 4.0 * 2.0 ** -24 + C_BOUND * (np.asarray(cnt, np.float64) + 16.0) * 2.0 ** -53 / np.asarray(gap, np.float64)


def unsigned_angle(a, b):
    """The angle between the LINES of two unit vectors, row by row."""
    t = angle(a, b)
    return np.minimum(t, np.pi - t)


# ---------------------------------------------------------------------------------------------- the definition
def neighbourhoods(s, ks, rows=256):
    """For one cloud s float32 [m, 3] and every k of ks: r2 float32 [m] (the k_eff-th smallest d2_f32 of each row, self
    included), cnt int64 [m], and the float64 moments S1 [m, 3], S2 [m, 3, 3] of the fp32 differences s_i - s_j over the members
    d2 <= r2, in ascending i.  The distances of a block of rows are formed once for all k.  -> {k: (r2, cnt, S1, S2)}."""
    s = np.asarray(s, np.float32)
    m = s.shape[0]
    out = {k: (np.zeros(m, np.float32), np.zeros(m, np.int64), np.zeros((m, 3)), np.zeros((m, 3, 3))) for k in ks}
    for lo in range(0, m, rows):
        q = s[lo:lo + rows]
        D = d2_f32(q[:, None, :], s[None, :, :])                           # [rows, m] float32
        kth = sorted({min(k, m) - 1 for k in ks})
        Ds = np.partition(D, kth, axis=1)
        for k in ks:
            r2, cnt, S1, S2 = out[k]
            r = Ds[:, min(k, m) - 1]
            jj, ii = np.nonzero(D <= r[:, None])                           # row-major: ascending i within a row
            d = (s[ii] - q[jj]).astype(np.float64)                         # fp32 difference, then widened
            r2[lo:lo + rows] = r
            cnt[lo:lo + rows] = np.bincount(jj, minlength=q.shape[0])
            for a in range(3):
                S1[lo:lo + rows, a] = np.bincount(jj, weights=d[:, a], minlength=q.shape[0])
                for b in range(3):
                    S2[lo:lo + rows, a, b] = np.bincount(jj, weights=d[:, a] * d[:, b], minlength=q.shape[0])
    return out


def covariance(cnt, S1, S2):
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.asarray(cnt, np.float64)[:, None]
        mean = S1 / c
        return S2 / c[:, :, None] - mean[:, :, None] * mean[:, None, :]


def canonical_sign(n):
    """The component of largest magnitude made positive, the lowest index on a tie."""
    lead = n[np.arange(n.shape[0]), np.abs(n).argmax(1)]
    return np.where((lead < 0)[:, None], -n, n)


def orient(n32, s, view):
    """The viewpoint rule on rounded normals: negated where (n_x w_x + n_y w_y) + n_z w_z < 0, w = v - s in float64."""
    w = np.asarray(view, np.float32).astype(np.float64) - np.asarray(s, np.float32).astype(np.float64)
    n = n32.astype(np.float64)
    dot = (n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2]
    return np.where((dot < 0)[:, None], -n32, n32), dot


def finish(cnt, S1, S2, s=None, view=None):
    """Moments -> (normal float32 [m, 3], var float32 [m], gap float64 [m], spread float64 [m], lam [m, 3]): eigh of the
    covariance, the unknown rule (zeros), the canonical sign, the viewpoint flip, var = max(l0, 0) / (l0 + l1 + l2); gap =
    (l1 - l0) / l2 and spread = T / l2 are what the angle bound reads (inf / 0 for an unknown point)."""
    C = covariance(cnt, S1, S2)
    ok = np.isfinite(C).all((1, 2)) & (np.asarray(cnt) >= 3)
    lam, vec = np.linalg.eigh(np.where(ok[:, None, None], C, np.eye(3)))
    l0, l1, l2 = lam[:, 0], lam[:, 1], lam[:, 2]
    known = ok & (l1 > RANK_MIN * l2)
    n = vec[:, :, 0]
    n = canonical_sign(n / np.linalg.norm(n, axis=1, keepdims=True))
    n32 = np.where(known[:, None], n, 0.0).astype(np.float32)
    if view is not None:
        n32 = np.where(known[:, None], orient(n32, s, np.broadcast_to(view, n32.shape))[0], np.float32(0)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.where(known, np.maximum(l0, 0.0) / ((l0 + l1) + l2), 0.0).astype(np.float32)
        gap = np.where(known, (l1 - l0) / l2, 0.0)
        spread = np.where(known, (np.trace(S2, axis1=1, axis2=2) / np.maximum(cnt, 1)) / l2, np.inf)
    return n32, var, gap, spread, np.where(known[:, None], lam, 0.0)


def estimate(s, k, view=None):
    """The whole definition for one cloud: (normal, var, r2, cnt, gap, spread)."""
    r2, cnt, S1, S2 = neighbourhoods(s, (k,))[k]
    n, var, gap, spread, _ = finish(cnt, S1, S2, s, view)
    return n, var, r2, cnt, gap, spread


# ---------------------------------------------------------------------------------------------- the kernel's eigen-solver
def jacobi_f64(C, sweeps=SWEEPS):
    """The kernel's fixed-sweep cyclic Jacobi on a stack of symmetric 3 x 3 matrices, rotation for rotation (order (0,1) (0,2)
    (1,2), the select form of the rotation) -> (diagonal [m, 3], eigenvector columns [m, 3, 3], largest |off-diagonal| over the
    largest |diagonal| after the sweeps [m])."""
    a = np.array(C, np.float64)
    v = np.broadcast_to(np.eye(3), a.shape).copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = a[:, p, q]
                tau = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                t = np.where((apq != 0) & (t == t), t, 0.0)
                c = 1.0 / np.sqrt(1.0 + t * t)
                sn = t * c
                for M in (a, v):                                           # columns p, q
                    mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                    M[:, :, p], M[:, :, q] = c[:, None] * mp - sn[:, None] * mq, sn[:, None] * mp + c[:, None] * mq
                rp, rq = a[:, p, :].copy(), a[:, q, :].copy()              # rows p, q
                a[:, p, :], a[:, q, :] = c[:, None] * rp - sn[:, None] * rq, sn[:, None] * rp + c[:, None] * rq
        diag = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], 1)
        off = np.max(np.abs(np.stack([a[:, 0, 1], a[:, 0, 2], a[:, 1, 2]], 1)), 1) / np.abs(diag).max(1)
    return diag, v, off


# ---------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def samples(name, M, seed=5, sigma=0.0):
    """M surface samples of a golden template - the vertices themselves, not a synth_batch body - with the float64 normals of the
    faces they came from: (points float32 [M, 3], normals float64 [M, 3])."""
    v, f = template(name)
    p, face = sample_surface_faces(v, f, M, seed=seed, sigma=sigma)
    return p, face_normals_f64(v, f)[face]


@functools.lru_cache(maxsize=None)
def reference(name, M, seed=5, sigma=0.0, ks=KS):
    """neighbourhoods() of samples(name, M, seed, sigma) for every k of ks, computed once and shared; treat as read-only."""
    return neighbourhoods(samples(name, M, seed, sigma)[0], ks)


def lattice():
    """A 6 x 6 x 2 integer lattice - many exact ties at every k-th distance - and five more exact copies of one of its points."""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(2), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    return np.concatenate([g, np.repeat(g[14:15], 5, 0)], 0)


def collinear(m=40):
    t = np.arange(m, dtype=np.float32)
    return np.stack([t, 2 * t, -t], 1) * np.float32(0.125)


def planar(m=300, seed=2):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.rand(m, 2), np.zeros((m, 1))], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the study
STUDY_CASES = (("template6890.npz", 5000, 16, 0.0), ("template6890.npz", 5000, 8, SIGMA), ("small_ae.npz", 1000, 16, 0.0))
# measured by `python -m tests.cloud_normals_ref` (seed 5): median and 90th percentile of the unsigned angle to the source
# face's normal in degrees - test_cloud_normals_host.py pins them
STUDY_MEDIAN = (1.241, 4.674, 4.612)
STUDY_P90 = (3.943, 10.486, 14.354)
STUDY_TOL = 0.002               # degrees: the figures above are printed to three decimals


def study_case(name, M, k, sigma):
    """-> (median, 90th percentile) of the unsigned angle in degrees between the estimate and the source face's normal over the
    points the estimate knows, the smallest relative gap, the share of points with a gap below GAP_MIN, the largest spread."""
    s, fn = samples(name, M, sigma=sigma)
    n, var, r2, cnt, gap, spread = estimate(s, k)
    known = np.abs(n).sum(1) > 0
    a = np.degrees(unsigned_angle(n[known], fn[known]))
    return float(np.median(a)), float(np.percentile(a, 90)), float(gap[known].min()), float((gap < GAP_MIN).mean()), float(spread[known].max())


if __name__ == "__main__":
    for case in STUDY_CASES + (("small_ae.npz", 63, 16, 0.0),):
        print("%-18s M=%-5d k=%-3d sigma=%-6g median %.3f deg  p90 %.3f deg  smallest gap %.3e  share below %.0e: %.4f  largest spread %.2f"
              % (case + study_case(*case)[:2] + (study_case(*case)[2], GAP_MIN) + study_case(*case)[3:]), flush=True)
    rs = np.random.RandomState(0)
    A = rs.randn(20000, 3, 3)
    A = A + A.transpose(0, 2, 1)
    A[:5000] = np.einsum("mi,mj->mij", A[:5000, 0], A[:5000, 0])           # rank one
    A[5000:10000, 2, :] = 0; A[5000:10000, :, 2] = 0                        # a zero row and column
    for sw in (3, 4, 5, 6, 8):
        print("jacobi: %d sweeps leave an off-diagonal of at most %.3e of the diagonal (20000 random, rank-one and singular matrices)"
              % (sw, np.nanmax(jacobi_f64(A, sw)[2])))
