"""Host references for the alignment tests (numpy only; scipy's KD-tree speeds the float64 ICP up when it is installed): the
header's fp32 transform mirrored bit for bit, the weighted moments in float64, Umeyama's SVD solution of the same moments, pose
algebra in float64, a float64 ICP, and the moved scans the tests share."""
import numpy as np

from tests import scan_ref as R

try:
    from scipy.spatial import cKDTree
except ImportError:                                                        # the brute-force float64 search of scan_ref does the same job
    cKDTree = None

AXIS = np.array([1.0, 2.0, 3.0])
SHIFT_DIR = np.array([0.6, -0.5, 0.62])
# (degrees about AXIS, scale, translation along SHIFT_DIR as a fraction of the body's extent): the true pose scan -> model
SIMILARITY_CASES = [(10.0, 1.1, 0.1), (20.0, 1.2, 0.3), (30.0, 0.8, 0.5), (45.0, 1.3, 0.5)]
RIGID_HALF_CASES = [(5.0, 0.02), (10.0, 0.05), (15.0, 0.05)]             # (degrees, translation fraction), scale 1, half scans


# ------------------------------------------------------------------------------------------------ pose algebra, float64
def rotation(axis, degrees):
    """Rodrigues: the rotation by `degrees` about `axis`."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def apply(A, t, p):
    return p @ np.asarray(A, np.float64).T + np.asarray(t, np.float64)


def compose(A1, t1, A0, t0):
    """(A1, t1) after (A0, t0)."""
    return A1 @ A0, A1 @ t0 + t1


def inverse(A, t):
    Ai = np.linalg.inv(A)
    return Ai, -Ai @ t


def pack(A, t):
    return np.concatenate([np.asarray(A, np.float32).reshape(9), np.asarray(t, np.float32).reshape(3)])


def transform_f32(pose12, p):
    """include/sh_kernels.h, sh_transform_points: dst_r = fma(A[r][2], z, fma(A[r][1], y, fma(A[r][0], x, t[r]))), bit for bit.
    pose12 float32 [12], p float32 [m, 3]."""
    P = np.asarray(pose12, np.float32)
    p = np.asarray(p, np.float32)
    out = np.empty_like(p)
    for r in range(3):
        a0, a1, a2, t = (np.full(p.shape[0], P[k], np.float32) for k in (3 * r, 3 * r + 1, 3 * r + 2, 9 + r))
        out[:, r] = R.fma32(a2, p[:, 2], R.fma32(a1, p[:, 1], R.fma32(a0, p[:, 0], t)))
    return out


# ------------------------------------------------------------------------------------------------ moments and their solution
def pairs(s, x, n, m, vmask, idx_sm, d2_sm, idx_ms, d2_ms, tau2, w_ms):
    """The matched pairs of the header for one body from given match arrays: (p [k, 3], q [k, 3], w [k]) float64."""
    s, x = np.asarray(s, np.float64), np.asarray(x, np.float64)
    tau2 = np.float32(tau2)
    j = np.nonzero((idx_sm[:m] >= 0) & (idx_sm[:m] < n) & (d2_sm[:m] < tau2))[0]
    P, Q, W = [s[j]], [x[idx_sm[j]]], [np.full(j.size, 1.0 / m if m else 0.0)]
    if w_ms > 0:
        act = np.ones(n, bool) if vmask is None else np.asarray(vmask, bool)[:n]
        i = np.nonzero(act & (idx_ms[:n] >= 0) & (idx_ms[:n] < m) & (d2_ms[:n] < tau2))[0]
        if m and act.sum():
            P.append(s[idx_ms[i]]); Q.append(x[i]); W.append(np.full(i.size, float(np.float32(w_ms)) / act.sum()))
    return np.concatenate(P), np.concatenate(Q), np.concatenate(W)


def moments(p, q, w):
    """[20] float64 in the header's layout, and sum w |.| of every entry (what a summation-order bound scales with)."""
    def both(f):
        return np.array([(w * c).sum() for c in f]), np.array([(w * np.abs(c)).sum() for c in f])
    cols = [np.ones(len(w))] + [p[:, k] for k in range(3)] + [q[:, k] for k in range(3)]
    cols += [q[:, r] * p[:, c] for r in range(3) for c in range(3)] + [(p * p).sum(1), (q * q).sum(1)]
    val, mag = both(cols)
    return np.concatenate([val, [len(w), 0.0]]), np.concatenate([mag, [0.0, 0.0]])


def umeyama(mom, mode):
    """The least-squares pose of the moments by SVD (Umeyama 1991): (c R, t, c, R).  mode as scan.align."""
    W = mom[0]
    if not W > 0:
        return np.eye(3), np.zeros(3), 1.0, np.eye(3)
    pb, qb = mom[1:4] / W, mom[4:7] / W
    H = mom[7:16].reshape(3, 3) / W - np.outer(qb, pb)
    Rm, c = np.eye(3), 1.0
    if mode != "translation":
        U, S, Vt = np.linalg.svd(H)
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
        Rm = U @ D @ Vt
    if mode == "similarity":
        var_p = mom[16] / W - pb @ pb
        num = np.trace(Rm.T @ H)
        c = num / var_p if (var_p > 0 and num > 0) else 1.0
    return c * Rm, qb - c * Rm @ pb, c, Rm


def residual(p, q, w, A, t):
    """sum w |A p + t - q|^2 over the pairs."""
    return float((w * ((apply(A, t, p) - q) ** 2).sum(1)).sum())


# ------------------------------------------------------------------------------------------------ float64 ICP
def nearest(q, t):
    """(index, squared distance) of the nearest t for every q, float64."""
    if cKDTree is not None:
        d, i = cKDTree(t).query(q)
        return i, d * d
    i, d2, _ = R.nearest_f64(q, t)
    return i, d2


def rms_scan_to_model(s, x):
    return float(np.sqrt(nearest(s, x)[1].mean()))


def moment_pose(s, x, scale=True):
    cs, cx = s.mean(0), x.mean(0)
    c = np.sqrt(((x - cx) ** 2).sum(1).mean() / ((s - cs) ** 2).sum(1).mean()) if scale else 1.0
    return c * np.eye(3), cx - c * cs


def icp(x, s, mode="similarity", iters=40, init="moments", w_ms=1.0):
    """float64 ICP of the scan s [m, 3] onto the vertices x [n, 3] with the pairs and weights of the header; (A, t)."""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    A, t = moment_pose(s, x, mode == "similarity") if init == "moments" else (np.eye(3), np.zeros(3))
    m, n = len(s), len(x)
    for _ in range(iters):
        cur = apply(A, t, s)
        i_sm, d_sm = nearest(cur, x)
        i_ms, d_ms = nearest(x, cur) if w_ms > 0 else (None, None)
        p, q, w = pairs(cur, x, n, m, None, i_sm, d_sm.astype(np.float32), i_ms, None if d_ms is None else d_ms.astype(np.float32), np.inf, w_ms)
        dA, dt, _, _ = umeyama(moments(p, q, w)[0], mode)
        A, t = compose(dA, dt, A, t)
    return A, t


# ------------------------------------------------------------------------------------------------ the shared cases
def jittered_scan(xb, m, seed):
    """scan_ref.make_scans' recipe on the body's OWN vertices: 1 % jitter, m points with replacement; float64, model frame."""
    rs = np.random.RandomState(seed)
    src = np.asarray(xb, np.float64)
    extent = (src.max(0) - src.min(0)).max()
    pts = src + 0.01 * extent * rs.randn(src.shape[0], 3)
    return pts[rs.randint(0, src.shape[0], size=int(m))], extent


def true_pose(case, extent):
    deg, c, frac = case
    return c * rotation(AXIS, deg), frac * extent * SHIFT_DIR


def moved_scan(xb, case, m=20011, seed=0, half=False):
    """(scan in its own frame float32 [m', 3], the same points in the model frame float64, the true pose (A, t))."""
    pts, extent = jittered_scan(xb, m, seed)
    if half:
        pts = pts[pts[:, 0] > np.median(pts[:, 0])]
    A, t = true_pose(case, extent)
    Ai, ti = inverse(A, t)
    return apply(Ai, ti, pts).astype(np.float32), pts, (A, t)
