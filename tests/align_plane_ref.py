"""Host references for the point-to-plane pose step (numpy only, float64): the pairs, the normals, the Jacobian row, the sums and
the solve of include/sh_kernels.h ("sh_align_plane_moments", "sh_align_plane_solve") transcribed operation by operation, a
float64 point-to-plane ICP built on the exhaustive search of tests/surface_ref.py, and the CPU study the feature was specified
from:

    python -m tests.align_plane_ref

prints, for the 170-vertex model and surface-sampled scans, the pose error of the point-to-point and the point-to-plane loop by
iteration."""
import numpy as np

from tests import align_ref as A
from tests import align_surface_ref as AS
from tests import normals_ref as N
from tests import scan_ref as R
from tests import surface_ref as S

NSYS = 37                                                                  # SH_ALIGN_PLANE_SYSTEM
MODE_K = {"translation": 3, "rigid": 6, "similarity": 7}
PIVOT_MIN = 1e-12                                                          # SH_ALIGN_PLANE_PIVOT_MIN
SERIES_BELOW = 1e-8                                                        # theta^2 below which Rodrigues' factors are series
TRI = [(i, j) for i in range(7) for j in range(i, 7)]                      # the 28 upper-triangle entries, row-major


# ------------------------------------------------------------------------------------------------ normals and pairs
def face_normals(x, faces, face):
    """The header's normal of the recorded face: ab = b - a, ac = c - a and the cross product fma(u, v, -(w * z)) in fp32 (the
    expression of "Vertex normals"), then float64: len = sqrt((cx cx + cy cy) + cz cz), c / len, zero when len is not positive
    and finite.  x float32 [rows, 3]; face must index `faces`."""
    x = np.asarray(x, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)[np.asarray(face, np.int64)]
    a, b, c = x[f[:, 0]], x[f[:, 1]], x[f[:, 2]]
    ab, ac = b - a, c - a
    with np.errstate(over="ignore", invalid="ignore"):
        cr = np.stack([R.fma32(ab[:, 1], ac[:, 2], -(ab[:, 2] * ac[:, 1])),
                       R.fma32(ab[:, 2], ac[:, 0], -(ab[:, 0] * ac[:, 2])),
                       R.fma32(ab[:, 0], ac[:, 1], -(ab[:, 1] * ac[:, 0]))], 1).astype(np.float64)
        ln = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
        ok = (ln > 0) & np.isfinite(ln)
        return np.where(ok[:, None], cr / np.where(ok, ln, 1.0)[:, None], 0.0)


def pairs_plane(s, x, n, m, vmask, idx_sm, d2_sm, idx_ms, d2_ms, tau2, w_ms, tn=None, surface=None):
    """The kept pairs of sh_align_plane_moments (surface=None: idx_sm / d2_sm are the vertex matches) or of
    sh_align_plane_moments_surface (surface=(faces, face, uv, d2)) for one body: (p, q, nrm [k, 3], w [k]) float64.  The kept
    rule, the weights and the order are those of align_ref.pairs / align_surface_ref.pairs_surface; tn float32 [n, 3] are the
    vertex normals (needed unless surface is given and w_ms == 0)."""
    x32 = np.asarray(x, np.float32)
    tn64 = None if tn is None else np.asarray(tn, np.float32).astype(np.float64)
    tau2 = np.float32(tau2)
    if surface is not None:
        faces, face, uv, d2 = surface
        p, q, w = AS.pairs_surface(s, x, n, m, vmask, faces, face, uv, d2, None, None, tau2, 0.0)
        fa = np.asarray(faces, np.int64).reshape(-1, 3)
        fc = np.asarray(face, np.int64)[:m]
        ok = (fc >= 0) & (fc < fa.shape[0]) & (np.asarray(d2, np.float32)[:m] < tau2)
        corners = fa[np.where(ok, fc, 0)] if fa.shape[0] else np.zeros((m, 3), np.int64)
        ok &= ((corners >= 0) & (corners < n)).all(1)
        nrm = face_normals(x32, fa, fc[ok]) if ok.any() else np.zeros((0, 3))
    else:
        none_i, none_d = np.full(n, -1, np.int64), np.zeros(n, np.float32)
        p, q, w = A.pairs(s, x, n, m, vmask, idx_sm, d2_sm, none_i, none_d, tau2, 0.0)
        j = np.nonzero((idx_sm[:m] >= 0) & (idx_sm[:m] < n) & (d2_sm[:m] < tau2))[0]
        nrm = tn64[idx_sm[j]]
    P, Q, Nr, W = [p], [q], [nrm], [w]
    if w_ms > 0:
        none = np.full(m, -1, np.int64)
        p2, q2, w2 = A.pairs(s, x, n, m, vmask, none, np.zeros(m, np.float32), idx_ms, d2_ms, tau2, w_ms)
        act = np.ones(n, bool) if vmask is None else np.asarray(vmask, bool)[:n]
        i = np.nonzero(act & (idx_ms[:n] >= 0) & (idx_ms[:n] < m) & (d2_ms[:n] < tau2))[0]
        P.append(p2); Q.append(q2); W.append(w2); Nr.append(tn64[i] if len(w2) else np.zeros((0, 3)))
    return np.concatenate(P), np.concatenate(Q), np.concatenate(Nr), np.concatenate(W)


def residual(p, q, nrm):
    """r = (n0 (p0 - q0) + n1 (p1 - q1)) + n2 (p2 - q2)."""
    d = p - q
    return (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]


def jacobian(p, nrm):
    """J [k, 7] = [nrm, p x nrm, nrm . p] - the derivative of r under p' = p + omega x p + sigma p + t, in the order t, omega, sigma."""
    cr = np.stack([p[:, 1] * nrm[:, 2] - p[:, 2] * nrm[:, 1], p[:, 2] * nrm[:, 0] - p[:, 0] * nrm[:, 2],
                   p[:, 0] * nrm[:, 1] - p[:, 1] * nrm[:, 0]], 1)
    dot = (nrm[:, 0] * p[:, 0] + nrm[:, 1] * p[:, 1]) + nrm[:, 2] * p[:, 2]
    return np.concatenate([nrm, cr, dot[:, None]], 1)


def plane_system(p, q, nrm, w):
    """(values [38], sum w |term| [38]) float64.  Entries 0 .. 36 are the joined system of sh_align_plane_solve ([0] W = sum w,
    [1..28] the upper triangle of sum w J J^T row-major, [29..35] sum w J r, [36] sum w r^2); entry 37 is the number of kept pairs.
    With w = 1 the first 37 are the sums a range stores at SH_ALIGN_PLANE_PARTIAL slots 0 .. 36."""
    J, r = jacobian(p, nrm), residual(p, q, nrm)
    cols = [np.ones(len(w))] + [J[:, i] * J[:, j] for i, j in TRI] + [J[:, i] * r for i in range(7)] + [r * r]
    val = np.array([(w * c).sum() for c in cols] + [float(len(w))])
    mag = np.array([(w * np.abs(c)).sum() for c in cols] + [0.0])
    return val, mag


def unpack(sys):
    """(H [7, 7] symmetric, g [7]) of a joined system."""
    H = np.zeros((7, 7))
    for c, (i, j) in enumerate(TRI):
        H[i, j] = H[j, i] = sys[1 + c]
    return H, np.asarray(sys[29:36], np.float64).copy()


def rodrigues(om):
    """exp of the cross-product matrix of om: I + a K + b K^2, a = sin(th) / th, b = (1 - cos(th)) / th^2, by series below
    th^2 = 1e-8."""
    th2 = float(om @ om)
    if th2 < SERIES_BELOW:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = np.sqrt(th2)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]], np.float64)
    return np.eye(3) + a * K + b * (K @ K)


def scaled_block(sys, mode):
    """The leading k x k block of H scaled to unit diagonal, or None when a diagonal entry is not positive and finite."""
    k = MODE_K[mode]
    H, g = unpack(sys)
    d = np.diag(H)[:k]
    if not (np.isfinite(d).all() and (d > 0).all()):
        return None
    sd = np.sqrt(d)
    return H[:k, :k] / np.outer(sd, sd), g[:k] / sd, sd


def plane_solve(sys, mode):
    """sh_align_plane_solve's lane 0 in float64: (c R, t, c, R, solved, delta [7]).  Diagonal scaling, Cholesky, H delta = -g on the
    leading block of the mode; singular (solved = 0, the identity) when W == 0, a diagonal entry is not positive and finite, or
    a pivot of the scaled block is <= 1e-12."""
    ident = (np.eye(3), np.zeros(3), 1.0, np.eye(3), 0, np.zeros(7))
    if not sys[0] > 0:
        return ident
    sc = scaled_block(sys, mode)
    if sc is None:
        return ident
    Hs, gs, sd = sc
    k = len(gs)
    L = np.zeros((k, k))
    for j in range(k):
        piv = Hs[j, j] - (L[j, :j] ** 2).sum()
        if not piv > PIVOT_MIN:
            return ident
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, k):
            L[i, j] = (Hs[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.zeros(k)
    for i in range(k):
        y[i] = (-gs[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    z = np.zeros(k)
    for i in range(k - 1, -1, -1):
        z[i] = (y[i] - (L[i + 1:, i] * z[i + 1:]).sum()) / L[i, i]
    delta = np.zeros(7)
    delta[:k] = z / sd
    if not np.isfinite(delta).all():
        return ident
    c = float(np.exp(delta[6]))
    Rm = rodrigues(delta[3:6])
    return c * Rm, delta[:3].copy(), c, Rm, 1, delta


def condition(sys, mode):
    """cond_2 of the scaled block (inf when it does not exist)."""
    sc = scaled_block(sys, mode)
    return np.inf if sc is None else float(np.linalg.cond(sc[0]))


# ------------------------------------------------------------------------------------------------ float64 point-to-plane ICP
def icp_plane(x, faces, s, mode="similarity", iters=10, init="moments", w_ms=0.0, normals="face", trace=None):
    """float64 point-to-plane ICP of the scan s [m, 3] onto the model x [n, 3] with triangles `faces`: the loop of
    align_surface_ref.icp_surface with plane_solve of the pairs' system in place of the closed form.  normals: "face" - partner
    the foot point of surface_ref.closest_f64, normal that of its face; "phong" - the same partner, the normal the foot point's
    barycentric blend of the vertex normals, renormalised; "vertex" - the vertex form: partner the nearest vertex, normal the
    vertex normal.  The model -> scan pairs (w_ms > 0) are (cur[nn(x_i)], x_i) with the vertex normal.  Returns (A, t, log [iters],
    solved [iters]); log[k] is the Chamfer value of the pairs BEFORE the k-th update.  trace: a list that receives (A, t) after
    every update."""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    faces = np.asarray(faces, np.int64)
    At, t = A.moment_pose(s, x, mode == "similarity") if init == "moments" else (np.eye(3), np.zeros(3))
    m, n = len(s), len(x)
    vn = N.normals_f64(x, faces) if (normals != "face" or w_ms > 0) else None
    log, solved = np.zeros(iters), np.zeros(iters, np.int64)
    for k in range(iters):
        cur = A.apply(At, t, s)
        if normals == "vertex":
            i_sm, d2 = A.nearest(cur, x)
            q, nrm = x[i_sm], vn[i_sm]
        else:
            face, d2, uv = S.closest_f64(cur, x, faces)
            q = S.rebuild_f64(x, faces, face, uv)
            f = faces[face]
            if normals == "face":
                cr = np.cross(x[f[:, 1]] - x[f[:, 0]], x[f[:, 2]] - x[f[:, 0]])
            else:
                l1, l2 = uv[:, 0:1], uv[:, 1:2]
                cr = (1 - l1 - l2) * vn[f[:, 0]] + l1 * vn[f[:, 1]] + l2 * vn[f[:, 2]]
            ln = np.sqrt((cr * cr).sum(1, keepdims=True))
            nrm = np.where(ln > 0, cr / np.where(ln > 0, ln, 1.0), 0.0)
        P, Q, Nr, W = [cur], [q], [nrm], [np.full(m, 1.0 / m)]
        log[k] = d2.mean()
        if w_ms > 0:
            i_ms, d_ms = A.nearest(x, cur)
            P.append(cur[i_ms]); Q.append(x); Nr.append(vn); W.append(np.full(n, w_ms / n))
            log[k] += w_ms * d_ms.mean()
        sys, _ = plane_system(np.concatenate(P), np.concatenate(Q), np.concatenate(Nr), np.concatenate(W))
        dA, dt, _, _, solved[k], _ = plane_solve(sys, mode)
        At, t = A.compose(dA, dt, At, t)
        if trace is not None:
            trace.append((At, t))
    return At, t, log, solved


def plane_errors(xb, faces, mv, iters=10, normals="face"):
    """(pose error / extent after 1 .. iters updates, log, the condition numbers of the scaled systems are not kept)."""
    s, pts, _, extent = mv
    trace = []
    _, _, log, solved = icp_plane(xb, faces, s, "similarity", iters, "moments", 0.0, normals, trace)
    return np.array([AS.pose_error(Ak, tk, s, pts) / extent for Ak, tk in trace]), log, solved


def point_errors(xb, faces, mv, at=(5, 10, 20, 39)):
    """The point-to-point surface loop's pose error / extent after the given numbers of updates (the loop is deterministic, so a
    shorter run is a prefix of a longer one)."""
    s, pts, _, extent = mv
    out = []
    for k in at:
        Ak, tk, _ = AS.icp_surface(xb, faces, s, "similarity", k, "moments", 0.0)
        out.append(AS.pose_error(Ak, tk, s, pts) / extent)
    return np.array(out)


def first_below(errors, level=1e-3):
    """The first iteration (1-based) whose error lies below `level`, or None."""
    hit = np.nonzero(np.asarray(errors) < level)[0]
    return int(hit[0]) + 1 if hit.size else None


def _main():
    x, faces, n, moved = AS.study_inputs()
    for k, case in enumerate(A.SIMILARITY_CASES):
        xb = x[k, :n].astype(np.float64)
        ep = point_errors(xb, faces, moved[k])
        ef, log, _ = plane_errors(xb, faces, moved[k])
        eb, _, _ = plane_errors(xb, faces, moved[k], normals="phong")
        rise = float((log[1:] - log[:-1]).max())
        print("%s: point-to-point 5 / 10 / 20 / 39: %s; point-to-plane (face normals) 5 / 10: %.2g / %.2g, first below 1e-3 at %s "
              "(blended normals: %s); largest rise of the log %.3g"
              % (case, " / ".join("%.2g" % e for e in ep), ef[4], ef[9], first_below(ef), first_below(eb), rise), flush=True)


if __name__ == "__main__":
    _main()
