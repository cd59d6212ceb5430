"""Host references for point-to-surface alignment (numpy only, float64): the kept rule and the foot-point expression of
include/sh_kernels.h ("sh_align_moments_surface") transcribed operation by operation, a float64 point-to-surface ICP built on
the exhaustive search of tests/surface_ref.py, and the CPU study the feature was specified from:

    python -m tests.align_surface_ref

prints, for the 170-vertex model and surface-sampled scans, where vertex ICP and surface ICP end."""
import os

import numpy as np

from tests import align_ref as A
from tests import surface_ref as S


def foot_points(x, faces, face, uv):
    """The header's partner q for the recorded (face, uv) of one body: ab, ac are fp32 differences, the rest is float64 with every
    operation rounded on its own - what the kernel computes, bit for bit.  x float32 [rows, 3]; face must index `faces`."""
    x = np.asarray(x, np.float32)
    f = np.asarray(faces, np.int64)[np.asarray(face, np.int64)]
    a, b, c = x[f[:, 0]], x[f[:, 1]], x[f[:, 2]]
    ab, ac = (b - a).astype(np.float64), (c - a).astype(np.float64)       # b - a rounds to fp32 first
    uv = np.asarray(uv, np.float32).astype(np.float64)
    return a.astype(np.float64) + (uv[:, 0:1] * ab + uv[:, 1:2] * ac)


def pairs_surface(s, x, n, m, vmask, faces, face, uv, d2, idx_ms, d2_ms, tau2, w_ms):
    """The matched pairs of sh_align_moments_surface for one body: (p [k, 3], q [k, 3], w [k]) float64.  scan -> model: j < m kept
    iff 0 <= face < nF, the face's corners lie in [0, n) and d2 < tau2 (the mask is not consulted); model -> scan: align_ref.pairs."""
    s64 = np.asarray(s, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    face = np.asarray(face, np.int64)[:m]
    tau2 = np.float32(tau2)
    ok = (face >= 0) & (face < faces.shape[0]) & (np.asarray(d2, np.float32)[:m] < tau2)
    corners = faces[np.where(ok, face, 0)] if faces.shape[0] else np.zeros((m, 3), np.int64)
    ok &= ((corners >= 0) & (corners < n)).all(1)
    j = np.nonzero(ok)[0]
    P, Q, W = [s64[j]], [foot_points(x, faces, face[j], np.asarray(uv)[j]) if j.size else np.zeros((0, 3))], \
        [np.full(j.size, 1.0 / m if m else 0.0)]
    if w_ms > 0:
        none = np.full(m, -1, np.int64)
        p2, q2, w2 = A.pairs(s, x, n, m, vmask, none, np.zeros(m, np.float32), idx_ms, d2_ms, tau2, w_ms)
        P.append(p2); Q.append(q2); W.append(w2)
    return np.concatenate(P), np.concatenate(Q), np.concatenate(W)


def icp_surface(x, faces, s, mode="similarity", iters=40, init="moments", w_ms=0.0):
    """float64 point-to-surface ICP of the scan s [m, 3] onto the triangles `faces` of the vertices x [n, 3]: the loop of
    align_ref.icp with the foot point of surface_ref.closest_f64 as the scan -> model partner.  Returns (A, t, log [iters]); log[k]
    is the surface Chamfer value BEFORE the k-th update."""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    At, t = A.moment_pose(s, x, mode == "similarity") if init == "moments" else (np.eye(3), np.zeros(3))
    m, n = len(s), len(x)
    log = np.zeros(iters)
    for k in range(iters):
        cur = A.apply(At, t, s)
        face, d2, uv = S.closest_f64(cur, x, faces)
        P, Q, W = [cur], [S.rebuild_f64(x, faces, face, uv)], [np.full(m, 1.0 / m)]
        log[k] = d2.mean()
        if w_ms > 0:
            i_ms, d_ms = A.nearest(x, cur)
            P.append(cur[i_ms]); Q.append(x); W.append(np.full(n, w_ms / n))
            log[k] += w_ms * d_ms.mean()
        dA, dt, _, _ = A.umeyama(A.moments(np.concatenate(P), np.concatenate(Q), np.concatenate(W))[0], mode)
        At, t = A.compose(dA, dt, At, t)
    return At, t, log


def surface_rms(s_model, x, faces):
    """RMS distance of model-frame points to the surface, float64."""
    return float(np.sqrt(S.closest_f64(s_model, x, faces)[1].mean()))


def scale_of(Am):
    return float(np.cbrt(np.linalg.det(Am)))


def pose_error(Am, t, s, pts):
    """The largest displacement of a scan point from its true model-frame position."""
    return float(np.sqrt(((A.apply(Am, t, np.asarray(s, np.float64)) - pts) ** 2).sum(1).max()))


def moved_surface_scan(xb, faces, case, m=2000, seed=0):
    """(scan in its own frame float32 [m, 3], the same points in the model frame float64, the true pose, the body's extent): m
    noise-free samples of the body's own surface, moved by the inverse of the case's similarity."""
    xb = np.asarray(xb, np.float64)
    pts = S.sample_surface(xb, faces, m, seed=seed).astype(np.float64)
    extent = float((xb.max(0) - xb.min(0)).max())
    At, tt = A.true_pose(case, extent)
    Ai, ti = A.inverse(At, tt)
    return A.apply(Ai, ti, pts).astype(np.float32), pts, (At, tt), extent


def study_inputs(template="small_ae.npz", m=2000):
    """The bodies, faces and moved scans of the CPU study: scan_ref.model_points(v, 4, seed=3), one case of SIMILARITY_CASES each."""
    from semantichuman_amd.hierarchy import load_hierarchy
    from tests import scan_ref
    h = load_hierarchy(os.path.join(os.path.dirname(__file__), "golden", template))
    v, faces = np.asarray(h.verts, np.float64), np.asarray(h.faces, np.int64)
    n = v.shape[0]
    x = scan_ref.model_points(v, 4, seed=3)
    moved = [moved_surface_scan(x[k, :n], faces, case, m=m, seed=100 + k) for k, case in enumerate(A.SIMILARITY_CASES)]
    return x, faces, n, moved


def study_case(xb, faces, mv, iters=40):
    """Both loops on one moved scan -> dict of the figures the host test gates."""
    s, pts, (At, tt), extent = mv
    c_true = scale_of(At)
    Av, tv = A.icp(xb, s, "similarity", iters, "moments", 0.0)
    As, ts, log = icp_surface(xb, faces, s, "similarity", iters, "moments", 0.0)
    return dict(c_true=c_true, c_vertex=scale_of(Av), c_surface=scale_of(As), e_vertex=pose_error(Av, tv, s, pts) / extent,
                e_surface=pose_error(As, ts, s, pts) / extent, log=log, extent=extent)


def _main():
    x, faces, n, moved = study_inputs()
    for k, case in enumerate(A.SIMILARITY_CASES):
        r = study_case(x[k, :n].astype(np.float64), faces, moved[k])
        rise = float((r["log"][1:] - r["log"][:-1]).max())
        print("%s: true scale %.4f; vertex ICP scale %.5f (%+.2f %%), pose error %.3g of the extent; surface ICP scale %.5f (%+.3f %%), pose "
              "error %.3g; surface Chamfer %.3g -> %.3g, largest rise %.3g"
              % (case, r["c_true"], r["c_vertex"], 100 * (r["c_vertex"] / r["c_true"] - 1), r["e_vertex"], r["c_surface"],
                 100 * (r["c_surface"] / r["c_true"] - 1), r["e_surface"], r["log"][0], r["log"][-1], rise), flush=True)


if __name__ == "__main__":
    _main()
