"""Host reference for the robust terms (include/sh_kernels.h, "Robust terms"), float64 numpy: the penalty rho and its weight
w = d rho / d u, the Chamfer value and gradient under it on given matches, both pose steps under weights (the pairs of
align_ref / align_surface_ref / align_plane_ref with every pair's weight multiplied by w of its recorded distance), a float64
IRLS ICP, and the inputs of the outlier experiment the host and the GPU test share."""
import functools
import os

import numpy as np

from semantichuman_amd.hierarchy import load_hierarchy
from tests import align_plane_ref as AP
from tests import align_ref as A
from tests import align_surface_ref as AS
from tests import scan_ref as R

FORMS = ("geman-mcclure", "huber")
# the extra fp32 roundings of the kernels' rho and w over the float64 expressions below, in units of 2^-24 relative (derived in
# tests/test_robust.py where they are used)
RHO_ULPS, W_ULPS = 4.0, 5.0


def rho(u, form, scale2):
    """The penalty of a truncated squared distance u, float64."""
    u = np.asarray(u, np.float64)
    if form is None:
        return u
    if form == "geman-mcclure":
        return u * (scale2 / (scale2 + u))
    if form == "huber":
        inside = u <= scale2
        return np.where(inside, u, 2.0 * np.sqrt(scale2 * u) - scale2)
    raise ValueError(form)


def weight(u, form, scale2):
    """d rho / d u, float64; 1 for form None."""
    u = np.asarray(u, np.float64)
    if form is None:
        return np.ones_like(u)
    if form == "geman-mcclure":
        t = scale2 / (scale2 + u)
        return t * t
    if form == "huber":
        inside = u <= scale2
        return np.where(inside, 1.0, np.sqrt(scale2 / np.where(inside, 1.0, u)))
    raise ValueError(form)


def pair_weights(d2, form, scale2, tau2=np.inf):
    """What scan.robust_weights returns: w of the kept pairs (d2 < tau2), 0 for the others."""
    d2 = np.asarray(d2, np.float64)
    keep = d2 < tau2
    return np.where(keep, weight(np.where(keep, d2, 0.0), form, scale2), 0.0)


# ------------------------------------------------------------------------------------------------ value and gradient
def chamfer_value(d2_sm, m, d2_ms, n, vmask, tau2, w_ms, form, scale2):
    """L of sh_chamfer_fwd_robust for one body from recorded distances (fp32 arrays, widened): float64."""
    if m == 0:
        return 0.0
    L = rho(np.minimum(np.asarray(d2_sm[:m], np.float64), tau2), form, scale2).sum() / m
    act = np.ones(n, bool) if vmask is None else np.asarray(vmask, bool)[:n]
    if w_ms > 0 and act.sum():
        L += float(np.float32(w_ms)) * rho(np.minimum(np.asarray(d2_ms[:n], np.float64)[act], tau2), form, scale2).sum() / act.sum()
    return float(L)


def chamfer_grad(x, s, n, m, vmask, tau2, w_ms, form, scale2, idx_ms, d2_ms, idx_sm=None, d2_sm=None, surface=None):
    """(g [rows, 3], mag [rows, 3]) float64: the gradient of that value w.r.t. the model points on the recorded matches, for
    gL = 1, and the sum of the absolute values of the terms each element is made of.  Vertex partner: idx_sm / d2_sm; surface
    partner: surface = (faces, face, uv, d2), the weights of the foot point taken as constants."""
    x64, s64 = np.asarray(x, np.float64), np.asarray(s, np.float64)
    g, mag = np.zeros_like(x64), np.zeros_like(x64)
    tau2 = np.float32(tau2)
    if m == 0:
        return g, mag
    act = np.ones(n, bool) if vmask is None else np.asarray(vmask, bool)[:n]
    if surface is None:
        j = np.nonzero((idx_sm[:m] >= 0) & (idx_sm[:m] < n) & (d2_sm[:m] < tau2))[0]
        w = weight(d2_sm[j], form, scale2)
        term = (2.0 / m) * w[:, None] * (x64[idx_sm[j]] - s64[j])
        np.add.at(g, idx_sm[j], term)
        np.add.at(mag, idx_sm[j], np.abs(term))
    else:
        faces, face, uv, d2 = surface
        faces = np.asarray(faces, np.int64).reshape(-1, 3)
        fc = np.asarray(face, np.int64)[:m]
        j = np.nonzero((fc >= 0) & (fc < faces.shape[0]) & (np.asarray(d2, np.float32)[:m] < tau2))[0]
        w = weight(np.asarray(d2)[j], form, scale2)
        q = AS.foot_points(x, faces, fc[j], np.asarray(uv)[j]) if j.size else np.zeros((0, 3))
        l = np.asarray(uv, np.float64)[j]
        lam = np.stack([1.0 - l[:, 0] - l[:, 1], l[:, 0], l[:, 1]], 1)
        for k in range(3):
            term = (2.0 / m) * (w * lam[:, k])[:, None] * (q - s64[j])
            np.add.at(g, faces[fc[j], k], term)
            np.add.at(mag, faces[fc[j], k], np.abs(term))
    if w_ms > 0 and act.sum():
        i = np.nonzero(act & (idx_ms[:n] >= 0) & (idx_ms[:n] < m) & (d2_ms[:n] < tau2))[0]
        term = float(np.float32(w_ms)) * (2.0 / act.sum()) * weight(d2_ms[i], form, scale2)[:, None] * (x64[i] - s64[idx_ms[i]])
        g[i] += term
        mag[i] += np.abs(term)
    g[:n][~act] = 0.0                                                      # a masked vertex takes no gradient, whatever points at it
    g[n:] = 0.0
    return g, mag


# ------------------------------------------------------------------------------------------------ pose steps under weights
def _kept_d2(n, m, vmask, d2_sm_kept, idx_ms, d2_ms, tau2, w_ms):
    """The recorded distances of the kept pairs in the order align_ref.pairs lists them: scan -> model, then model -> scan."""
    out = [np.asarray(d2_sm_kept, np.float64)]
    if w_ms > 0:
        act = np.ones(n, bool) if vmask is None else np.asarray(vmask, bool)[:n]
        i = np.nonzero(act & (idx_ms[:n] >= 0) & (idx_ms[:n] < m) & (d2_ms[:n] < np.float32(tau2)))[0]
        if m and act.sum():
            out.append(np.asarray(d2_ms[i], np.float64))
    return np.concatenate(out)


def weighted_pairs(s, x, n, m, vmask, idx_ms, d2_ms, tau2, w_ms, form, scale2, idx_sm=None, d2_sm=None, surface=None, tn=None, plane=False):
    """The kept pairs of a robust moments call for one body with their full weights (direction weight times w of the recorded
    distance): (p, q, w) or, with plane=True, (p, q, nrm, w).  surface = (faces, face, uv, d2) or None (idx_sm / d2_sm)."""
    tau2 = np.float32(tau2)
    if surface is None:
        keep = (idx_sm[:m] >= 0) & (idx_sm[:m] < n) & (d2_sm[:m] < tau2)
        d_kept = np.asarray(d2_sm[:m])[keep]
    else:
        faces, face, uv, d2 = surface
        fa = np.asarray(faces, np.int64).reshape(-1, 3)
        fc = np.asarray(face, np.int64)[:m]
        keep = (fc >= 0) & (fc < fa.shape[0]) & (np.asarray(d2, np.float32)[:m] < tau2)
        corners = fa[np.where(keep, fc, 0)] if fa.shape[0] else np.zeros((m, 3), np.int64)
        keep &= ((corners >= 0) & (corners < n)).all(1)
        d_kept = np.asarray(d2[:m])[keep]
    if plane:
        p, q, nrm, w = AP.pairs_plane(s, x, n, m, vmask, idx_sm, d2_sm, idx_ms, d2_ms, tau2, w_ms, tn=tn, surface=surface)
    elif surface is None:
        none_i, none_d = np.full(n, -1, np.int64), np.zeros(n, np.float32)
        p, q, w = A.pairs(s, x, n, m, vmask, idx_sm, d2_sm, idx_ms if w_ms > 0 else none_i, d2_ms if w_ms > 0 else none_d, tau2, w_ms)
    else:
        p, q, w = AS.pairs_surface(s, x, n, m, vmask, *surface, idx_ms, d2_ms, tau2, w_ms)
    d = _kept_d2(n, m, vmask, d_kept, idx_ms, d2_ms, tau2, w_ms)
    assert d.shape == w.shape, (d.shape, w.shape)
    w = w * weight(d, form, scale2)
    return (p, q, nrm, w) if plane else (p, q, w)


# ------------------------------------------------------------------------------------------------ float64 IRLS ICP
def icp(x, s, mode="similarity", iters=40, init="moments", w_ms=1.0, form=None, scale2=1.0, tau2=np.inf):
    """align_ref.icp with every pair weighed by w of its own squared distance (float64 throughout, the search included):
    (A, t).  form=None is align_ref.icp itself."""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    Am, t = A.moment_pose(s, x, mode == "similarity") if init == "moments" else (np.eye(3), np.zeros(3))
    m, n = len(s), len(x)
    for _ in range(iters):
        cur = A.apply(Am, t, s)
        i_sm, d_sm = A.nearest(cur, x)
        keep = d_sm < tau2
        P, Q, W = [cur[keep]], [x[i_sm[keep]]], [weight(d_sm[keep], form, scale2) / m]
        if w_ms > 0:
            i_ms, d_ms = A.nearest(x, cur)
            keep = d_ms < tau2
            P.append(cur[i_ms[keep]]); Q.append(x[keep]); W.append(w_ms * weight(d_ms[keep], form, scale2) / n)
        dA, dt, _, _ = A.umeyama(A.moments(np.concatenate(P), np.concatenate(Q), np.concatenate(W))[0], mode)
        Am, t = A.compose(dA, dt, Am, t)
    return Am, t


def pose_error(Am, t, truth):
    """(rotation angle in degrees, |translation| difference, |scale ratio - 1|) of a pose against the true one; the translation
    is compared where it acts, at the model's side: t - t_true."""
    At, tt = truth
    c, ct = np.cbrt(np.linalg.det(Am)), np.cbrt(np.linalg.det(At))
    Rd = (Am / c) @ (At / ct).T
    ang = np.degrees(np.arccos(np.clip((np.trace(Rd) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(np.asarray(t) - np.asarray(tt))), float(abs(c / ct - 1.0))


# ------------------------------------------------------------------------------------------------ the outlier experiment
OUTLIER_SEED = 11
OUTLIER_SHARE = 0.15
OUTLIER_CASE = (10.0, 1.1, 0.1)            # align_ref.SIMILARITY_CASES[0]: degrees about AXIS, scale, shift / extent
OUTLIER_SIGMA = 0.03                       # of the body's extent: three times the scan's jitter
OUTLIER_M = 2000
OUTLIER_ITERS = 30


def outlier_inputs(xb):
    """The 170-vertex body's experiment: a jittered scan of xb [n, 3] under OUTLIER_CASE plus OUTLIER_SHARE extra points drawn
    uniformly in a box that hangs on the +x side of the body (a hand-held object: no counterpart on the model, one-sided, so
    least squares is biased towards it).  -> (scan float32 [m', 3] in its own frame, the true pose (A, t), sigma in model units,
    the extent)."""
    xb = np.asarray(xb, np.float64)
    scan, pts, truth = A.moved_scan(xb, OUTLIER_CASE, m=OUTLIER_M, seed=OUTLIER_SEED)
    extent = (xb.max(0) - xb.min(0)).max()
    rs = np.random.RandomState(OUTLIER_SEED + 1)
    lo = np.array([xb[:, 0].max() + 0.05 * extent, xb[:, 1].mean() - 0.15 * extent, xb[:, 2].mean() - 0.15 * extent])
    box = lo + rs.rand(int(round(OUTLIER_SHARE * OUTLIER_M)), 3) * np.array([0.3, 0.3, 0.3]) * extent
    Ai, ti = A.inverse(*truth)
    cloud = np.concatenate([scan, A.apply(Ai, ti, box).astype(np.float32)])
    return cloud, truth, OUTLIER_SIGMA * extent, extent


def outlier_body():
    """The 170-vertex body of the experiment: (x float32 [1, n + 1, 3], n)."""
    v = np.asarray(load_hierarchy(os.path.join(os.path.dirname(__file__), "golden", "small_ae.npz")).verts, np.float64)
    return R.model_points(v, 1, seed=3), v.shape[0]


@functools.lru_cache(maxsize=None)
def outlier_reference():
    """The float64 loops of the outlier experiment: {form: (angle, translation, scale) error}, form None the plain loop."""
    x, n = outlier_body()
    xb = x[0, :n].astype(np.float64)
    cloud, truth, sigma, extent = outlier_inputs(xb)
    out = {}
    for form in (None,) + FORMS:
        Am, t = icp(xb, cloud, iters=OUTLIER_ITERS, form=form, scale2=sigma * sigma)
        out[form] = pose_error(Am, t, truth)
    return out
