"""Host reference of the lens model (include/sh_kernels.h, "Camera rays"), numpy only, in the header's order of operations: the
inverse (rays, limit, complete) in float64 and rounded once, the forward projection in float32, the unprojection with a ray
table for one camera and for a rig (on tests/depth_ref.py and tests/depth_views_ref.py), the overlap rule and the free-space
case list with a table (on tests/views_merge_ref.py, tests/field_ref.py and tests/field_views_ref.py), a float64 restatement of
the term, and the scenes the distortion tests share: depth cast along the reference's own rays."""
import math

import numpy as np

from tests import depth_ref as R
from tests import depth_views_ref as RV
from tests import field_ref as RF
from tests import field_views_ref as RFV
from tests import views_merge_ref as RM

F32 = np.float32
F64 = np.float64
STEPS = 20
TOL_PX = 1e-3

# (k1, k2, p1, p2, k3, k4, k5, k6).  AZURE: a rational set with tangential terms of the size a time-of-flight camera of the
# Azure-Kinect kind is calibrated to (8 pixels at the corners of the test image); BARREL: plain radial; BROWN5: a 5-coefficient
# Brown-Conrady set, padded; FOLDING: k1 alone, not invertible beyond r = 0.86 (1 + 3 k1 r^2 = 0).
AZURE = (5.0, 3.3, 1.0e-4, -5.0e-5, 0.17, 5.3, 4.9, 0.9)
BARREL = (-0.18, 0.03, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
BROWN5 = (-0.12, 0.05, 8.0e-4, -5.0e-4, -0.01)
FOLDING = (-0.45,)
H, W = 29, 37                           # 2 x 3 tiles of 16, ragged both ways
INTR = (28.0, 27.0, 17.6, 13.8)         # fx about 28: r exceeds 1 in the corners


def pad8(d):
    """4, 5 or 8 (or here: any leading part of) coefficients -> float32 [8], zero-padded in OpenCV's order."""
    out = np.zeros(8, F32)
    out[:len(d)] = np.asarray(d, F32)
    return out


def _terms(a, b, d, T):
    """The header's shared expressions at (a, b) in the type T -> (num, den, tx, ty), one rounded operation at a time."""
    k1, k2, p1, p2, k3, k4, k5, k6 = (T(v) for v in d)
    one, two = T(1), T(2)
    a2, b2 = a * a, b * b
    r2 = a2 + b2
    r4 = r2 * r2
    r6 = r4 * r2
    num = ((one + k1 * r2) + k2 * r4) + k3 * r6
    den = ((one + k4 * r2) + k5 * r4) + k6 * r6
    ab = a * b
    tx = (two * p1) * ab + p2 * (r2 + two * a2)
    ty = p1 * (r2 + two * b2) + (two * p2) * ab
    return num, den, tx, ty


def forward64(x, y, intr, d):
    """The forward model in float64 on float32 parameters -> (u, v, num, den)."""
    fx, fy, cx, cy = (F64(F32(v)) for v in intr)
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    with np.errstate(all="ignore"):
        num, den, tx, ty = _terms(x, y, pad8(d), F64)
        rad = num / den
        return fx * (x * rad + tx) + cx, fy * (y * rad + ty) + cy, num, den


def invert(intr, d, u, v):
    """The header's inverse at the samples (u, v), float64 arrays -> (x, y float64, converged bool)."""
    fx, fy, cx, cy = (F64(F32(t)) for t in intr)
    u, v = np.asarray(u, F64), np.asarray(v, F64)
    d = pad8(d)
    with np.errstate(all="ignore"):
        xd, yd = (u - cx) / fx, (v - cy) / fy
        x, y = xd.copy(), yd.copy()
        for _ in range(STEPS):
            num, den, tx, ty = _terms(x, y, d, F64)
            s = den / num
            x, y = (xd - tx) * s, (yd - ty) * s
        uu, vv, num, den = forward64(x, y, intr, d)
        ok = (np.abs(uu - u) <= TOL_PX) & (np.abs(vv - v) <= TOL_PX) & (num > 0) & (den > 0)
    return x, y, ok


def ray_r2(x, y):
    """The header's r2 of a ray: float32 from the rounded ray, the forward model's own form."""
    xf, yf = np.asarray(x).astype(F32), np.asarray(y).astype(F32)
    with np.errstate(all="ignore"):
        r2 = xf * xf + yf * yf
    assert r2.dtype == F32
    return r2


def boundary(H, W):
    """The image rectangle's boundary samples at half-pixel positions -> (u, v) float64."""
    i, j = np.arange(W + 1, dtype=F64), np.arange(H + 1, dtype=F64)
    u = np.concatenate([i - 0.5, i - 0.5, np.full(H + 1, -0.5), np.full(H + 1, W - 0.5)])
    v = np.concatenate([np.full(W + 1, -0.5), np.full(W + 1, H - 0.5), j - 0.5, j - 0.5])
    return u, v


def camera_rays(intr, d, H, W):
    """One camera -> (rays float32 [H, W, 2], NaN where not converged; limit float32; complete int)."""
    u, v = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    x, y, ok = invert(intr, d, u, v)
    rays = np.where(ok[..., None], np.stack([x, y], -1), np.nan).astype(F32)
    bx, by, bok = invert(intr, d, *boundary(H, W))
    r2 = np.concatenate([ray_r2(x, y)[ok], ray_r2(bx, by)[bok]])
    return rays, (r2.max() if r2.size else F32(0)), int(ok.all())


def project(x, intr, d, limit, H, W):
    """The forward model in float32 on camera-frame points float32 [n, 3] -> (uf, vf, inside, u, v): field_ref.project's results
    under the lens; a point beyond the limit, or with a NaN, is not inside.  u, v are 0 where not inside."""
    X, Y, Z = (np.ascontiguousarray(x[:, k], F32) for k in range(3))
    fx, fy, cx, cy = (F32(t) for t in intr)
    with np.errstate(all="ignore"):
        a, b = X / Z, Y / Z
        num, den, tx, ty = _terms(a, b, pad8(d), F32)
        r2 = a * a + b * b
        rad = num / den
        uf = fx * (a * rad + tx) + cx
        vf = fy * (b * rad + ty) + cy
        assert uf.dtype == F32 and r2.dtype == F32
        inside = (Z > 0) & (r2 <= F32(limit)) & (uf >= F32(-0.5)) & (uf < F32(W) - F32(0.5)) & (vf >= F32(-0.5)) & (vf < F32(H) - F32(0.5))
        u = np.minimum(np.floor(np.where(inside, uf, F32(0)) + F32(0.5)), F32(W - 1)).astype(np.int64)
        v = np.minimum(np.floor(np.where(inside, vf, F32(0)) + F32(0.5)), F32(H - 1)).astype(np.int64)
    return uf, vf, inside, u, v


# ------------------------------------------------------------------------------------------------ unprojection with a table
def unproject(depth, table, depth_scale=1.0, mask=None, z_range=None, max_step=None, drop_isolated=False, stride=1):
    """depth_ref.unproject with the points from a ray table float32 [H, W, 2]: P = (ra z, rb z, z) in float32, and the mask rule -
    a pixel without a ray counts as masked; everything after the points is depth_ref's, restated on the same fields."""
    depth = np.asarray(depth)
    H, W = depth.shape
    has_ray = ~np.isnan(table).any(-1)
    mask = has_ray if mask is None else has_ray & (np.asarray(mask) != 0)
    out = R.unproject(depth, (1.0, 1.0, 0.0, 0.0), depth_scale, mask, z_range, max_step, False, 1)      # z, valid and usable: pixel space
    z, valid, usable = out.z, out.valid, out.usable
    with np.errstate(all="ignore"):
        P = np.stack([table[..., 0] * z, table[..., 1] * z, z], -1)
        assert P.dtype == F32
        Pn = {key: R._neighbour(P, du, dv, F32(np.nan)) for key, (du, dv) in {"L": (-1, 0), "R": (1, 0), "U": (0, -1), "D": (0, 1)}.items()}

        def tangent(lo, hi):
            a = np.where(usable[hi][..., None], Pn[hi], P)
            b = np.where(usable[lo][..., None], Pn[lo], P)
            return (a - b).astype(F64), usable[lo] | usable[hi]

        (dx, has_dx), (dy, has_dy) = tangent("L", "R"), tangent("U", "D")
        c0 = dx[..., 1] * dy[..., 2] - dx[..., 2] * dy[..., 1]
        c1 = dx[..., 2] * dy[..., 0] - dx[..., 0] * dy[..., 2]
        c2 = dx[..., 0] * dy[..., 1] - dx[..., 1] * dy[..., 0]
        len2 = (c0 * c0 + c1 * c1) + c2 * c2
        known = valid & has_dx & has_dy & (len2 > 0)
        Pd = P.astype(F64)
        away = (c0 * Pd[..., 0] + c1 * Pd[..., 1]) + c2 * Pd[..., 2] > 0
        n = np.stack([c0, c1, c2], -1) / np.sqrt(len2)[..., None]
        n = np.where(away[..., None], -n, n)
        normal = np.where(known[..., None], n, 0.0).astype(F32)
    ui, vi = np.meshgrid(np.arange(W), np.arange(H))
    kept = valid & (ui % stride == 0) & (vi % stride == 0)
    if drop_isolated:
        kept &= known
    ku, kv = ui[kept], vi[kept]
    order = np.lexsort((R.z_rank(ku % R.TILE, kv % R.TILE), ku // R.TILE, kv // R.TILE))
    ku, kv = ku[order], kv[order]
    out.P, out.normal, out.known, out.kept = P, normal, known, kept
    out.points, out.normals = P[kv, ku], normal[kv, ku]
    out.pixel = (kv * W + ku).astype(np.int32)
    return out


def unproject_views(depths, tables, exts, masks=None, **options):
    """One body of a rig: depths [V] images, tables [V] ray tables, exts [V, 3, 4] / [V, 12] float32 (a NaN anywhere: absent) ->
    depth_views_ref.Fused, by depth_views_ref.move on this module's per-view reference."""
    V = len(depths)
    out = RV.Fused()
    out.refs, pts, nrm, pix, view, first = [], [], [], [], [], [0]
    for k in range(V):
        e = np.asarray(exts[k], F32).reshape(3, 4)
        if np.isnan(e).any():
            out.refs.append(None)
        else:
            ref = unproject(depths[k], tables[k], mask=None if masks is None else masks[k], **options)
            p, n = RV.move(ref, e)
            out.refs.append(ref)
            pts.append(p), nrm.append(n), pix.append(ref.pixel), view.append(np.full(len(ref.pixel), k, np.uint8))
        first.append(sum(len(p) for p in pix))
    out.points = np.concatenate(pts).astype(F32) if pts else np.zeros((0, 3), F32)
    out.normals = np.concatenate(nrm).astype(F32) if nrm else np.zeros((0, 3), F32)
    out.pixel = np.concatenate(pix).astype(np.int32) if pix else np.zeros(0, np.int32)
    out.view = np.concatenate(view) if view else np.zeros(0, np.uint8)
    out.view_first = np.asarray(first, np.int32)
    return out


def overlap(points, normals, view, depths, intrs, dists, tables, limits, exts, tol, depth_scale=1.0, masks=None, z_range=None):
    """views_merge_ref.overlap under the lens: the point in camera c's frame by its expressions, the pixel by `project`, validity
    with the mask rule."""
    V, m = len(depths), len(points)
    P, n, own = np.asarray(points, F32).reshape(m, 3), np.asarray(normals, F32).reshape(m, 3), np.asarray(view).astype(np.int64)
    e = np.asarray(exts, F32).reshape(V, 3, 4)
    present = ~np.isnan(e).any((1, 2))
    q = np.zeros((V, m), F32)
    for c in np.flatnonzero(present):
        q[c] = RM.quality(P, n, e[c, :, 3])
    q_own = q[own, np.arange(m)]
    seen = (np.uint32(1) << own.astype(np.uint32)).astype(np.uint32)
    keep = np.ones(m, bool)
    for c in np.flatnonzero(present):
        img = unproject(depths[c], tables[c], depth_scale=depth_scale, mask=None if masks is None else masks[c], z_range=z_range)
        Hc, Wc = img.z.shape
        with np.errstate(all="ignore"):
            d = [P[:, i] - e[c, i, 3] for i in range(3)]
            Q = np.stack([(e[c, 0, j] * d[0] + e[c, 1, j] * d[1]) + e[c, 2, j] * d[2] for j in range(3)], 1)
            assert Q.dtype == F32
            _, _, hit, u, v = project(Q, intrs[c], dists[c], limits[c], Hc, Wc)
            agree = np.abs(img.z[v, u] - Q[:, 2]) <= F32(tol)
        obs = hit & img.valid[v, u] & agree & (own != c)
        seen |= obs.astype(np.uint32) << np.uint32(c)
        keep &= ~(obs & ((q[c] > q_own) | ((q[c] == q_own) & (c < own))))
    return keep, seen


# ------------------------------------------------------------------------------------------------ the free-space term with a table
class Lens:
    """One camera's calibration as the term reads it: intr, d float32 [8], table float32 [H, W, 2], limit float32."""

    def __init__(self, intr, d, H, W):
        self.intr, self.d = np.asarray(intr, F32), pad8(d)
        self.table, self.limit, self.complete = camera_rays(intr, d, H, W)

    def has_ray(self):
        return ~np.isnan(self.table).any(-1)


def terms(x, n, f, lens, v_mask=None, margin=0.0):
    """field_ref.terms under a lens: x float32 [rows, 3] in the camera's frame, f a field_ref.Field -> (term, kind, g, counts)."""
    Hf, Wf = f.cls.shape
    x = np.asarray(x, F32)[:n]
    active = np.ones(n, bool) if v_mask is None else np.asarray(v_mask)[:n] != 0
    X, Y, Z = (np.ascontiguousarray(x[:, k]) for k in range(3))
    _, _, inside, u, v = project(x, lens.intr, lens.d, lens.limit, Hf, Wf)
    c = f.cls[v, u]
    kind = np.full(n, RF.NONE, np.uint8)
    term, g = np.zeros(n, F32), np.zeros((n, 3), F32)
    kind[active & ~inside] = RF.OUTSIDE
    kind[active & inside & (c == RF.UNKNOWN)] = RF.AT_UNKNOWN
    with np.errstate(all="ignore"):
        e = (f.z[v, u] - F32(margin)) - Z
        free = active & inside & (c == RF.SURFACE) & (e > 0)
        kind[free] = RF.FREE
        term[free] = (e * e)[free]
        g[free, 2] = (F32(-2) * e)[free]
        q = f.nearest[v, u].astype(np.int64)
        ray = lens.table.reshape(-1, 2)[np.maximum(q, 0)]
        a, b = ray[:, 0], ray[:, 1]
        sil = active & inside & (c == RF.EMPTY) & (q >= 0) & ~np.isnan(a) & ~np.isnan(b)
        rx = X - a * Z
        ry = Y - b * Z
        kind[sil] = RF.SILHOUETTE
        term[sil] = (rx * rx + ry * ry)[sil]
        g[sil, 0] = (F32(2) * rx)[sil]
        g[sil, 1] = (F32(2) * ry)[sil]
        g[sil, 2] = (F32(-2) * (a * rx + b * ry))[sil]
    assert term.dtype == F32 and g.dtype == F32 and e.dtype == F32 and rx.dtype == F32
    counts = np.asarray([active.sum(), (kind == RF.FREE).sum(), (kind == RF.SILHOUETTE).sum(), (kind == RF.OUTSIDE).sum()], np.int32)
    return term, kind, g, counts


def terms_views(x, n, fields, lenses, cam, v_mask=None, margin=0.0):
    """field_views_ref.terms under lenses: x in the model's frame, cam float32 [V, 12] -> (term [V, n], kind [V, n], g [V, n, 3],
    counts [V, 4])."""
    per = [terms(RFV.transform(np.asarray(x, F32)[:n], cam[v]), n, f, lenses[v], v_mask, margin) for v, f in enumerate(fields)]
    return tuple(np.stack([p[j] for p in per]) for j in range(4))


def terms64(x, n, f, lens, v_mask=None, margin=0.0):
    """The term restated in float64 under a lens: the forward model, the guard, the pixel rule and the cases in float64 on the
    float32 table and limit -> (free [n], silhouette [n], kind [n], pixel [n]: v * W + u or -1, the number of active vertices)."""
    Hf, Wf = f.cls.shape
    x = np.asarray(x, F64)[:n]
    active = np.ones(n, bool) if v_mask is None else np.asarray(v_mask)[:n] != 0
    X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
    with np.errstate(all="ignore"):
        a, b = X / Z, Y / Z
        uf, vf, _, _ = forward64(a, b, lens.intr, lens.d)
        inside = active & (Z > 0) & (a * a + b * b <= F64(lens.limit)) & (uf >= -0.5) & (uf < Wf - 0.5) & (vf >= -0.5) & (vf < Hf - 0.5)
        u = np.where(inside, np.floor(uf + 0.5), 0).astype(np.int64)
        v = np.where(inside, np.floor(vf + 0.5), 0).astype(np.int64)
        c = f.cls[v, u]
        e = f.z[v, u].astype(F64) - float(margin) - Z
        is_free = inside & (c == RF.SURFACE) & (e > 0)
        q = f.nearest[v, u].astype(np.int64)
        ray = lens.table.reshape(-1, 2)[np.maximum(q, 0)].astype(F64)
        rx, ry = X - ray[:, 0] * Z, Y - ray[:, 1] * Z
        is_sil = inside & (c == RF.EMPTY) & (q >= 0) & ~np.isnan(ray).any(1)
    kind = np.where(is_free, RF.FREE, np.where(is_sil, RF.SILHOUETTE, RF.NONE))
    return np.where(is_free, e * e, 0.0), np.where(is_sil, rx * rx + ry * ry, 0.0), kind, np.where(inside, v * Wf + u, -1), int(active.sum())


def losses64(x, n, f, lens, v_mask=None, margin=0.0):
    free, sil, _, _, n_act = terms64(x, n, f, lens, v_mask, margin)
    return (math.fsum(free) / n_act, math.fsum(sil) / n_act) if n_act else (0.0, 0.0)


# ------------------------------------------------------------------------------------------------ scenes
def cast(table, surface, ext=None):
    """The depth image of a camera whose pixels look along the reference's rays (x, y, 1), float32 table widened: `surface` as
    views_merge_ref.render takes it (origin, rays in the surface's frame -> depth along the camera's z, NaN: a miss).  ext float32
    [3, 4]: camera -> surface frame, None: the identity.  Pixels without a ray get NaN."""
    e = np.concatenate([np.eye(3), np.zeros((3, 1))], 1) if ext is None else np.asarray(ext, F64).reshape(3, 4)
    dirs = np.concatenate([table.astype(F64), np.ones(table.shape[:2] + (1,))], -1)
    with np.errstate(all="ignore"):
        return surface(e[:, 3], dirs @ e[:, :3].T).astype(F32)


def plane(normal=(0.15, -0.1, 1.0), through=(0.0, 0.0, 2.0)):
    """The plane normal . (P - through) = 0 as a `cast` surface, and its residual function P -> normal . (P - through) / |normal|."""
    n, p0 = np.asarray(normal, F64), np.asarray(through, F64)

    def hit(o, r):
        t = (n @ (p0 - o)) / (r @ n)
        return np.where(t > 0, t, np.nan)

    return hit, lambda P: (np.asarray(P, F64) - p0) @ n / np.linalg.norm(n)


def ellipsoid(centre=(0.05, -0.03, 2.5), radii=(4.0, 3.5, 0.8)):
    """An ellipsoid in front of the camera, wide enough to fill the image, as a `cast` surface, and its residual function P ->
    sum(((P - centre) / radii)^2) - 1."""
    c, s = np.asarray(centre, F64), 1.0 / np.asarray(radii, F64)
    return RM.ellipsoid(centre, radii), lambda P: (((np.asarray(P, F64) - c) * s) ** 2).sum(-1) - 1.0


def with_holes(depth, seed=0):
    """depth_ref.holes, and a miss (NaN) stays a hole."""
    return R.holes(depth, seed)


def render_mesh(vertices, faces, lens, H, W, background, samples=12):
    """field_ref.render through a lens: dense barycentric samples of every face of a camera-frame mesh, each projected by the
    forward model in float64 (samples beyond the limit are dropped) to its nearest pixel, the minimum depth per pixel."""
    v = np.asarray(vertices, F64)
    f = np.asarray(faces, np.int64)
    i, j = np.meshgrid(np.arange(samples + 1), np.arange(samples + 1), indexing="ij")
    keep = i + j <= samples
    w1, w2 = i[keep] / samples, j[keep] / samples
    w0 = 1.0 - w1 - w2
    P = (w0[None, :, None] * v[f[:, 0]][:, None, :] + w1[None, :, None] * v[f[:, 1]][:, None, :]
         + w2[None, :, None] * v[f[:, 2]][:, None, :]).reshape(-1, 3)
    P = P[P[:, 2] > 0]
    a, b = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    uf, vf, _, _ = forward64(a, b, lens.intr, lens.d)
    ok = (a * a + b * b <= F64(lens.limit)) & np.isfinite(uf) & np.isfinite(vf)
    pu, pv = np.floor(uf[ok] + 0.5).astype(np.int64), np.floor(vf[ok] + 0.5).astype(np.int64)
    z = P[ok, 2]
    ok = (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
    depth = np.full(H * W, np.inf)
    np.minimum.at(depth, pv[ok] * W + pu[ok], z[ok])
    return np.where(np.isfinite(depth), depth, background).astype(F32).reshape(H, W)
