"""Host reference of the rig merge (include/sh_kernels.h, "Depth views: overlap" and "Scan compaction"), numpy only, on top of
tests/depth_views_ref.py and tests/depth_ref.py: the header's expressions one operation at a time in float32 - the quality q of
a row under every camera, the projection into every other camera in sh_free_space_fwd's form, the depth read and the two tests
on it - then `keep` and `seen`, and the stable compaction with `view_first` and the padding."""
import numpy as np

from tests import depth_ref as R
from tests import depth_views_ref as RV

F32 = np.float32


def quality(P, n, t):
    """q of rows P, n float32 [m, 3] under the camera centre t float32 [3] -> float32 [m]: cos^2 / d^4 with the cosine's sign."""
    P, n, t = np.asarray(P, F32), np.asarray(n, F32), np.asarray(t, F32)
    with np.errstate(all="ignore"):
        ex, ey, ez = t[0] - P[:, 0], t[1] - P[:, 1], t[2] - P[:, 2]
        len2 = (ex * ex + ey * ey) + ez * ez
        dot = (n[:, 0] * ex + n[:, 1] * ey) + n[:, 2] * ez
        q = (dot * np.abs(dot)) / ((len2 * len2) * len2)
        assert q.dtype == F32
    return np.where(len2 == 0, F32(0), q)


def project(P, ext, intr, H, W):
    """Rows P float32 [m, 3] (rig frame) into the camera ext float32 [3, 4] with intr = (fx, fy, cx, cy) -> (Q_z float32 [m], hit
    bool [m]: in front and inside the image, u, v int64 [m]: the nearest pixel, 0 where not hit)."""
    e = np.asarray(ext, F32).reshape(3, 4)
    fx, fy, cx, cy = (F32(v) for v in intr)
    with np.errstate(all="ignore"):
        d = [P[:, i] - e[i, 3] for i in range(3)]
        X, Y, Z = ((e[0, j] * d[0] + e[1, j] * d[1]) + e[2, j] * d[2] for j in range(3))
        assert Z.dtype == F32
        front = Z > 0
        uf, vf = (X * fx) / Z + cx, (Y * fy) / Z + cy
        inside = (uf >= F32(-0.5)) & (uf < F32(W) - F32(0.5)) & (vf >= F32(-0.5)) & (vf < F32(H) - F32(0.5))
        hit = front & inside
        u = np.minimum(np.floor(np.where(hit, uf, F32(0)) + F32(0.5)), F32(W - 1)).astype(np.int64)
        v = np.minimum(np.floor(np.where(hit, vf, F32(0)) + F32(0.5)), F32(H - 1)).astype(np.int64)
    return Z, hit, u, v


def overlap(points, normals, view, depths, intrs, exts, tol, depth_scale=1.0, masks=None, z_range=None):
    """One body's live rows (points, normals float32 [m, 3], view uint8 [m]) against its V images -> (keep bool [m], seen uint32
    [m]).  depths [V] images, intrs [V] (or one) intrinsics, exts [V, 3, 4] / [V, 12] float32, a NaN anywhere: the view is absent."""
    V, m = len(depths), len(points)
    intrs = [intrs] * V if np.ndim(intrs) == 1 else intrs
    P, n, own = np.asarray(points, F32).reshape(m, 3), np.asarray(normals, F32).reshape(m, 3), np.asarray(view).astype(np.int64)
    e = np.asarray(exts, F32).reshape(V, 3, 4)
    present = ~np.isnan(e).any((1, 2))
    q = np.zeros((V, m), F32)
    for c in np.flatnonzero(present):
        q[c] = quality(P, n, e[c, :, 3])
    q_own = q[own, np.arange(m)]
    seen = (np.uint32(1) << own.astype(np.uint32)).astype(np.uint32)
    keep = np.ones(m, bool)
    for c in np.flatnonzero(present):
        img = R.unproject(depths[c], intrs[c], depth_scale=depth_scale, mask=None if masks is None else masks[c], z_range=z_range)
        H, W = img.z.shape
        Z, hit, u, v = project(P, e[c], intrs[c], H, W)
        with np.errstate(all="ignore"):
            agree = np.abs(img.z[v, u] - Z) <= F32(tol)
        obs = hit & img.valid[v, u] & agree & (own != c)
        seen |= obs.astype(np.uint32) << np.uint32(c)
        keep &= ~(obs & ((q[c] > q_own) | ((q[c] == q_own) & (c < own))))
    return keep, seen


class Merged(RV.Fused):
    """A Fused after the merge: its rows, and `seen` uint32 [m] (`refs` is not carried)."""


def compact(points, normals, pixel, view, seen, keep, V):
    """The kept rows in their old order -> Merged; view_first[v] = the kept rows of the views below v."""
    keep = np.asarray(keep, bool)
    out = Merged()
    out.points, out.normals, out.pixel, out.view, out.seen = points[keep], normals[keep], pixel[keep], view[keep], seen[keep]
    out.view_first = np.asarray([int((out.view < v).sum()) for v in range(V + 1)], np.int32)
    return out


def merge(fused, depths, intrs, exts, tol, **options):
    """A Fused of depth_views_ref and the images it came from -> (Merged, keep bool [m], seen uint32 [m])."""
    keep, seen = overlap(fused.points, fused.normals, fused.view, depths, intrs, exts, tol, **options)
    return compact(fused.points, fused.normals, fused.pixel, fused.view, seen, keep, len(depths)), keep, seen


def pack(bodies, width=None):
    """A list of Merged -> (points, normals, pixel, view, seen [B, M], counts [B], view_first [B, V + 1]) as sh_scan_compact pads
    them: zeros, zeros, -1, 255, 0; M = width, or the largest count and at least 1."""
    points, normals, pixel, view, counts, first = RV.pack(bodies, width)
    seen = np.zeros(pixel.shape, np.uint32)
    for b, f in enumerate(bodies):
        seen[b, :counts[b]] = f.seen
    return points, normals, pixel, view, seen, counts, first


def pack_planes(planes, width=None):
    """Per-body row planes [m_b] of one dtype -> [B, M] with zeros in the padding (keep and seen as sh_depth_views_overlap pads)."""
    M = max(max(len(p) for p in planes), 1) if width is None else width
    out = np.zeros((len(planes), M), planes[0].dtype)
    for b, p in enumerate(planes):
        out[b, :len(p)] = p
    return out


# ------------------------------------------------------------------------------------------------ scenes
def look_at(centre, target, up=(0.0, -1.0, 0.0)):
    """A camera at `centre` whose +z axis points at `target` -> extrinsics float32 [3, 4] (camera -> rig; x right, y down)."""
    c, t = np.asarray(centre, np.float64), np.asarray(target, np.float64)
    z = (t - c) / np.linalg.norm(t - c)
    x = np.cross(-np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), c[:, None]], 1).astype(F32)


def render(H, W, intr, ext, surface):
    """The depth image of camera (intr, ext float32 [3, 4]) looking at `surface`, a function (origin float64 [3], rays float64
    [H, W, 3] in the rig frame, unit z in the camera's) -> depth float64 [H, W] along the camera's z (NaN: a miss) -> float32."""
    e = np.asarray(ext, np.float64)
    with np.errstate(all="ignore"):
        return surface(e[:, 3], R.rays(H, W, intr) @ e[:, :3].T).astype(F32)


def plane_z(z0):
    """The plane z = z0 of the rig frame as a `render` surface."""
    def hit(o, r):
        t = (z0 - o[2]) / r[..., 2]
        return np.where(t > 0, t, np.nan)
    return hit


def ellipsoid(centre=(0.0, 0.0, 0.0), radii=(0.25, 0.6, 0.18)):
    """An ellipsoid of the rig frame as a `render` surface: the nearer intersection."""
    c, s = np.asarray(centre, np.float64), 1.0 / np.asarray(radii, np.float64)

    def hit(o, r):
        a, d = (o - c) * s, r * s
        dd, ad = (d * d).sum(-1), d @ a
        disc = ad * ad - dd * (a @ a - 1.0)
        t = (-ad - np.sqrt(np.where(disc > 0, disc, np.nan))) / dd
        return np.where(t > 0, t, np.nan)
    return hit


def ring(V, radius=1.6, height=0.0, phase=0.3):
    """V cameras on a circle around the rig's origin, each looking at it -> extrinsics float32 [V, 3, 4]."""
    return np.stack([look_at((radius * np.sin(phase + 2 * np.pi * k / V), height, -radius * np.cos(phase + 2 * np.pi * k / V)), (0, 0, 0))
                     for k in range(V)])
