"""Host reference of the depth-image kernels (include/sh_kernels.h, "Depth images"), numpy only: the header's expressions one by
one - float32 for depth, validity and points, float64 for the normal - and the output order by sorting the kept pixels on (tile
row, tile column, Z-rank).  Also the analytic scenes the depth tests share."""
import numpy as np

TILE = 16
F32 = np.float32
Z_RANGE = (0.5, 5.0)                    # what the scenes' surfaces lie in; the `holes` value 9.0 does not


def z_rank(lu, lv):
    """Rank of pixel (lu, lv) of a tile, 0 <= lu, lv < 16: bit k of lu -> bit 2k, bit k of lv -> bit 2k + 1."""
    lu, lv = np.asarray(lu, np.int64), np.asarray(lv, np.int64)
    r = np.zeros(np.broadcast(lu, lv).shape, np.int64)
    for k in range(4):
        r |= ((lu >> k) & 1) << (2 * k) | ((lv >> k) & 1) << (2 * k + 1)
    return r


def _neighbour(a, du, dv, fill):
    """a[v + dv, u + du] for every (v, u); `fill` outside the image."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    out[max(-dv, 0):H - max(dv, 0), max(-du, 0):W - max(du, 0)] = a[max(dv, 0):H + min(dv, 0), max(du, 0):W + min(du, 0)]
    return out


class Unprojected:
    """One image's reference: per pixel `z`, `valid`, `P` [H, W, 3], `usable` {"L", "R", "U", "D"}, `normal` [H, W, 3], `known`,
    `kept`; and the packed rows `points`, `normals` [m, 3] float32, `pixel` [m] int32 in the contract's order."""


def unproject(depth, intr, depth_scale=1.0, mask=None, z_range=None, max_step=None, drop_isolated=False, stride=1):
    """The reference of one image: depth [H, W] float32 or uint16, intr = (fx, fy, cx, cy) -> Unprojected."""
    depth = np.asarray(depth)
    assert depth.ndim == 2 and depth.dtype in (np.float32, np.uint16)
    H, W = depth.shape
    fx, fy, cx, cy = (F32(v) for v in intr)
    near, far = (F32(-np.inf), F32(np.inf)) if z_range is None else (F32(z_range[0]), F32(z_range[1]))
    step = F32(np.inf) if max_step is None else F32(max_step)
    out = Unprojected()
    with np.errstate(all="ignore"):
        z = depth.astype(F32) * F32(depth_scale)
        valid = np.isfinite(z) & (z > 0) & (near <= z) & (z <= far)
        if depth.dtype == np.uint16:
            valid &= depth != 0
        if mask is not None:
            valid &= np.asarray(mask) != 0
        u = np.arange(W, dtype=F32)[None, :]
        v = np.arange(H, dtype=F32)[:, None]
        P = np.stack([((u - cx) * z) / fx, ((v - cy) * z) / fy, z], -1)
        assert P.dtype == F32
        usable, Pn = {}, {}
        for key, (du, dv) in {"L": (-1, 0), "R": (1, 0), "U": (0, -1), "D": (0, 1)}.items():
            usable[key] = valid & _neighbour(valid, du, dv, False) & (np.abs(_neighbour(z, du, dv, F32(np.nan)) - z) <= step)
            Pn[key] = _neighbour(P, du, dv, F32(np.nan))

        def tangent(lo, hi):
            a = np.where(usable[hi][..., None], Pn[hi], P)
            b = np.where(usable[lo][..., None], Pn[lo], P)
            return (a - b).astype(np.float64), usable[lo] | usable[hi]

        (dx, has_dx), (dy, has_dy) = tangent("L", "R"), tangent("U", "D")
        c0 = dx[..., 1] * dy[..., 2] - dx[..., 2] * dy[..., 1]
        c1 = dx[..., 2] * dy[..., 0] - dx[..., 0] * dy[..., 2]
        c2 = dx[..., 0] * dy[..., 1] - dx[..., 1] * dy[..., 0]
        len2 = (c0 * c0 + c1 * c1) + c2 * c2
        known = valid & has_dx & has_dy & (len2 > 0)
        Pd = P.astype(np.float64)
        away = (c0 * Pd[..., 0] + c1 * Pd[..., 1]) + c2 * Pd[..., 2] > 0
        n = np.stack([c0, c1, c2], -1) / np.sqrt(len2)[..., None]
        n = np.where(away[..., None], -n, n)
        normal = np.where(known[..., None], n, 0.0).astype(F32)
    ui, vi = np.meshgrid(np.arange(W), np.arange(H))
    kept = valid & (ui % stride == 0) & (vi % stride == 0)
    if drop_isolated:
        kept &= known
    ku, kv = ui[kept], vi[kept]
    order = np.lexsort((z_rank(ku % TILE, kv % TILE), ku // TILE, kv // TILE))
    ku, kv = ku[order], kv[order]
    out.z, out.valid, out.P, out.usable, out.normal, out.known, out.kept = z, valid, P, usable, normal, known, kept
    out.points, out.normals = P[kv, ku], normal[kv, ku]
    out.pixel = (kv * W + ku).astype(np.int32)
    return out


def pack(refs, width=None):
    """A list of Unprojected -> (points [B, M, 3], normals [B, M, 3], pixel [B, M], counts [B]) as sh_depth_points pads them; M =
    width, or the largest count and at least 1."""
    counts = np.asarray([len(r.pixel) for r in refs], np.int32)
    M = max(int(counts.max()), 1) if width is None else width
    points, normals = np.zeros((len(refs), M, 3), F32), np.zeros((len(refs), M, 3), F32)
    pixel = np.full((len(refs), M), -1, np.int32)
    for b, r in enumerate(refs):
        points[b, :counts[b]], normals[b, :counts[b]], pixel[b, :counts[b]] = r.points, r.normals, r.pixel
    return points, normals, pixel, counts


# ------------------------------------------------------------------------------------------------ scenes
def rays(H, W, intr):
    """The pixel rays (x', y', 1), float64 [H, W, 3]."""
    fx, fy, cx, cy = (float(F32(v)) for v in intr)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)


def intrinsics_for(H, W):
    """A camera whose view the test scenes fill: focal length 1.2 max(H, W), the principal point off-centre and off-grid."""
    f = 1.2 * max(H, W)
    return (f, f * 1.05, 0.5 * (W - 1) + 0.25, 0.5 * (H - 1) - 0.125)


def fronto_plane(H, W, z0=2.0):
    return np.full((H, W), z0, F32)


def tilted_plane(H, W, intr, normal, through):
    """Depth of the plane normal . (P - through) = 0 along every pixel ray, float64 [H, W]."""
    n = np.asarray(normal, np.float64)
    return float(n @ np.asarray(through, np.float64)) / (rays(H, W, intr) @ n)


def sphere_over_plane(H, W, intr, centre=(0.02, -0.01, 1.5), radius=0.12, z_plane=2.0):
    """A sphere in front of a fronto-parallel plane -> (depth float32 [H, W], on_sphere bool [H, W]): a depth step of about
    z_plane - centre_z at the silhouette."""
    r, c = rays(H, W, intr), np.asarray(centre, np.float64)
    rr, rc = (r * r).sum(-1), r @ c
    disc = rc * rc - rr * (c @ c - radius * radius)
    hit = disc > 0
    t = (rc - np.sqrt(np.where(hit, disc, 0.0))) / rr
    return np.where(hit, t, z_plane).astype(F32), hit


HOLES = (0.0, np.nan, np.inf, -1.0, 9.0)          # zero, NaN, +inf, negative, outside Z_RANGE


def holes(depth, seed=0, every=8):
    """A copy with one pixel in `every` replaced by the HOLES values in turn, at seeded places; none when the image has fewer
    than `every` pixels."""
    out = np.array(depth, F32)
    flat = out.reshape(-1)
    where = np.random.default_rng(seed).permutation(flat.size)[:flat.size // every]
    flat[where] = np.resize(np.asarray(HOLES, F32), where.size)
    return out


def scene(H, W, seed=0):
    """The sphere-over-plane scene with holes at H x W -> (depth float32, intrinsics)."""
    intr = intrinsics_for(H, W)
    return holes(sphere_over_plane(H, W, intr)[0], seed), intr


def to_words(depth, scale=0.001):
    """A float depth image -> 16-bit words at `scale` metres per unit; anything not finite and in (0, 65.5) -> the word 0."""
    with np.errstate(all="ignore"):
        w = np.rint(depth.astype(np.float64) / scale)
    return np.where(np.isfinite(w) & (w > 0) & (w < 65536), w, 0).astype(np.uint16)
