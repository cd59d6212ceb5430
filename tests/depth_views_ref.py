"""Host reference of the rig form of the depth kernels (include/sh_kernels.h, "Depth views"), numpy only: tests/depth_ref.py per
view, then the header's transform one operation at a time - the point in float32, the normal in float64 from the reference's
normal BEFORE its rounding, which depth_ref keeps only rounded: its last step is restated here from the fields it does expose -
and the rows concatenated view-major with `view`, `view_first` and the padding."""
import numpy as np

from tests import depth_ref as R

F32 = np.float32


def random_rotation(rng):
    """A proper rotation, float64 [3, 3], uniform over SO(3) (a normalised quaternion)."""
    w, x, y, z = (lambda q: q / np.linalg.norm(q))(rng.standard_normal(4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def extrinsic(rng, spread=1.0):
    """A random rigid camera -> rig transform, float32 [3, 4] (the rotation orthonormal to float32's rounding)."""
    return np.concatenate([random_rotation(rng), spread * rng.standard_normal((3, 1))], 1).astype(F32)


def normal64(ref):
    """The float64 unit normal of every pixel of an `Unprojected` after its flip towards the camera, [H, W, 3] - depth_ref's own
    expressions up to (and without) the rounding to float32; rows where `ref.known` is False mean nothing."""
    P = ref.P
    Pn = {key: R._neighbour(P, du, dv, F32(np.nan)) for key, (du, dv) in {"L": (-1, 0), "R": (1, 0), "U": (0, -1), "D": (0, 1)}.items()}

    def tangent(lo, hi):
        a = np.where(ref.usable[hi][..., None], Pn[hi], P)
        b = np.where(ref.usable[lo][..., None], Pn[lo], P)
        return (a - b).astype(np.float64)

    with np.errstate(all="ignore"):
        dx, dy = tangent("L", "R"), tangent("U", "D")
        c0 = dx[..., 1] * dy[..., 2] - dx[..., 2] * dy[..., 1]
        c1 = dx[..., 2] * dy[..., 0] - dx[..., 0] * dy[..., 2]
        c2 = dx[..., 0] * dy[..., 1] - dx[..., 1] * dy[..., 0]
        len2 = (c0 * c0 + c1 * c1) + c2 * c2
        Pd = P.astype(np.float64)
        away = (c0 * Pd[..., 0] + c1 * Pd[..., 1]) + c2 * Pd[..., 2] > 0
        n = np.stack([c0, c1, c2], -1) / np.sqrt(len2)[..., None]
        n = np.where(away[..., None], -n, n)
    assert np.array_equal(np.where(ref.known[..., None], n, 0.0).astype(F32).view(np.int32), ref.normal.view(np.int32))   # depth_ref's last step, restated
    return n


def move(ref, ext):
    """One view's packed rows under ext float32 [3, 4] (or [12]) -> (points', normals') float32 [m, 3], the header's expressions."""
    e = np.asarray(ext, F32).reshape(3, 4)
    H, W = ref.z.shape
    v, u = ref.pixel // W, ref.pixel % W
    P, n, known = ref.points, normal64(ref)[v, u], ref.known[v, u]
    with np.errstate(all="ignore"):
        pts = np.stack([((e[i, 0] * P[:, 0] + e[i, 1] * P[:, 1]) + e[i, 2] * P[:, 2]) + e[i, 3] for i in range(3)], -1)
        assert pts.dtype == F32
        r = e[:, :3].astype(np.float64)
        nrm = np.stack([(r[i, 0] * n[:, 0] + r[i, 1] * n[:, 1]) + r[i, 2] * n[:, 2] for i in range(3)], -1)
    return pts, np.where(known[:, None], nrm, 0.0).astype(F32)


class Fused:
    """One body's reference: `points`, `normals` [m, 3] float32, `pixel` [m] int32, `view` [m] uint8, `view_first` [V + 1] int32,
    and `refs`, the per-view Unprojected (None for an absent view)."""


def unproject_views(depths, intrs, exts, masks=None, **options):
    """One body: depths [V] images, intrs [V] (or one) intrinsics, exts [V, 3, 4] / [V, 12] float32 (a NaN anywhere: the view is
    absent) -> Fused."""
    V = len(depths)
    intrs = [intrs] * V if np.ndim(intrs) == 1 else intrs
    out = Fused()
    out.refs, pts, nrm, pix, view, first = [], [], [], [], [], [0]
    for k in range(V):
        e = np.asarray(exts[k], F32).reshape(3, 4)
        if np.isnan(e).any():
            out.refs.append(None)
        else:
            ref = R.unproject(depths[k], intrs[k], mask=None if masks is None else masks[k], **options)
            p, n = move(ref, e)
            out.refs.append(ref)
            pts.append(p), nrm.append(n), pix.append(ref.pixel), view.append(np.full(len(ref.pixel), k, np.uint8))
        first.append(sum(len(p) for p in pix))
    out.points = np.concatenate(pts).astype(F32) if pts else np.zeros((0, 3), F32)
    out.normals = np.concatenate(nrm).astype(F32) if nrm else np.zeros((0, 3), F32)
    out.pixel = np.concatenate(pix).astype(np.int32) if pix else np.zeros(0, np.int32)
    out.view = np.concatenate(view) if view else np.zeros(0, np.uint8)
    out.view_first = np.asarray(first, np.int32)
    return out


def pack(bodies, width=None):
    """A list of Fused -> (points [B, M, 3], normals [B, M, 3], pixel [B, M], view [B, M], counts [B], view_first [B, V + 1]) as
    sh_depth_views_points pads them; M = width, or the largest count and at least 1."""
    counts = np.asarray([len(f.pixel) for f in bodies], np.int32)
    M = max(int(counts.max()), 1) if width is None else width
    B = len(bodies)
    points, normals = np.zeros((B, M, 3), F32), np.zeros((B, M, 3), F32)
    pixel, view = np.full((B, M), -1, np.int32), np.full((B, M), 255, np.uint8)
    for b, f in enumerate(bodies):
        c = counts[b]
        points[b, :c], normals[b, :c], pixel[b, :c], view[b, :c] = f.points, f.normals, f.pixel, f.view
    return points, normals, pixel, view, counts, np.stack([f.view_first for f in bodies])
