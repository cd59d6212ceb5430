"""Host reference of the depth field and of the free-space / silhouette term (include/sh_kernels.h, "Depth field"), numpy only:
classification and z in float32, the feature transform by brute force over all pixel pairs with the lexicographic key (and once
more in the two-pass form the kernel uses), the term and its gradient in float32 one operation at a time, a float64 restatement
of the term for the fit experiment, and a scene helper that renders a mesh to a depth image."""
import math

import numpy as np

F32 = np.float32
EMPTY, UNKNOWN, SURFACE = 0, 1, 2
NONE, FREE, SILHOUETTE, AT_UNKNOWN, OUTSIDE = 0, 1, 2, 3, 4


# ------------------------------------------------------------------------------------------------ the field
def classify(depth, depth_scale=1.0, mask=None, z_range=None):
    """depth [H, W] float32 or uint16 -> (cls uint8 [H, W], z float32 [H, W])."""
    depth = np.asarray(depth)
    assert depth.ndim == 2 and depth.dtype in (np.float32, np.uint16)
    near, far = (F32(-np.inf), F32(np.inf)) if z_range is None else (F32(z_range[0]), F32(z_range[1]))
    with np.errstate(all="ignore"):
        z = depth.astype(F32) * F32(depth_scale)
        reading = np.isfinite(z) & (z > 0)
        if depth.dtype == np.uint16:
            reading &= depth != 0
        valid = reading & (near <= z) & (z <= far)
        if mask is not None:
            valid &= np.asarray(mask) != 0
        empty = reading & ~valid & (z >= near)
    cls = np.where(valid, SURFACE, np.where(empty, EMPTY, UNKNOWN)).astype(np.uint8)
    return cls, np.where(valid, z, F32(0)).astype(F32)


def nearest_brute(cls):
    """The feature transform of cls != 0 by brute force: per pixel the minimum of (d2, v' * W + u') over every allowed pixel."""
    H, W = cls.shape
    av, au = np.nonzero(cls != EMPTY)                                      # row-major: ascending index
    out = np.full((H, W), -1, np.int32)
    if av.size == 0:
        return out
    index = (av * W + au).astype(np.int64)
    u = np.arange(W, dtype=np.int64)
    for v in range(H):
        d2 = (u[:, None] - au[None, :]) ** 2 + (v - av[None, :]) ** 2      # [W, allowed]
        out[v] = index[np.argmin(d2, axis=1)]                              # the first minimum: the smallest index
    return out


def column_candidates(cls):
    """The column pass: per pixel the row of the nearest allowed pixel of its own column, a tie between up and down to up; -1
    for a column without one."""
    H, W = cls.shape
    allowed = cls != EMPTY
    cand = np.full((H, W), -1, np.int64)
    for u in range(W):
        up, above = -1, np.full(H, -1, np.int64)
        for v in range(H):
            up = v if allowed[v, u] else up
            above[v] = up
        down = -1
        for v in range(H - 1, -1, -1):
            down = v if allowed[v, u] else down
            a = above[v]
            cand[v, u] = a if a >= 0 and (down < 0 or v - a <= down - v) else down
    return cand


def nearest_two_pass(cls):
    """The two-pass form: the column candidates, then per pixel the lexicographic minimum of (d2, v', u') over the columns."""
    H, W = cls.shape
    cand = column_candidates(cls)
    out = np.full((H, W), -1, np.int32)
    u = np.arange(W, dtype=np.int64)
    for v in range(H):
        r = cand[v]
        if (r < 0).all():
            continue
        d2 = np.where(r >= 0, (v - r) ** 2, 1 << 30)[None, :] + (u[:, None] - u[None, :]) ** 2
        key = (d2 << 32) | np.where(r >= 0, r * W + u, 0)[None, :]
        out[v] = (key.min(axis=1) & 0xffffffff).astype(np.int32)
    return out


class Field:
    """One image's reference: cls, z, nearest [H, W] and intr (fx, fy, cx, cy) float32."""

    def __init__(self, cls, z, nearest, intr):
        self.cls, self.z, self.nearest, self.intr = cls, z, nearest, np.asarray(intr, F32)


def field(depth, intr, depth_scale=1.0, mask=None, z_range=None):
    cls, z = classify(depth, depth_scale, mask, z_range)
    return Field(cls, z, nearest_brute(cls), intr)


def field_of_classes(cls, intr, z=None):
    """A field with the classes given (the tests' constructed masks); z: the surface depth where cls is SURFACE."""
    cls = np.asarray(cls, np.uint8)
    zz = np.zeros(cls.shape, F32) if z is None else np.where(cls == SURFACE, np.asarray(z, F32), F32(0)).astype(F32)
    return Field(cls, zz, nearest_brute(cls), intr)


# ------------------------------------------------------------------------------------------------ the term, float32
def project(x, intr, H, W):
    """The header's projection of float32 points [n, 3] -> (uf, vf, inside, u, v); u, v are 0 where not inside."""
    X, Y, Z = (np.ascontiguousarray(x[:, k], F32) for k in range(3))
    fx, fy, cx, cy = (F32(t) for t in intr)
    with np.errstate(all="ignore"):
        front = Z > 0
        uf = (X * fx) / Z + cx
        vf = (Y * fy) / Z + cy
        inside = front & (uf >= F32(-0.5)) & (uf < F32(W) - F32(0.5)) & (vf >= F32(-0.5)) & (vf < F32(H) - F32(0.5))
        u = np.where(inside, np.floor(uf + F32(0.5)), 0).astype(np.int64)
        v = np.where(inside, np.floor(vf + F32(0.5)), 0).astype(np.int64)
    assert uf.dtype == F32
    return uf, vf, inside, u, v


def terms(x, n, f, v_mask=None, margin=0.0):
    """One body: x float32 [rows, 3], f a Field -> (term float32 [n], kind uint8 [n], g float32 [n, 3] (not yet scaled), counts
    int [4] = (active, kind 1, kind 2, kind 4))."""
    H, W = f.cls.shape
    x = np.asarray(x, F32)[:n]
    active = np.ones(n, bool) if v_mask is None else np.asarray(v_mask)[:n] != 0
    X, Y, Z = (np.ascontiguousarray(x[:, k]) for k in range(3))
    fx, fy, cx, cy = (F32(t) for t in f.intr)
    _, _, inside, u, v = project(x, f.intr, H, W)
    c = f.cls[v, u]
    kind = np.full(n, NONE, np.uint8)
    term, g = np.zeros(n, F32), np.zeros((n, 3), F32)
    kind[active & ~inside] = OUTSIDE
    kind[active & inside & (c == UNKNOWN)] = AT_UNKNOWN
    with np.errstate(all="ignore"):
        e = (f.z[v, u] - F32(margin)) - Z
        free = active & inside & (c == SURFACE) & (e > 0)
        kind[free] = FREE
        term[free] = (e * e)[free]
        g[free, 2] = (F32(-2) * e)[free]
        q = f.nearest[v, u].astype(np.int64)
        sil = active & inside & (c == EMPTY) & (q >= 0)
        uq, vq = q % W, q // W
        a = (uq.astype(F32) - cx) / fx
        b = (vq.astype(F32) - cy) / fy
        rx = X - a * Z
        ry = Y - b * Z
        kind[sil] = SILHOUETTE
        term[sil] = (rx * rx + ry * ry)[sil]
        g[sil, 0] = (F32(2) * rx)[sil]
        g[sil, 1] = (F32(2) * ry)[sil]
        g[sil, 2] = (F32(-2) * (a * rx + b * ry))[sil]
    assert term.dtype == F32 and g.dtype == F32 and e.dtype == F32 and rx.dtype == F32
    counts = np.asarray([active.sum(), (kind == FREE).sum(), (kind == SILHOUETTE).sum(), (kind == OUTSIDE).sum()], np.int32)
    return term, kind, g, counts


def losses(term, kind, counts):
    """(free, silhouette) of one body as exact sums (math.fsum) divided by n_act, float64."""
    if counts[0] == 0:
        return 0.0, 0.0
    return (math.fsum(term[kind == FREE].astype(np.float64)) / int(counts[0]),
            math.fsum(term[kind == SILHOUETTE].astype(np.float64)) / int(counts[0]))


def gradient(kind, g, counts, gL, rows):
    """g_x float32 [rows, 3] of one body: fl(fl(gL[k] * fl(1 / n_act)) * g) per component, zeros elsewhere."""
    out = np.zeros((rows, 3), F32)
    if counts[0] == 0:
        return out
    inv = F32(1) / F32(int(counts[0]))
    with np.errstate(all="ignore"):
        for k, what in ((0, FREE), (1, SILHOUETTE)):
            s = F32(gL[k]) * inv
            rows_k = np.nonzero(kind == what)[0]
            out[rows_k] = s * g[rows_k]
    assert out.dtype == F32
    return out


def edge_rows(f):
    """Camera-frame vertices of field f on which taking a vertex as it is and carrying it through an identity map part ways: M x
    with M = I multiplies Z = +inf or X = -inf by the zeros of the other rows (0 * inf: a NaN, kind 4 where the case list has
    another answer), and M^T w added to 0 turns a gradient word -0 into +0.  Z = +inf projects onto the principal point's pixel
    whatever X and Y are; the last row stands in front of that pixel's column with X = -0: where the pixel is SURFACE its term is
    of kind 1 with g = (0, 0, -2 e), and a negative gL makes the first two words -0."""
    fx, fy, cx, cy = (float(t) for t in f.intr)
    v0 = math.floor(float(F32(cy) + F32(0.5)))
    near = 2.0 ** -3
    return np.asarray([[0.25, -0.125, np.inf], [-np.inf, 0.1, 2.0], [np.nan, 0.1, 2.0], [-0.0, (v0 - cy) / fy * near, near]], F32)


def edge_fields():
    """Three 17 x 33 fields whose principal point's pixel, (u, v) = (15, 9), is of each class -> {name: Field}: "surface" all
    SURFACE, "empty" EMPTY around the principal point with allowed pixels beyond, "none" EMPTY everywhere (no allowed pixel)."""
    H, W, intr = 17, 33, (32.0, 16.0, 15.25, 8.5)
    z = 1.5 + 0.01 * np.random.default_rng(2).standard_normal((H, W))
    surface = np.full((H, W), SURFACE, np.uint8)
    empty = surface.copy()
    empty[7:12, 13:18] = EMPTY
    return {"surface": field_of_classes(surface, intr, z), "empty": field_of_classes(empty, intr, z),
            "none": field_of_classes(np.zeros((H, W), np.uint8), intr)}


# ------------------------------------------------------------------------------------------------ the term, float64
def terms64(x, n, f, v_mask=None, margin=0.0):
    """The term restated in float64: the same pixel rule (projection and rounding to a pixel in float64), the same cases -> (free
    [n], silhouette [n]) float64 per vertex, zero where there is no term, and the number of active vertices."""
    H, W = f.cls.shape
    x = np.asarray(x, np.float64)[:n]
    active = np.ones(n, bool) if v_mask is None else np.asarray(v_mask)[:n] != 0
    fx, fy, cx, cy = (float(t) for t in f.intr)
    X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
    with np.errstate(all="ignore"):
        uf, vf = X * fx / Z + cx, Y * fy / Z + cy
        inside = active & (Z > 0) & (uf >= -0.5) & (uf < W - 0.5) & (vf >= -0.5) & (vf < H - 0.5)
        u = np.where(inside, np.floor(uf + 0.5), 0).astype(np.int64)
        v = np.where(inside, np.floor(vf + 0.5), 0).astype(np.int64)
        c = f.cls[v, u]
        e = f.z[v, u].astype(np.float64) - float(margin) - Z
        free = np.where(inside & (c == SURFACE) & (e > 0), e * e, 0.0)
        q = f.nearest[v, u].astype(np.int64)
        a, b = ((q % W) - cx) / fx, ((q // W) - cy) / fy
        rx, ry = X - a * Z, Y - b * Z
        sil = np.where(inside & (c == EMPTY) & (q >= 0), rx * rx + ry * ry, 0.0)
    return free, sil, int(active.sum())


def losses64(x, n, f, v_mask=None, margin=0.0):
    free, sil, n_act = terms64(x, n, f, v_mask, margin)
    return (math.fsum(free) / n_act, math.fsum(sil) / n_act) if n_act else (0.0, 0.0)


# ------------------------------------------------------------------------------------------------ scenes
def tie_masks():
    """The constructed class images of the tests -> {name: cls uint8 [H, W]} (0 EMPTY, 2 allowed)."""
    out = {}
    c = np.zeros((5, 5), np.uint8)
    c[0, 0] = c[0, 4] = c[4, 0] = c[4, 4] = SURFACE
    out["corners"] = c                                                     # the centre: four at d2 = 8, the smallest index is 0
    c = np.zeros((7, 9), np.uint8)
    c[5, 6] = SURFACE
    out["single"] = c
    out["none"] = np.zeros((6, 7), np.uint8)
    out["all"] = np.full((4, 6), SURFACE, np.uint8)
    c = np.zeros((13, 13), np.uint8)                                       # (u, v) = (6, 6): below at 5 and left at 5 tie at d2 = 25;
    c[11, 6] = c[6, 1] = UNKNOWN                                           # the left one, in the pixel's own row, has the smaller index
    out["row_tie"] = c                                                     # and is met only at k = 5, when k * k == the best d2
    c = np.zeros((11, 3), np.uint8)
    c[2, 1] = c[8, 1] = SURFACE                                            # (1, 5): up and down tie in the column pass
    out["column_tie"] = c
    return out


def camera_for(vertices, H, W, fill=0.8, distance=2.5):
    """A camera that sees a body [n, 3] along the axis of its smallest extent, its largest extent upright in the image and
    spanning `fill` of the image's height from `distance` times that extent away -> (Rm [3, 3] a proper rotation, t [3],
    intr, the largest extent): camera-frame points are vertices @ Rm.T + t."""
    v = np.asarray(vertices, np.float64)
    lo, hi = v.min(0), v.max(0)
    order = np.argsort(hi - lo)                                            # smallest, middle, largest extent
    Rm = np.zeros((3, 3))
    Rm[0, order[1]], Rm[1, order[2]], Rm[2, order[0]] = 1.0, -1.0, 1.0
    if np.linalg.det(Rm) < 0:
        Rm[0] = -Rm[0]
    size = float((hi - lo).max())
    t = -Rm @ ((lo + hi) / 2) + np.asarray([0.0, 0.0, distance * size])
    f = fill * H * distance
    return Rm, t, (f, f, 0.5 * (W - 1) + 0.25, 0.5 * (H - 1) - 0.125), size


def render(vertices, faces, intr, H, W, background, samples=12):
    """A mesh seen by the camera at the origin looking along +z -> depth float32 [H, W]: dense barycentric samples of every face
    (a grid of `samples` steps along two edges), each projected to its nearest pixel, the minimum depth per pixel; `background` where no
    sample lands."""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    fx, fy, cx, cy = (float(F32(t)) for t in intr)
    i, j = np.meshgrid(np.arange(samples + 1), np.arange(samples + 1), indexing="ij")
    keep = i + j <= samples
    w1, w2 = i[keep] / samples, j[keep] / samples
    w0 = 1.0 - w1 - w2
    P = (w0[None, :, None] * v[f[:, 0]][:, None, :] + w1[None, :, None] * v[f[:, 1]][:, None, :]
         + w2[None, :, None] * v[f[:, 2]][:, None, :]).reshape(-1, 3)
    P = P[P[:, 2] > 0]
    pu = np.floor(P[:, 0] * fx / P[:, 2] + cx + 0.5).astype(np.int64)
    pv = np.floor(P[:, 1] * fy / P[:, 2] + cy + 0.5).astype(np.int64)
    ok = (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
    depth = np.full(H * W, np.inf)
    np.minimum.at(depth, pv[ok] * W + pu[ok], P[ok, 2])
    return np.where(np.isfinite(depth), depth, background).astype(F32).reshape(H, W)
