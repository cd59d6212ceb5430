"""Host reference for the visibility tests (numpy only, float64): the definition of include/sh_kernels.h, "Vertex visibility",
evaluated in blocks of 256 vertices so that nothing larger than 256 x nF ever exists, and a classification of every vertex by
how far its decision is from flipping.

With the Moeller-Trumbore quantities in normalised form (u, w, t divided by det) and ins = min(u, w, 1 - u - w, t, 1 - t) - the
signed margin by which the segment passes inside the face - a vertex is SURELY OCCLUDED when some face that does not name it has
ins >= DELTA, SURELY VISIBLE when every such face has ins <= -DELTA, AMBIGUOUS otherwise (a ray through an edge, along a
face's plane, or ending next to another vertex).  Only the sure vertices bind an fp32 evaluation.  The facing test is exempted
the same way: ambiguous when the cosine lies within DELTA of the bound.

Also here: the analytic scenes (icosphere, screen), viewpoints placed from a body's own extent, surface samples of the visible
faces, and the float64 ICP of tests/align_ref.py with a visibility mask per iteration."""
import numpy as np

from tests import align_ref as A
from tests import normals_ref as N

DELTA = 1e-4
VISIBLE, OCCLUDED, AMBIGUOUS = 0, 1, 2
ROWS = 256
# directions off the planes x = 0 and y = 0: rays from a viewpoint on a symmetry plane of the templates run along seam edges
DIRECTIONS = np.array([[-0.33, -0.9, 0.21], [0.55, 0.62, 0.56], [0.8, -0.35, -0.49]])


def _names(f, idx, n):
    """bool [len(idx), nF]: face names vertex idx[r]."""
    names = np.zeros((len(idx), f.shape[0]), bool)
    pos = np.full(n, -1, np.int64)
    pos[idx] = np.arange(len(idx))
    for k in range(3):
        r = pos[f[:, k]]
        sel = np.nonzero(r >= 0)[0]
        names[r[sel], sel] = True
    return names


def _classify(det, u, w, t, names):
    """From the Moeller-Trumbore quantities of a block [r, nF]: (largest ins per vertex over the faces that do not name it, any hit
    by the definition's test, taken on the normalised values: min(u, w, 1 - u - w) >= 0 and min(t, 1 - t) > 0).  A face parallel
    to the ray (det == 0) is no hit; its margin is -inf unless the ray lies in its plane, where it counts as 0 (ambiguous)."""
    if det.shape[1] == 0:
        return np.full(det.shape[0], -np.inf), np.zeros(det.shape[0], bool)
    flat = det == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (1.0 / det).astype(det.dtype)
        un, wn, tn = u * inv, w * inv, t * inv
        side = np.minimum(np.minimum(un, wn), 1 - un - wn)
        along = np.minimum(tn, 1 - tn)
    h = (side >= 0) & (along > 0)
    ins = np.minimum(side, along).astype(np.float64)
    if flat.any():
        h &= ~flat
        ins[flat] = np.where((u[flat] == 0) | (w[flat] == 0) | (t[flat] == 0), 0.0, -np.inf)
    ins[np.isnan(ins)] = 0.0
    ins[names] = -np.inf
    h &= ~names
    return ins.max(1), h.any(1)


def margins(x, faces, view, rows=ROWS, select=None):
    """For every vertex of x [n, 3] (or those listed in `select`, in that order): (best = the largest ins over the faces that do not name it, hit = whether the definition's
    test holds for one of them), float64.  The triple products are expanded into per-face and per-vertex vectors so that a block
    is four [rows, 3] x [3, nF] matrix products (with N = e1 x e2, c = o x v:  det = -d . N,  t = s . N,
    u = e2 . c - e2 . (a x v) + o . (e2 x a),  w = -e1 . c - e1 . (v x a) + o . (a x e1)); exact identities, and float64's rounding
    is ten orders below DELTA."""
    x = np.asarray(x, np.float64)
    v = np.asarray(view, np.float64)
    f = np.asarray(faces, np.int64)
    n = x.shape[0]
    a = x[f[:, 0]]
    e1, e2 = x[f[:, 1]] - a, x[f[:, 2]] - a
    nrm = np.cross(e1, e2)
    a_n = (a * nrm).sum(1)
    ku = (e2 * np.cross(a, v[None])).sum(1)
    kw = (e1 * np.cross(v[None], a)).sum(1)
    e2a, ae1 = np.cross(e2, a), np.cross(a, e1)
    select = np.arange(n) if select is None else np.asarray(select, np.int64)
    best, hit = np.full(len(select), -np.inf), np.zeros(len(select), bool)
    for lo in range(0, len(select), rows):
        hi = min(lo + rows, len(select))
        o = x[select[lo:hi]]
        c = np.cross(o, v[None])
        det = -((v[None] - o) @ nrm.T)
        t = o @ nrm.T - a_n[None]
        u = c @ e2.T - ku[None] + o @ e2a.T
        w = -(c @ e1.T) - kw[None] + o @ ae1.T
        best[lo:hi], hit[lo:hi] = _classify(det, u, w, t, _names(f, select[lo:hi], n))
    return best, hit


def margins_direct(x, faces, view, dtype=np.float64, rows=ROWS, select=None):
    """The same from the header's own sequence of differences, cross and dot products, every operation in `dtype` (numpy: no
    fused multiply-add) - what the host study compares between fp32 and fp64.  select as in `margins`."""
    x = np.asarray(x, dtype)
    view = np.asarray(view, dtype)
    f = np.asarray(faces, np.int64)
    select = np.arange(x.shape[0]) if select is None else np.asarray(select, np.int64)
    a = x[f[:, 0]]
    e1, e2 = x[f[:, 1]] - a, x[f[:, 2]] - a
    best, hit = np.full(len(select), -np.inf), np.zeros(len(select), bool)
    A, E1, E2 = (tuple(m[None, :, k] for k in range(3)) for m in (a, e1, e2))      # per component, [1, nF]

    def cross(u, v):
        return u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]

    def dot(u, v):
        return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]

    for lo in range(0, len(select), rows):
        hi = min(lo + rows, len(select))
        o = tuple(x[select[lo:hi], k][:, None] for k in range(3))                   # [r, 1]
        d = tuple(view[k] - o[k] for k in range(3))
        p = cross(d, E2)
        det = dot(E1, p)
        s = tuple(o[k] - A[k] for k in range(3))
        u = dot(s, p)
        q = cross(s, E1)
        w = dot(d, q)
        t = dot(E2, q)
        best[lo:hi], hit[lo:hi] = _classify(det, u, w, t, _names(f, select[lo:hi], x.shape[0]))
    return best, hit


def facing(x, tn, view, cos_g):
    """The facing test in float64: (passes, ambiguous) per vertex; a zero normal has cosine 0."""
    d = np.asarray(view, np.float64)[None, :] - np.asarray(x, np.float64)
    ln = np.sqrt((d * d).sum(1))
    cos = (np.asarray(tn, np.float64) * d).sum(1) / np.where(ln > 0, ln, 1.0)
    zero = np.abs(tn).sum(1) == 0
    amb = (np.abs(cos - cos_g) < DELTA) & ~(zero & (cos_g == 0.0))
    return cos >= cos_g, amb


def visibility(x, faces, view, mask=None, tn=None, cos_g=None, delta=DELTA, select=None):
    """(visible bool [n] by the definition in float64, cls int8 [n]: VISIBLE / OCCLUDED / AMBIGUOUS).  A masked vertex is surely
    not visible; a NaN viewpoint makes every active vertex surely visible.  select: an index array - only those vertices are
    judged (against ALL faces), and both results have its length and order."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    sel = np.arange(n) if select is None else np.asarray(select, np.int64)
    act = (np.ones(n, bool) if mask is None else np.asarray(mask, bool))[sel]
    if np.isnan(np.asarray(view, np.float64)).any():
        return act.copy(), np.where(act, VISIBLE, OCCLUDED).astype(np.int8)
    best, hit = margins(x, faces, view, select=sel)
    vis = act & ~hit
    cls = np.where(best >= delta, OCCLUDED, np.where(best <= -delta, VISIBLE, AMBIGUOUS)).astype(np.int8)
    if tn is not None:
        ok, amb = facing(x[sel], np.asarray(tn)[sel], view, cos_g)
        vis &= ok
        cls = np.where(~ok & ~amb, OCCLUDED, np.where(amb & (cls == VISIBLE), AMBIGUOUS, cls)).astype(np.int8)
    cls[~act] = OCCLUDED
    return vis, cls


def agree(got, vis, cls, cap=0.01):
    """The parity check of one body: the ambiguous share within the cap FIRST, then every surely-decided vertex equal to the
    reference.  -> the number of ambiguous vertices."""
    amb = cls == AMBIGUOUS
    assert amb.sum() <= cap * len(cls), "ambiguous %d of %d: over the %.0f %% cap" % (amb.sum(), len(cls), 100 * cap)
    sure = ~amb
    assert np.array_equal(np.asarray(got, bool)[sure], (cls == VISIBLE)[sure]), \
        "%d surely-decided vertices differ" % (np.asarray(got, bool)[sure] != (cls == VISIBLE)[sure]).sum()
    assert np.array_equal(vis[sure], (cls == VISIBLE)[sure])                # the reference agrees with itself
    return int(amb.sum())


def viewpoint(x, direction, distance=3.0):
    """centre + distance x extent x direction (normalised): a viewpoint placed from the body's own size."""
    x = np.asarray(x, np.float64)
    lo, hi = x.min(0), x.max(0)
    d = np.asarray(direction, np.float64)
    return (lo + hi) / 2 + distance * (hi - lo).max() * d / np.linalg.norm(d)


def outside(x, view):
    """Whether the viewpoint lies outside the body's bounding box by at least half its extent."""
    x = np.asarray(x, np.float64)
    lo, hi = x.min(0), x.max(0)
    gap = np.maximum(np.maximum(lo - view, view - hi), 0.0)
    return bool(np.linalg.norm(gap) >= 0.5 * (hi - lo).max())


# ------------------------------------------------------------------------------------------------ analytic scenes
def icosphere(level=2, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """A convex unit icosphere, `level` subdivisions: (verts float64 [n, 3], faces int64 [nF, 3]) wound counter-clockwise seen from
    outside.  level 2: 162 vertices, 320 faces."""
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius + np.asarray(centre, np.float64), np.asarray(f, np.int64)


def sphere_expected(verts, faces, view):
    """Convex body: a vertex is visible iff some incident face faces the sensor.  (visible, margin): margin = the largest
    (normal . (view - a)) / (|normal| |view - a|) over the vertex's faces - near 0 the vertex sits on the silhouette."""
    a, b, c = (verts[faces[:, k]] for k in range(3))
    nrm = np.cross(b - a, c - a)
    to = np.asarray(view, np.float64)[None] - a
    cos = (nrm * to).sum(1) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(to, axis=1))
    best = np.full(len(verts), -np.inf)
    for k in range(3):
        np.maximum.at(best, faces[:, k], cos)
    return best > 0, best


def screen_scene(level=2):
    """The sphere at the origin, the sensor on the +z side and between them a two-triangle screen covering x < 0 only:
    (verts [n + 4, 3], faces, view, n_sphere).  The screen's vertices are the last four."""
    v, f = icosphere(level)
    n = len(v)
    view = np.array([0.13, 0.07, 6.0])
    z = 2.5
    sv = np.array([[-3.0, -3.0, z], [-0.011, -3.0, z], [-0.011, 3.0, z], [-3.0, 3.0, z]])
    sf = np.array([[n, n + 1, n + 2], [n, n + 2, n + 3]])
    return np.concatenate([v, sv]), np.concatenate([f, sf]), view, n


def screen_expected(verts, view, n_sphere, z=2.5, edge=-0.011, clear=0.05):
    """Sphere vertices on the sensor's side: (in_shadow, in_light), each only where the ray crosses the screen's plane at least
    `clear` away from the screen's border."""
    o = verts[:n_sphere]
    d = view[None] - o
    t = (z - o[:, 2]) / d[:, 2]
    px = o[:, 0] + t * d[:, 0]
    py = o[:, 1] + t * d[:, 1]
    front = (o * d).sum(1) > 0.2 * np.linalg.norm(d, axis=1)                # well on the sensor's side of the silhouette
    shadow = front & (px < edge - clear) & (px > -3 + clear) & (np.abs(py) < 3 - clear)
    light = front & (px > edge + clear)
    return shadow, light


# ------------------------------------------------------------------------------------------------ partial scans and their ICP
def visible_samples(x, faces, vis, m, seed):
    """m points on the faces whose three corners are visible, area-weighted, float64 [m, 3]."""
    rs = np.random.RandomState(seed)
    f = faces[vis[faces].all(1)]
    a, b, c = (x[f[:, k]] for k in range(3))
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    k = rs.choice(len(f), size=m, p=area / area.sum())
    r1, r2 = np.sqrt(rs.rand(m, 1)), rs.rand(m, 1)
    return (1 - r1) * a[k] + r1 * (1 - r2) * b[k] + r1 * r2 * c[k]


def icp(x, faces, s, view, mode="similarity", iters=30, w_ms=1.0, visibility_on=True):
    """tests/align_ref.icp (float64, moment start, vertex pairs) with the mask of every iteration = the vertices visible from
    the viewpoint under the pose so far; visibility_on=False is align_ref.icp itself.  s, view in the scan's frame.  -> (A, t)."""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    P, t = A.moment_pose(s, x, mode == "similarity")
    m, n = len(s), len(x)
    for _ in range(iters):
        cur = A.apply(P, t, s)
        act = visibility(x, faces, A.apply(P, t, np.asarray(view, np.float64)[None])[0])[0] if visibility_on else np.ones(n, bool)
        live = np.nonzero(act)[0]
        j, d_sm = A.nearest(cur, x[live])
        i_sm = live[j]
        i_ms, d_ms = A.nearest(x, cur)
        p, q, w = A.pairs(cur, x, n, m, act, i_sm, d_sm.astype(np.float32), i_ms, d_ms.astype(np.float32), np.inf, w_ms)
        dA, dt, _, _ = A.umeyama(A.moments(p, q, w)[0], mode)
        P, t = A.compose(dA, dt, P, t)
    return P, t


def pose_error(P, t, P0, t0, pts):
    """RMS distance between the points under the two poses."""
    return float(np.sqrt(((A.apply(P, t, pts) - A.apply(P0, t0, pts)) ** 2).sum(1).mean()))


def template(name):
    return N.template(name)
