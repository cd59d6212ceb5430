"""Host references for the point-to-surface tests (numpy only): the region test of include/sh_kernels.h ("Nearest surface
points") in float64 and transcribed to fp32 operation by operation, the exhaustive closest-point search built on either, the
float64 gradient formula of the surface Chamfer term, and the seeded surface samples the tests share."""
import numpy as np

from tests.scan_ref import fma32

# ---------------------------------------------------------------------------------------------- measured constants
# Foot-point error of the header's fp32 expression against float64, as a multiple of 2^-24 * max|coordinate|, over exactly the
# inputs of tests/test_surface.py::test_against_float64 (host code only, no kernel):
#     python -m tests.surface_ref
# prints "delta multiple: max ..." and "gradient: max ..."; the two constants below are those maxima, rounded up.  The kernel is
# given four times each (fma contraction and the order of the cross terms may differ).
F32_DELTA_MULTIPLE = 1.01
F32_GRAD_REL = 1.3e-6
KERNEL_FACTOR = 4.0
TIE = 1e-6            # medial-axis rule: best and second-best DISTINCT foot point closer than this (in distance) -> left out
TIE_CAP = 0.01        # share of points the rule may leave out


def _dot(u, v, f32):
    if f32:
        return fma32(u[..., 2], v[..., 2], fma32(u[..., 1], v[..., 1], u[..., 0] * v[..., 0]))
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def foot(a, b, c, s, f32=False):
    """The header's region test for broadcastable corners a, b, c and points s [..., 3] -> (v, w, d2): the weights of b and c and
    the squared distance, in float64, or in fp32 with every operation rounded as the header states (f32=True)."""
    dt = np.float32 if f32 else np.float64
    a, b, c, s = (np.asarray(t, dt) for t in (a, b, c, s))
    one, zero = dt(1), dt(0)
    ab, ac = b - a, c - a
    ap = s - a
    e11, e12, e22 = _dot(ab, ab, f32), _dot(ab, ac, f32), _dot(ac, ac, f32)
    d1, d2 = _dot(ab, ap, f32), _dot(ac, ap, f32)
    d3, d4, d5, d6 = d1 - e11, d2 - e12, d1 - e12, d2 - e22
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        total = (va + vb) + vc
        den = np.where(total > 0, one / np.where(total > 0, total, one), zero)
        v, w = vb * den, vc * den
        den_bc, den_ac, den_ab = e43 + e56, d2 - d6, d1 - d3

        def quot(num, d):
            return np.where(d > 0, num / np.where(d > 0, d, one), zero)

        r6 = (va <= 0) & (e43 >= 0) & (e56 >= 0) & (den_bc > 0)
        w6 = quot(e43, den_bc)
        v, w = np.where(r6, one - w6, v), np.where(r6, w6, w)
        r5 = (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (den_ac > 0)
        v, w = np.where(r5, zero, v), np.where(r5, quot(d2, den_ac), w)
        r4 = (d6 >= 0) & (d5 <= d6)
        v, w = np.where(r4, zero, v), np.where(r4, one, w)
        r3 = (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (den_ab > 0)
        v, w = np.where(r3, quot(d1, den_ab), v), np.where(r3, zero, w)
        r2 = (d3 >= 0) & (d4 <= d3)
        v, w = np.where(r2, one, v), np.where(r2, zero, w)
        r1 = (d1 <= 0) & (d2 <= 0)
        v, w = np.where(r1, zero, v), np.where(r1, zero, w)
    v = np.minimum(np.maximum(v, zero), one).astype(dt)
    w = np.minimum(np.maximum(w, zero), one - v).astype(dt)
    if f32:
        r = [ap[..., k] - fma32(w, ac[..., k], v * ab[..., k]) for k in range(3)]
        dd = fma32(r[2], r[2], fma32(r[1], r[1], r[0] * r[0]))
    else:
        r = [ap[..., k] - (w * ac[..., k] + v * ab[..., k]) for k in range(3)]
        dd = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    return v, w, dd


def region_of(v, w):
    """0 interior, 1 / 2 / 3 edge ab / bc / ca, 4 / 5 / 6 vertex a / b / c (csrc_host/preprocess.cpp's convention)."""
    u = 1.0 - v - w
    z = lambda t: np.abs(t) < 1e-14
    return np.select([z(v) & z(w), z(u) & z(w), z(u) & z(v), z(w), z(u), z(v)], [4, 5, 6, 1, 2, 3], 0)


def _closest(q, verts, faces, allowed, f32, cells=1 << 19):
    dt = np.float32 if f32 else np.float64
    q, verts = np.asarray(q, dt), np.asarray(verts, dt)
    faces = np.asarray(faces, np.int64)
    nq, nF = q.shape[0], faces.shape[0]
    ok = np.ones(nF, bool) if allowed is None else np.asarray(allowed, bool)[faces].all(1)
    best = np.full(nq, np.inf, dt)
    bi = np.full(nq, -1, np.int64)
    bv, bw = np.zeros(nq, dt), np.zeros(nq, dt)
    fb = min(nF, 512) or 1
    qb = max(1, cells // fb)
    A, Bc, Cc = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    for q0 in range(0, nq, qb):
        qs = q[q0:q0 + qb, None, :]
        r = np.arange(qs.shape[0])
        sl = slice(q0, q0 + qb)
        for lo in range(0, nF, fb):
            v, w, d = foot(A[None, lo:lo + fb], Bc[None, lo:lo + fb], Cc[None, lo:lo + fb], qs, f32)
            d = np.where(ok[None, lo:lo + fb], d, dt(np.inf))
            k = d.argmin(1)                                                # the lowest face of the block on a tie
            dk = d[r, k]
            take = dk < best[sl]                                           # strict: an earlier block's face wins a tie
            best[sl] = np.where(take, dk, best[sl])
            bi[sl] = np.where(take, lo + k, bi[sl])
            bv[sl], bw[sl] = np.where(take, v[r, k], bv[sl]), np.where(take, w[r, k], bw[sl])
    return bi, best, np.stack([bv, bw], 1)


def closest_f64(q, verts, faces, allowed=None):
    """Exhaustive float64 search: (face - lowest on a tie, d2, uv [nq, 2]) per point; `allowed` [n] bool marks the active vertices
    (a triangle with an inactive corner is no target).  No target: face -1, d2 inf."""
    return _closest(q, verts, faces, allowed, False)


def closest_f32(q, verts, faces, allowed=None):
    """The kernel's answer computed on the host: the header's fp32 expression, lexicographic minimum of (d2, face)."""
    return _closest(q, verts, faces, allowed, True)


def rebuild_f64(verts, faces, face, uv):
    """The foot points of (face, uv) in float64: a + l1 (b - a) + l2 (c - a)."""
    verts = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)[np.asarray(face, np.int64)]
    a, b, c = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    uv = np.asarray(uv, np.float64)
    return a + uv[:, 0:1] * (b - a) + uv[:, 1:2] * (c - a)


def tie_mask_f64(q, verts, faces, face, uv, d2, allowed=None, cells=1 << 19):
    """True for the points the medial-axis rule leaves out: some triangle's foot point is DISTINCT from the best one and its
    distance is within TIE of the best distance.  Distinct: two foot points a distance e apart on one smooth piece of surface
    (the foot point inside a face near an edge, and the neighbour's foot point on that edge) are the same local minimum; their
    distances differ by about e^2 / (2 dist).  So a foot point counts as another one when e^2 > 8 TIE dist + TIE^2, four times
    what that effect explains at a difference of TIE.  float64, exhaustive."""
    q, verts = np.asarray(q, np.float64), np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    nq, nF = q.shape[0], faces.shape[0]
    ok = np.ones(nF, bool) if allowed is None else np.asarray(allowed, bool)[faces].all(1)
    fstar = rebuild_f64(verts, faces, face, uv)
    dist = np.sqrt(d2)
    out = np.zeros(nq, bool)
    fb = min(nF, 512) or 1
    qb = max(1, cells // fb)
    A, Bc, Cc = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    for q0 in range(0, nq, qb):
        qs = q[q0:q0 + qb, None, :]
        sl = slice(q0, q0 + qb)
        for lo in range(0, nF, fb):
            a, b, c = A[None, lo:lo + fb], Bc[None, lo:lo + fb], Cc[None, lo:lo + fb]
            v, w, d = foot(a, b, c, qs)
            p = a + v[..., None] * (b - a) + w[..., None] * (c - a)
            far = ((p - fstar[sl, None, :]) ** 2).sum(-1) > 8.0 * TIE * dist[sl, None] + TIE * TIE
            near = np.sqrt(d) - dist[sl, None] < TIE
            out[sl] |= (far & near & ok[None, lo:lo + fb]).any(1)
    return out


def surface_grad_f64(s, verts, faces, face, uv, keep, rows, m):
    """d/dx of (1/m) sum_{j kept} |s_j - q_j|^2 with q_j = sum_k l_k x[face_j[k]], the weights constant: corner k of the recorded
    face gets -2 l_k (s_j - q_j) / m.  float64 [rows, 3]."""
    verts = np.asarray(verts, np.float64)
    g = np.zeros((rows, 3))
    j = np.nonzero(keep)[0]
    f = np.asarray(faces, np.int64)[np.asarray(face, np.int64)[j]]
    uvj = np.asarray(uv, np.float64)[j]
    r = np.asarray(s, np.float64)[j] - rebuild_f64(verts, faces, np.asarray(face)[j], uvj)
    l = np.stack([1.0 - uvj[:, 0] - uvj[:, 1], uvj[:, 0], uvj[:, 1]], 1)
    for k in range(3):
        np.add.at(g, f[:, k], (-2.0 / m) * l[:, k:k + 1] * r)
    return g


def sample_surface(verts, faces, m, seed, sigma=0.0):
    """m points drawn uniformly by area on the triangles (seeded), plus Gaussian noise sigma, rounded to float32."""
    rs = np.random.RandomState(seed)
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    f = rs.choice(faces.shape[0], size=int(m), p=area / area.sum())
    r1, r2 = np.sqrt(rs.rand(int(m))), rs.rand(int(m))
    p = (1 - r1)[:, None] * a[f] + (r1 * (1 - r2))[:, None] * b[f] + (r1 * r2)[:, None] * c[f]
    if sigma:
        p = p + sigma * rs.randn(int(m), 3)
    return p.astype(np.float32)


def delta_bound(d2_64, delta):
    """|d2 - d2_64| allowed for a foot point displaced by at most delta: 2 sqrt(d2_64) delta + delta^2."""
    return 2.0 * np.sqrt(d2_64) * delta + delta * delta


def case_inputs(template, B, M, masked, kind, seed=3):
    """The inputs of one case of the GPU tests: model bodies x [B, n + 1, 3] float32 (synth_batch), the face table, ragged clouds
    and the vertex mask.  kind: "s0" / "s01" - samples of body (b + 1) % B's surface with noise 0 / 0.01; "far" - the same
    samples scaled by 3 about the origin (the nearest-vertex bound is loose)."""
    import os
    from semantichuman_amd.hierarchy import load_hierarchy
    from tests import scan_ref
    h = load_hierarchy(os.path.join(os.path.dirname(__file__), "golden", template))
    v, faces = np.asarray(h.verts, np.float64), np.asarray(h.faces, np.int64)
    n = v.shape[0]
    x = scan_ref.model_points(v, B, seed=seed)
    counts = [max(1, (M * (B - b)) // B - (b % 3)) if b else M for b in range(B)]
    clouds = []
    for b, m in enumerate(counts):
        src = x[(b + 1) % B, :n]
        p = sample_surface(src, faces, m, seed=1000 * seed + 17 * b + M, sigma={"s0": 0.0, "s01": 0.01, "far": 0.0}[kind])
        clouds.append((p * np.float32(3.0)) if kind == "far" else p)
    vmask = (np.random.RandomState(7).rand(n) < 0.7) if masked else None
    return x, faces, n, counts, clouds, vmask


FLOAT64_CASES = [(t, B, M, masked, kind) for t in ("template6890.npz", "small_ae.npz") for (B, M) in ((1, 1), (3, 63), (3, 1000))
                 for masked in (False, True) for kind in ("s0", "s01", "far")]


def grad_inputs():
    """The inputs of the GPU gradient test: three synth_batch bodies of the 6890-vertex template, noisy samples (sigma 0.01) of
    body (b + 1) % 3's surface, a vertex mask."""
    import os
    from semantichuman_amd.hierarchy import load_hierarchy
    from tests import scan_ref
    h = load_hierarchy(os.path.join(os.path.dirname(__file__), "golden", "template6890.npz"))
    v, faces = np.asarray(h.verts, np.float64), np.asarray(h.faces, np.int64)
    n = v.shape[0]
    x = scan_ref.model_points(v, 3, seed=3)
    counts = [2000, 1001, 277]
    clouds = [sample_surface(x[(b + 1) % 3, :n], faces, m, seed=21 + b, sigma=0.01) for b, m in enumerate(counts)]
    vmask = np.random.RandomState(2).rand(n) < 0.8
    return x, faces, n, counts, clouds, vmask


def _measure():
    """Prints the constants above (see the top of the file)."""
    worst = 0.0
    for (t, B, M, masked, kind) in FLOAT64_CASES:
        x, faces, n, counts, clouds, vmask = case_inputs(t, B, M, masked, kind)
        for b in range(B):
            s, xb = clouds[b], x[b, :n]
            f64, d64, uv64 = closest_f64(s, xb, faces, vmask)
            f32, d32, uv32 = closest_f32(s, xb, faces, vmask)
            scale = 2.0 ** -24 * max(np.abs(xb).max(), np.abs(s).max())
            d32 = d32.astype(np.float64)
            # the smallest delta that satisfies |d2_32 - d2_64| <= 2 sqrt(d2_64) delta + delta^2, and the same for (b)
            delta = -np.sqrt(d64) + np.sqrt(d64 + np.abs(d32 - d64))
            d_re = ((s.astype(np.float64) - rebuild_f64(xb, faces, f32, uv32)) ** 2).sum(1)
            delta2 = -np.sqrt(d32) + np.sqrt(d32 + np.abs(d_re - d32))
            worst = max(worst, delta.max() / scale, delta2.max() / scale)
        print("%s B=%d M=%d masked=%d %s: delta multiple so far %.3f" % (t, B, M, masked, kind, worst), flush=True)
    print("delta multiple: max %.3f" % worst, flush=True)
    x, faces, n, counts, clouds, vmask = grad_inputs()
    gworst = 0.0
    for b, m in enumerate(counts):
        s, xb = clouds[b], x[b, :n]
        f64, d64, uv64 = closest_f64(s, xb, faces, vmask)
        f32, d32, uv32 = closest_f32(s, xb, faces, vmask)
        keep = ~tie_mask_f64(s, xb, faces, f64, uv64, d64, vmask)
        g64 = surface_grad_f64(s, xb, faces, f64, uv64, keep, n, m)
        g32 = surface_grad_f64(s, xb.astype(np.float32), faces, f32, uv32, keep, n, m)
        gworst = max(gworst, np.abs(g32 - g64).max() / np.abs(g64).max())
        print("gradient body %d: %d of %d left out, rel so far %.3g" % (b, int((~keep).sum()), m, gworst), flush=True)
    print("gradient: max %.3g" % gworst, flush=True)


if __name__ == "__main__":
    _measure()
