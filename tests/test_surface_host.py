"""Point-to-surface fitting, the part that needs no GPU: the float64 reference against constructions with known answers, the
gradient formula against central differences, what the feature is for (the vertex objective's floor on on-surface samples),
FaceTable validation, the spatial order of ScanBatch, and the new symbols of the built library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, scan
from semantichuman_amd.hierarchy import load_hierarchy
from tests import scan_ref
from tests import surface_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_reference_recovers_constructed_foot_points():
    """Points built as q + t * normal above the interior, beyond an edge (pushed outwards in the plane as well) and beyond a
    vertex of an isolated triangle: the exhaustive float64 search recovers q, the region and t^2 (+ the in-plane offset)."""
    rs = np.random.RandomState(0)
    verts = np.array([[0.3, -0.2, 0.1], [1.4, 0.1, -0.3], [0.2, 1.1, 0.5], [9.0, 9.0, 9.0], [9.5, 9.0, 9.0], [9.0, 9.5, 9.0]])
    faces = np.array([[3, 4, 5], [0, 1, 2]])                              # the triangle under test is face 1; face 0 is far away
    a, b, c = verts[0], verts[1], verts[2]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm)
    pts, foots, regions, d2s = [], [], [], []
    for _ in range(200):
        t = rs.uniform(-0.5, 0.5)
        l = rs.dirichlet([1, 1, 1])
        q = l[0] * a + l[1] * b + l[2] * c                                # interior
        pts.append(q + t * nrm); foots.append(q); regions.append(0); d2s.append(t * t)
        for (p0, p1, opp, reg) in ((a, b, c, 1), (b, c, a, 2), (c, a, b, 3)):
            u = rs.uniform(0.05, 0.95)
            q = p0 + u * (p1 - p0)
            e = p1 - p0
            out = np.cross(e, nrm)
            out /= np.linalg.norm(out)
            if np.dot(out, opp - p0) > 0:
                out = -out
            k = rs.uniform(0.01, 0.4)
            pts.append(q + k * out + t * nrm); foots.append(q); regions.append(reg); d2s.append(k * k + t * t)
        for (p0, o1, o2, reg) in ((a, b, c, 4), (b, c, a, 5), (c, a, b, 6)):
            d = -((o1 - p0) / np.linalg.norm(o1 - p0) + (o2 - p0) / np.linalg.norm(o2 - p0))   # into the vertex's own cone
            d /= np.linalg.norm(d)
            k = rs.uniform(0.01, 0.4)
            pts.append(p0 + k * d + t * nrm); foots.append(p0); regions.append(reg); d2s.append(k * k + t * t)
    pts, foots, regions, d2s = np.array(pts), np.array(foots), np.array(regions), np.array(d2s)
    face, d2, uv = R.closest_f64(pts, verts, faces)
    assert (face == 1).all()
    assert np.abs(R.rebuild_f64(verts, faces, face, uv) - foots).max() < 1e-12
    assert np.abs(d2 - d2s).max() < 1e-12
    assert np.array_equal(R.region_of(uv[:, 0], uv[:, 1]), regions)
    # the fp32 transcription finds the same things to fp32 accuracy, and a masked vertex removes the triangle
    f32, d32, uv32 = R.closest_f32(pts.astype(np.float32), verts.astype(np.float32), faces)
    assert (f32 == 1).all() and np.abs(d32 - d2s).max() < 1e-5
    allowed = np.ones(6, bool)
    allowed[2] = False
    face_m, d2_m, _ = R.closest_f64(pts, verts, faces, allowed)
    assert (face_m == 0).all() and (d2_m > d2).all()
    face_n, d2_n, uv_n = R.closest_f64(pts, verts, faces, np.zeros(6, bool))
    assert (face_n == -1).all() and np.isinf(d2_n).all() and (uv_n == 0).all()


def test_degenerate_triangles_give_finite_distances_and_valid_weights():
    rs = np.random.RandomState(1)
    p = rs.randn(3, 3)
    verts = np.stack([p[0], p[0], p[0], p[1], p[1], p[2], p[0], 0.5 * (p[0] + p[1]), p[1]]).astype(np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5], [5, 3, 4], [6, 7, 8], [7, 8, 6]])   # a point, two doubled corners, two collinear
    s = rs.randn(500, 3).astype(np.float32)
    for f in range(faces.shape[0]):
        for fn, dt in ((R.closest_f32, np.float32), (R.closest_f64, np.float64)):
            face, d2, uv = fn(s, verts, faces[f:f + 1])
            assert (face == 0).all() and np.isfinite(d2).all()
            l0 = (dt(1) - uv[:, 0]) - uv[:, 1]
            assert (uv >= 0).all() and (uv <= 1).all() and (l0 >= 0).all() and (l0 <= 1).all()
            # no worse than the nearest corner by more than rounding, for what the rules promise on these shapes
            corner = ((s[:, None, :].astype(np.float64) - verts[faces[f]][None].astype(np.float64)) ** 2).sum(-1)
            if f < 3:
                assert (d2 <= corner.min(1) * (1 + 1e-5) + 1e-12).all()
            else:
                assert (d2 <= corner.max(1) * (1 + 1e-5) + 1e-12).all()


def test_gradient_formula_against_central_differences():
    """d/dx of mean_j |s_j - q_j(x)|^2 with the weights held constant, against central differences of the float64 distance, on
    semantic.npz's mesh with jittered vertices.  Points within TIE of a medial-axis tie are left out (share printed, capped)."""
    h = load_hierarchy(os.path.join(GOLD, "semantic.npz"))
    rs = np.random.RandomState(5)
    verts = np.asarray(h.verts, np.float64) + 0.004 * rs.randn(*h.verts.shape)
    faces = np.asarray(h.faces, np.int64)
    n = verts.shape[0]
    s = R.sample_surface(verts, faces, 600, seed=8, sigma=0.02).astype(np.float64)
    face, d2, uv = R.closest_f64(s, verts, faces)
    tie = R.tie_mask_f64(s, verts, faces, face, uv, d2)
    share = tie.mean()
    print("central differences: %d of %d points left out by the medial-axis rule (%.3f %%)" % (tie.sum(), tie.size, 100 * share))
    assert share <= R.TIE_CAP
    keep = ~tie
    m = s.shape[0]
    g = R.surface_grad_f64(s, verts, faces, face, uv, keep, n, m)
    assert (R.region_of(uv[keep, 0], uv[keep, 1]) == 0).any() and (R.region_of(uv[keep, 0], uv[keep, 1]) > 0).any()

    def value(v):
        return R.closest_f64(s[keep], v, faces)[1].sum() / m

    used = np.unique(faces[face[keep]])
    step = 1e-6
    worst = 0.0
    for i in rs.choice(used, 24, replace=False):
        for k in range(3):
            vp, vm = verts.copy(), verts.copy()
            vp[i, k] += step; vm[i, k] -= step
            cd = (value(vp) - value(vm)) / (2 * step)
            worst = max(worst, abs(cd - g[i, k]))
    print("central differences: max |cd - formula| %.3g of max |g| %.3g" % (worst, np.abs(g).max()))
    assert worst <= 1e-6 * np.abs(g).max() + 1e-12, (worst, np.abs(g).max())


def test_vertex_objective_has_a_floor_on_surface_samples_and_the_surface_objective_has_none():
    """What the feature is for: 4000 points sampled on the 6890-vertex template's own triangles (fp32-rounded) lie at a mean
    squared distance above 1e-4 from the nearest VERTEX and below 1e-12 from the SURFACE (float64, reference only)."""
    h = load_hierarchy(os.path.join(GOLD, "template6890.npz"))
    verts, faces = np.asarray(h.verts, np.float64), np.asarray(h.faces, np.int64)
    s = R.sample_surface(verts, faces, 4000, seed=0)
    d_vertex = scan_ref.nearest_f64(s, verts)[1].mean()
    d_surface = R.closest_f64(s, verts, faces)[1].mean()
    print("on-surface samples: mean d2 to the nearest vertex %.3g, to the surface %.3g" % (d_vertex, d_surface))
    assert d_surface < 1e-12 and d_vertex > 1e-4


def test_face_table_validation():
    ok = np.array([[0, 1, 2], [2, 1, 3]])
    ft = scan.FaceTable(ok, 4, "cpu")
    assert len(ft) == 2 and ft.n == 4 and ft.faces.dtype == torch.int32 and ft.faces.tolist() == ok.tolist()
    assert scan.FaceTable(torch.from_numpy(ok), 4, "cpu").faces.tolist() == ok.tolist()
    assert len(scan.FaceTable(np.zeros((0, 3), np.int32), 4, "cpu")) == 0
    for bad in (ok.astype(np.float32), ok.reshape(-1), ok[:, :2], np.array([[0, 1, 4]]), np.array([[0, -1, 2]]), np.array([[0, 1, 1]]),
                np.array([[3, 1, 3]])):
        with pytest.raises(ValueError):
            scan.FaceTable(bad, 4, "cpu")
    with pytest.raises(ValueError):                                       # a table that touches the dummy row (row n)
        scan.FaceTable(np.array([[0, 1, 4]]), 4, "cpu")
    x = torch.zeros((2, 5, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        scan.nearest_surface(x, x, ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        scan.chamfer(x, [np.zeros((3, 3)), np.zeros((2, 3))], faces=ok)


def test_scanbatch_morton_order_is_a_permutation_and_the_default_is_unchanged():
    rs = np.random.RandomState(2)
    clouds = [rs.randn(m, 3).astype(np.float32) for m in (700, 1, 33)]
    plain = scan.ScanBatch(clouds, "cpu")
    pts, counts = scan.pack_clouds(clouds)                                 # today's packing, untouched by the new argument
    assert plain.perm is None and np.array_equal(plain.points.numpy().view(np.int32), pts.view(np.int32))
    assert np.array_equal(scan.ScanBatch(clouds, "cpu", order=None).points.numpy().view(np.int32), pts.view(np.int32))
    sb = scan.ScanBatch(clouds, "cpu", order="morton")
    assert sb.counts.tolist() == [700, 1, 33] and tuple(sb.perm.shape) == (3, 700) and sb.perm.dtype == np.int64
    for b, c in enumerate(clouds):
        m = c.shape[0]
        assert np.array_equal(np.sort(sb.perm[b, :m]), np.arange(m)) and (sb.perm[b, m:] == -1).all()
        assert np.array_equal(sb.points[b, :m].numpy(), c[sb.perm[b, :m]])  # points[b, k] = cloud[perm[b, k]]
        assert float(sb.points[b, m:].abs().sum()) == 0.0
    # neighbours in memory are neighbours in space: the mean step along the sorted cloud is far shorter than along the given one
    step = lambda p: np.linalg.norm(np.diff(p, axis=0), axis=1).mean()
    assert step(sb.points[0].numpy()) < 0.5 * step(clouds[0])
    one = sb.select(slice(2, 3))
    assert np.array_equal(one.perm, sb.perm[2:3])
    with pytest.raises(ValueError):
        scan.ScanBatch(clouds, "cpu", order="hilbert")


def test_new_symbols_are_exported_and_validate_before_the_device():
    lib = _lib.load()
    for name in ("sh_nearest_surface", "sh_nearest_surface_workspace", "sh_nearest_surface_chunks", "sh_chamfer_surface_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    null, some, f = ctypes.c_void_p(0), ctypes.c_void_p(64), ctypes.c_float
    rc = lib.sh_nearest_surface(null, 0, 0, null, null, 0, 0, null, 0, null, 0, null, 0, 0, 1, null, null, null, null, null, 0, null)
    assert rc == -1 and b"null pointer" in lib.sh_last_error()
    rc = lib.sh_chamfer_surface_bwd(null, 0, 0, 0, null, 0, 0, null, null, 0, null, null, null, null, null, null, 0, null, f(0), f(0), null, 0,
                                    null, null)
    assert rc == -1 and b"null pointer" in lib.sh_last_error()
    for B, nq, nF, chunks in ((-1, 4, 4, 0), (1, -4, 4, 0), (1, 4, -4, 0), (1, 4, 4, -1)):
        rc = lib.sh_nearest_surface(some, 12, nq, null, some, 15, 5, some, nF, null, 0, null, B, chunks, 1, some, some, some, null, null, 0, null)
        assert rc == -1 and b"negative size" in lib.sh_last_error(), (B, nq, nF, chunks)
    assert lib.sh_nearest_surface(some, 12, 4, null, some, 15, 5, some, 4, null, 0, null, 0, 0, 1, some, some, some, null, null, 0, null) == 0
    assert lib.sh_nearest_surface(some, 12, 0, null, some, 15, 5, some, 4, null, 0, null, 2, 0, 1, some, some, some, null, null, 0, null) == 0
    # the workspace is always needed (records, spheres, partial results) and a call without it is refused on the host
    assert lib.sh_nearest_surface_workspace(1, 100, 1000, 4) == 1000 * 16 + 1000 * 48 + 4 * 100 * 8
    rc = lib.sh_nearest_surface(some, 300, 100, null, some, 3000, 1000, some, 1000, null, 0, null, 1, 4, 1, some, some, some, null, null, 0, null)
    assert rc == -3 and b"workspace" in lib.sh_last_error()
    assert lib.sh_nearest_surface_chunks(64, 50000, 13776) == 1 and lib.sh_nearest_surface_chunks(1, 1000, 13776) > 1
    assert lib.sh_chamfer_surface_bwd(some, 15, 5, 4, some, 12, 4, null, some, 2, some, some, some, null, null, null, 0, some, f(1), f(0), some, 0,
                                      some, null) == 0                                                                    # B == 0
    assert lib.sh_chamfer_surface_bwd(some, 15, 5, 4, some, 12, 4, null, some, 2, some, some, some, some, null, null, 0, some, f(1), f(0), some, 1,
                                      some, null) == -1                                                                   # idx_ms without d2_ms
