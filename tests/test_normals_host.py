"""Matching by normal, the host side (no GPU): ScanBatch's normals, FaceTable's vertex-to-face incidence against a brute-force
listing, and the fp32 transcription of the vertex-normal expression against float64 (the measured constant F32_ANGLE)."""
import numpy as np
import pytest

from semantichuman_amd import scan
from tests import normals_ref as N


def clouds_and_normals(counts, seed):
    rs = np.random.RandomState(seed)
    clouds = [rs.randn(m, 3).astype(np.float32) for m in counts]
    normals = [rs.randn(m, 3) * 10.0 ** rs.uniform(-3, 3, size=(m, 1)) for m in counts]      # any length: normalised at packing
    for nb in normals:
        nb[::7] = 0.0                                                                        # "unknown"
    return clouds, normals


# ------------------------------------------------------------------------------------------------ H1
def test_scanbatch_normals_unit_zero_morton_select():
    counts = [40, 13, 2]
    clouds, normals = clouds_and_normals(counts, 0)
    sb = scan.ScanBatch(clouds, "cpu", normals=normals)
    nrm = sb.normals.numpy()
    assert nrm.dtype == np.float32 and nrm.shape == (3, 40, 3)
    for b, m in enumerate(counts):
        zero = (normals[b] == 0).all(1)
        assert (nrm[b, :m][zero] == 0).all() and (nrm[b, m:] == 0).all()
        if zero.all():
            continue
        ln = np.linalg.norm(nrm[b, :m][~zero].astype(np.float64), axis=1)
        assert np.abs(ln - 1.0).max() <= 2.0 ** -23
        ref = normals[b][~zero] / np.linalg.norm(normals[b][~zero], axis=1, keepdims=True)
        assert np.abs(nrm[b, :m][~zero] - ref).max() <= 2.0 ** -24          # normalised in float64, rounded to fp32 once
    # one [B, M, 3] array
    arr = np.stack([normals[0], normals[0][::-1]])
    sb2 = scan.ScanBatch(np.stack([clouds[0], clouds[0]]), "cpu", normals=arr)
    assert np.array_equal(sb2.normals.numpy()[0], nrm[0]) and np.array_equal(sb2.normals.numpy()[1], nrm[0][::-1])
    # morton: the normals follow their points
    sm = scan.ScanBatch(clouds, "cpu", order="morton", normals=normals)
    for b, m in enumerate(counts):
        perm = sm.perm[b, :m]
        assert np.array_equal(sm.points.numpy()[b, :m], sb.points.numpy()[b, :m][perm])
        assert np.array_equal(sm.normals.numpy()[b, :m], nrm[b, :m][perm])
        assert (sm.normals.numpy()[b, m:] == 0).all()
    # select carries them, sharing memory
    sel = sb.select(slice(1, 3))
    assert np.array_equal(sel.normals.numpy(), nrm[1:3]) and sel.normals.data_ptr() == sb.normals[1:3].data_ptr()
    assert scan.ScanBatch(clouds, "cpu").select(slice(0, 1)).normals is None


def test_scanbatch_without_normals_is_what_it_was():
    clouds, normals = clouds_and_normals([17, 5], 1)
    for order in (None, "morton"):
        a = scan.ScanBatch(clouds, "cpu", order=order)
        b = scan.ScanBatch(clouds, "cpu", order=order, normals=normals)
        pts, cnt = scan.pack_clouds(clouds)
        assert a.normals is None and b.normals is not None
        assert np.array_equal(a.points.numpy().view(np.int32), b.points.numpy().view(np.int32))
        assert np.array_equal(a.counts.numpy(), b.counts.numpy()) and np.array_equal(a.counts.numpy(), cnt)
        if order is None:
            assert np.array_equal(a.points.numpy().view(np.int32), pts.view(np.int32))
        else:
            assert np.array_equal(a.perm, b.perm)


@pytest.mark.parametrize("bad", ["rows", "cols", "bodies", "nan", "inf", "ndim"])
def test_scanbatch_normals_value_errors(bad):
    clouds, normals = clouds_and_normals([6, 4], 2)
    if bad == "rows":
        normals[1] = normals[1][:3]
    elif bad == "cols":
        normals[0] = normals[0][:, :2]
    elif bad == "bodies":
        normals = normals[:1]
    elif bad == "nan":
        normals[0][2, 1] = np.nan
    elif bad == "inf":
        normals[1][0, 0] = np.inf
    elif bad == "ndim":
        normals[0] = normals[0].reshape(-1)
    with pytest.raises(ValueError):
        scan.ScanBatch(clouds, "cpu", normals=normals)


# ------------------------------------------------------------------------------------------------ H2
@pytest.mark.parametrize("name", N.TEMPLATES)
def test_facetable_incidence_against_brute_force(name):
    v, f = N.template(name)
    n = v.shape[0]
    ft = scan.FaceTable(f, n, "cpu")
    ptr, idx = ft.vf_ptr.numpy(), ft.vf_idx.numpy()
    assert ptr.dtype == np.int32 and idx.dtype == np.int32 and ptr.shape == (n + 1,) and idx.shape == (3 * f.shape[0],)
    assert ptr[0] == 0 and ptr[-1] == 3 * f.shape[0] and (np.diff(ptr) >= 0).all()
    brute = N.incidence_brute(f, n)
    for vtx in range(n):
        mine = idx[ptr[vtx]:ptr[vtx + 1]]
        assert list(mine) == brute[vtx]
        assert (np.diff(mine) > 0).all()                                   # ascending face order, no face twice
    assert (np.bincount(idx, minlength=f.shape[0]) == 3).all()             # every face listed exactly three times


def test_facetable_incidence_with_isolated_vertices_and_no_faces():
    ft = scan.FaceTable(np.array([[4, 1, 2], [2, 1, 0]]), 7, "cpu")         # vertices 3, 5, 6 are in no face
    assert ft.vf_ptr.tolist() == [0, 1, 3, 5, 5, 6, 6, 6] and ft.vf_idx.tolist() == [1, 0, 1, 0, 1, 0]
    e = scan.FaceTable(np.zeros((0, 3), np.int64), 3, "cpu")
    assert e.vf_ptr.tolist() == [0, 0, 0, 0] and e.vf_idx.numel() == 0


# ------------------------------------------------------------------------------------------------ H3
def test_transcription_error_is_the_recorded_constant():
    """F32_ANGLE is measured, not derived: the largest angle between the header's expression in fp32 and float64 normals over the
    bodies `python -m tests.normals_ref` uses.  The recorded value must cover the measurement and not exceed it by more than a
    rounding-up (so that 4 x F32_ANGLE stays the bound the GPU test means)."""
    worst = N.measure_f32_angle()
    print("fp32 transcription vs float64, largest angle per template: %s; F32_ANGLE %.3e" % (worst, N.F32_ANGLE))
    assert max(worst.values()) <= N.F32_ANGLE <= 1.05 * max(worst.values())


def test_transcription_edge_cases_and_float64_reference():
    # a unit square in the plane z = 0, two faces, counter-clockwise seen from +z: every normal is exactly +z
    x = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 5]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    for fn in (N.normals_f32, N.normals_f64):
        nrm = fn(x, f)
        assert np.array_equal(nrm[:4], np.tile([0.0, 0.0, 1.0], (4, 1))) and (nrm[4] == 0).all()      # vertex 4 is in no face
    # a fan of zero-area faces (collinear corners) gives exact zeros
    x = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], np.float32)
    assert (N.normals_f32(x, np.array([[0, 1, 2], [0, 2, 3]])) == 0).all()
    # the gate's dot product: zero normals give 0, NaN compares false
    assert N.dot_f32(np.zeros(3, np.float32), np.array([0, 0, 1], np.float32)) == 0
    assert not (N.dot_f32(np.array([np.nan, 0, 0], np.float32), np.array([1, 0, 0], np.float32)) >= -np.inf)
