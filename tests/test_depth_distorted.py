"""distortion= of the depth wrappers on the GPU against tests/camera_ref.py: unproject_depth and ScanBatch.from_depth with a ray
table - points, normals, pixels and counts bit for bit, fp32 and 16-bit depth, B = 2 and each body alone, stride, drop_isolated,
a mask, an incomplete table, one shared table against per-body tables -, the rig form with an absent camera and merge_tol, what
the feature is for (the unprojected points lie on the analytic surface, the pinhole ones do not), and the default path's launches."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import scan
from tests import camera_ref as C
from tests import depth_ref as R
from tests import depth_views_ref as RV
from tests import views_merge_ref as RM
from tests.launch_record import launches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = C.H, C.W
NEW = ("rays", "camera")                 # what the names of the kernels this form adds hold


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.int32)


@functools.lru_cache(maxsize=None)
def lens(name):
    return C.Lens(C.INTR, getattr(C, name), H, W)


@functools.lru_cache(maxsize=None)
def images(name):
    """Two depth images of the camera `name`: an ellipsoid and a tilted plane cast along the reference's rays, a reading of 2.0
    where a pixel has no ray (so that only the mask rule drops it), holes as in tests/depth_ref.py -> float32 [2, H, W]."""
    table = lens(name).table
    out = []
    for k, surface in enumerate((C.ellipsoid()[0], C.plane()[0])):
        d = C.cast(table, surface)
        out.append(R.holes(np.where(np.isnan(table).any(-1), np.float32(2.0), d), seed=k + 1))
    return np.stack(out)


OPTIONS = {"plain": {}, "stride": dict(stride=2), "isolated": dict(drop_isolated=True, max_step=0.05), "stride_isolated": dict(stride=3, drop_isolated=True)}


def check_rows(got, refs):
    points, normals, pixel, counts = (t.cpu().numpy() for t in got)
    rp, rn, rx, rc = R.pack(refs)
    assert np.array_equal(counts, rc) and points.shape == rp.shape
    assert np.array_equal(pixel, rx)
    assert np.array_equal(bits(points), bits(rp)) and np.array_equal(bits(normals), bits(rn))


@pytest.mark.parametrize("words", [False, True])
@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("name", ["AZURE", "FOLDING"])
def test_unproject_bits(name, opt, words):
    depth, options = images(name), dict(OPTIONS[opt], z_range=R.Z_RANGE)
    mask = np.random.default_rng(5).random((2, H, W)) > 0.1 if opt == "isolated" else None
    scale = 1.0
    if words:
        depth, scale = np.stack([R.to_words(d) for d in depth]), 0.001
    refs = [C.unproject(depth[b], lens(name).table, depth_scale=scale, mask=None if mask is None else mask[b], **options) for b in range(2)]
    assert all(len(r.pixel) > 50 for r in refs)
    d = C.pad8(getattr(C, name))
    got, rec = launches(lambda: scan.unproject_depth(depth, C.INTR, depth_scale=scale, mask=mask, device=DEV, distortion=d, **options))
    assert [k for k, _ in rec] == ["camera_rays_kernel", "camera_limit_kernel", "depth_rays_count_kernel", "depth_scan_kernel", "depth_rays_emit_kernel"]
    assert rec[-1][1].endswith("tables=0")                                 # one table for both bodies
    check_rows(got, refs)
    for b in range(2):                                                     # each body alone: the same bits
        alone = scan.unproject_depth(depth[b], C.INTR, depth_scale=scale, mask=None if mask is None else mask[b], device=DEV, distortion=d, **options)
        check_rows(alone, refs[b:b + 1])
    if name == "FOLDING":                                                  # the incomplete table drops exactly the pixels without a ray
        has = lens(name).has_ray().reshape(-1)
        assert not has.all() and all(has[r.pixel].all() for r in refs)


def test_shared_and_per_body_tables():
    depth = images("AZURE")
    shared = scan.camera_rays(C.INTR, C.AZURE, (H, W), DEV)
    own = scan.camera_rays(np.tile(np.asarray(C.INTR, np.float32), (2, 1)), C.AZURE, (H, W), DEV)
    assert shared.lead == () and own.lead == (2,)
    a, rec_a = launches(lambda: scan.ScanBatch.from_depth(depth, C.INTR, DEV, z_range=R.Z_RANGE, distortion=shared))
    b, rec_b = launches(lambda: scan.ScanBatch.from_depth(depth, C.INTR, DEV, z_range=R.Z_RANGE, distortion=own))
    assert [k for k, _ in rec_a] == ["depth_rays_count_kernel", "depth_scan_kernel", "depth_rays_emit_kernel"]    # a ready table: no ray launch
    assert rec_a[-1][1].endswith("tables=0") and rec_b[-1][1].endswith("tables=1")
    for name in ("points", "normals", "pixels", "counts"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    refs = [C.unproject(depth[k], lens("AZURE").table, z_range=R.Z_RANGE) for k in range(2)]
    check_rows((a.points, a.normals, a.pixels, a.counts), refs)
    assert np.array_equal(a.host_counts, [len(r.pixel) for r in refs]) and (a.viewpoints == 0).all()


# ------------------------------------------------------------------------------------------------ the rig
RIG_SETS = ("AZURE", "BARREL", "BROWN5")


@functools.lru_cache(maxsize=None)
def rig_scene():
    """B = 2 bodies x V = 3 cameras on a ring around an ellipsoid, each with its own lens and intrinsics; camera 1 of body 1 is
    absent (an all-NaN extrinsic) -> (depth [2, 3, H, W], intr [3, 4], dist [3, 8], ext [2, 3, 3, 4], lenses)."""
    intr = np.asarray([C.INTR, (27.0, 28.5, 18.0, 14.25), (29.0, 27.5, 17.0, 13.5)], np.float32)
    lenses = [C.Lens(intr[v], getattr(C, RIG_SETS[v]), H, W) for v in range(3)]
    ring = RM.ring(8, radius=1.5)[:3]                                       # 45 degrees apart: neighbours overlap
    ext = np.stack([ring, ring]).astype(np.float32)
    surfaces = (RM.ellipsoid(radii=(0.5, 0.7, 0.4)), RM.ellipsoid(radii=(0.45, 0.6, 0.5)))
    depth = np.stack([np.stack([R.holes(C.cast(lenses[v].table, surfaces[b], ext[b, v]), seed=3 * b + v) for v in range(3)]) for b in range(2)])
    ext[1, 1] = np.nan
    return depth, intr, np.stack([l.d for l in lenses]), ext, lenses


@pytest.mark.parametrize("words", [False, True])
def test_rig_bits_and_merge(words):
    depth, intr, dist, ext, lenses = rig_scene()
    scale, z_range = 1.0, (0.3, 4.0)
    if words:
        depth, scale = np.stack([[R.to_words(d) for d in body] for body in depth]), 0.001
    tables = [l.table for l in lenses]
    refs = [C.unproject_views(depth[b], tables, ext[b], depth_scale=scale, z_range=z_range, max_step=0.1) for b in range(2)]
    assert all(len(f.pixel) > 100 for f in refs) and refs[1].view_first[1] == refs[1].view_first[2]
    options = dict(depth_scale=scale, z_range=z_range, max_step=0.1, distortion=dist)
    scans, rec = launches(lambda: scan.ScanBatch.from_depth(depth, intr, DEV, extrinsics=ext, **options))
    assert [k for k, _ in rec] == ["camera_rays_kernel", "camera_limit_kernel", "depth_views_rays_count_kernel", "depth_scan_kernel",
                                   "depth_views_rays_emit_kernel"]
    assert rec[-1][1].endswith("tables=0")                                 # [V, 8] coefficients: one table per camera, not per body
    rp, rn, rx, rv, rc, rf = RV.pack(refs)
    assert np.array_equal(scans.counts.cpu().numpy(), rc) and np.array_equal(scans.view_first.cpu().numpy(), rf)
    assert np.array_equal(scans.pixels.cpu().numpy(), rx) and np.array_equal(scans.view.cpu().numpy(), rv)
    assert np.array_equal(bits(scans.points.cpu().numpy()), bits(rp)) and np.array_equal(bits(scans.normals.cpu().numpy()), bits(rn))
    for b in range(2):                                                     # a body alone: the same bits
        alone = scan.ScanBatch.from_depth(depth[b], intr, DEV, extrinsics=ext[b], **options)
        c = int(rc[b])
        assert int(alone.counts[0]) == c and torch.equal(alone.points[0, :c].view(torch.int32), scans.points[b, :c].view(torch.int32))
        assert torch.equal(alone.normals[0, :c].view(torch.int32), scans.normals[b, :c].view(torch.int32))
    # the overlap rule under the lenses
    tol = 0.02
    (keep, seen), rec = launches(lambda: scan.views_overlap(scans, depth, intr, ext, tol=tol, depth_scale=scale, z_range=z_range, distortion=dist))
    assert [k for k, _ in rec] == ["camera_rays_kernel", "camera_limit_kernel", "depth_views_rays_overlap_kernel"]
    keep, seen = keep.cpu().numpy(), seen.cpu().numpy().view(np.uint32)
    want = [C.overlap(f.points, f.normals, f.view, depth[b], intr, [l.d for l in lenses], tables, [l.limit for l in lenses], ext[b], tol,
                      depth_scale=scale, z_range=z_range) for b, f in enumerate(refs)]
    assert np.array_equal(keep, RM.pack_planes([k for k, _ in want]).astype(bool))
    assert np.array_equal(seen, RM.pack_planes([s for _, s in want]))
    assert any((~k).any() for k, _ in want) and any((s & (s - 1)).any() for _, s in want)        # rows are dropped, rows are seen twice
    merged = scan.ScanBatch.from_depth(depth, intr, DEV, extrinsics=ext, merge_tol=tol, **options)
    kept = [RM.compact(f.points, f.normals, f.pixel, f.view, s, k, 3) for f, (k, s) in zip(refs, want)]
    mp, mn, mx, mv, ms, mc, mf = RM.pack(kept)
    assert np.array_equal(merged.counts.cpu().numpy(), mc) and np.array_equal(bits(merged.points.cpu().numpy()), bits(mp))
    assert np.array_equal(merged.seen.cpu().numpy().view(np.uint32), ms) and np.array_equal(merged.view_first.cpu().numpy(), mf)


# ------------------------------------------------------------------------------------------------ what it is for
@pytest.mark.parametrize("shape", ["plane", "ellipsoid"])
def test_points_lie_on_the_surface(shape):
    """With the right coefficients the points satisfy the analytic surface's equation as well as the reference's do (twice its
    worst residual); the pinhole unprojection of the same image misses it by at least 100 times that in the image's corners."""
    surface, residual = getattr(C, shape)()
    table = lens("AZURE").table
    depth = C.cast(table, surface)
    assert np.isfinite(depth).all()
    ref = C.unproject(depth, table)
    bound = 2.0 * np.abs(residual(ref.points)).max()
    points, _, pixel, counts = scan.unproject_depth(depth, C.INTR, device=DEV, distortion=C.AZURE)
    got = points[0].cpu().numpy()
    assert int(counts[0]) == H * W and np.abs(residual(got)).max() <= bound
    pin, _, pin_pixel, _ = scan.unproject_depth(depth, C.INTR, device=DEV)
    pin, pin_pixel = pin[0].cpu().numpy(), pin_pixel[0].cpu().numpy()
    v, u = pin_pixel // W, pin_pixel % W
    corners = ((u < 3) | (u >= W - 3)) & ((v < 3) | (v >= H - 3))
    assert corners.sum() == 36 and np.abs(residual(pin[corners])).min() >= 100.0 * bound


# ------------------------------------------------------------------------------------------------ distortion=None
def test_default_path_launches_nothing_new():
    depth, intr = R.scene(H, W, seed=2)
    _, rec = launches(lambda: scan.ScanBatch.from_depth(depth, intr, DEV, z_range=R.Z_RANGE))
    assert [k for k, _ in rec] == ["depth_count_kernel", "depth_scan_kernel", "depth_emit_kernel"]
    field, rec2 = launches(lambda: scan.DepthField.from_depth(depth, intr, DEV, z_range=R.Z_RANGE))
    x = torch.tensor([[[0.0, 0.0, 1.0], [0.1, 0.0, 1.5], [0.0, 0.0, 0.0]]], device=DEV, requires_grad=True)
    _, rec3 = launches(lambda: sum(scan.free_space(x, field)).sum().backward())
    assert [k for k, _ in rec3] == ["free_space_fwd_kernel", "free_space_bwd_kernel"]
    assert field.rays is None and not any(word in k for k, _ in rec + rec2 + rec3 for word in NEW)
