"""The rig form of the depth kernels without a GPU: the host reference of tests/depth_views_ref.py against what it must satisfy
(rotated normals stay unit and keep facing their camera, identity extrinsics change nothing, a known move lands where it must),
and every refusal of scan.unproject_depth_views, of the rig viewpoints and of the new C entry points - all raised before a
device is touched, which on a machine without one is what lets them be seen at all."""
import ctypes

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, scan
from tests import depth_ref as R
from tests import depth_views_ref as RV

H, W = 17, 33


def test_proper_rotations_keep_normals_unit_and_facing():
    """200 random proper rotations (float32 extrinsics) of the sphere-over-plane scene at 17 x 33: | |n'| - 1 | <= 2^-23, and
    n' . (t - P') >= 0 wherever the camera-frame normal was known - the normal still faces its own camera, whose centre is t."""
    depth, intr = R.scene(H, W)
    ref = R.unproject(depth, intr, z_range=R.Z_RANGE)
    v, u = ref.pixel // W, ref.pixel % W
    known = ref.known[v, u]
    assert known.sum() > 100
    rng = np.random.default_rng(11)
    worst_len, least_dot = 0.0, np.inf
    for _ in range(200):
        e = RV.extrinsic(rng)
        assert np.linalg.det(e[:, :3].astype(np.float64)) > 0
        pts, nrm = RV.move(ref, e)
        n64, p64 = nrm[known].astype(np.float64), pts[known].astype(np.float64)
        worst_len = max(worst_len, np.abs(np.linalg.norm(n64, axis=1) - 1).max())
        least_dot = min(least_dot, (n64 * (e[:, 3].astype(np.float64)[None] - p64)).sum(1).min())
        assert (nrm[~known] == 0).all()
    print("largest | |n'| - 1 | = %.3e (2^-23 = %.3e), least n' . (t - P') = %.3e" % (worst_len, 2.0 ** -23, least_dot))
    assert worst_len <= 2.0 ** -23
    assert least_dot >= 0


def test_identity_extrinsics_are_the_single_view_reference():
    depth, intr = R.scene(H, W, seed=3)
    ref = R.unproject(depth, intr, z_range=R.Z_RANGE)
    eye = np.eye(3, 4, dtype=np.float32)
    fused = RV.unproject_views([depth], intr, eye[None], z_range=R.Z_RANGE)
    assert np.array_equal(fused.points, ref.points) and np.array_equal(fused.normals, ref.normals)     # values: the sign of a zero may differ
    assert np.array_equal(fused.pixel, ref.pixel) and (fused.view == 0).all()
    assert np.array_equal(fused.view_first, [0, len(ref.pixel)])


def test_known_move_of_a_fronto_parallel_plane():
    """Camera frame: the plane z = 2, normal (0, 0, -1) towards the camera at the origin.  R = 90 degrees about y maps (X, Y, Z) to
    (Z, Y, -X), so with t = (1, 2, 3) the plane lands on x' = 2 + 1 = 3 and its normal on R (0, 0, -1) = (-1, 0, 0): it faces
    the camera centre t = (1, 2, 3), which lies on the side x' < 3.  Every operation involved is exact."""
    intr = R.intrinsics_for(H, W)
    ref = R.unproject(R.fronto_plane(H, W, 2.0), intr)
    e = np.array([[0, 0, 1, 1], [0, 1, 0, 2], [-1, 0, 0, 3]], np.float32)
    pts, nrm = RV.move(ref, e)
    assert len(pts) == H * W
    assert (pts[:, 0] == 3.0).all()
    assert np.array_equal(pts[:, 1], ref.points[:, 1] + np.float32(2)) and np.array_equal(pts[:, 2], -ref.points[:, 0] + np.float32(3))
    assert np.array_equal(nrm, np.broadcast_to(np.array([-1, 0, 0], np.float32), nrm.shape))


# ------------------------------------------------------------------------------------------------ refusals, Python
def rig(V=2, B=None):
    """Valid inputs: (depth, intrinsics, extrinsics) for V views (and B bodies)."""
    rng = np.random.default_rng(V)
    lead = (V,) if B is None else (B, V)
    ext = np.stack([RV.extrinsic(rng) for _ in range(int(np.prod(lead)))]).reshape(lead + (3, 4))
    return np.full(lead + (4, 5), 2.0, np.float32), (6.0, 6.0, 2.0, 1.5), ext


def bad_extrinsics():
    _, _, ext = rig(2)
    cases = {"rank": ext[0], "shape": ext[:, :, :3], "empty": ext[:0]}
    for name, edit in {"scale": lambda e: e.__setitem__((0, slice(None), slice(0, 3)), e[0, :, :3] * 1.01),
                       "mirror": lambda e: e.__setitem__((1, 0), -e[1, 0]),
                       "partly NaN": lambda e: e.__setitem__((0, 1, 2), np.nan),
                       "inf": lambda e: e.__setitem__((1, 2, 3), np.inf)}.items():
        e = ext.copy()
        edit(e)
        cases[name] = e
    four = np.concatenate([ext, np.broadcast_to(np.array([0, 0, 0, 1], np.float32), (2, 1, 4))], 1)
    four[1, 3, 0] = 0.5
    cases["4 x 4 last row"] = four
    return cases


@pytest.mark.parametrize("name", sorted(bad_extrinsics()))
def test_bad_extrinsics_are_refused_before_the_device(name):
    depth, intr, _ = rig(2)
    with pytest.raises(ValueError):
        scan.unproject_depth_views(depth, intr, bad_extrinsics()[name])


def test_an_all_nan_matrix_and_a_4x4_matrix_are_accepted_by_the_packing():
    _, _, ext = rig(3)
    ext[1] = np.nan
    four = np.concatenate([ext, np.broadcast_to(np.array([0, 0, 0, 1], np.float32), (3, 1, 4))], 1)
    four[1] = np.nan
    a, batched = scan.pack_extrinsics(ext)
    b, _ = scan.pack_extrinsics(four)
    assert not batched and a.shape == (1, 3, 12) and a.dtype == np.float32 and np.array_equal(a, b, equal_nan=True)
    assert np.isnan(a[0, 1]).all() and np.array_equal(a[0, 0, :9].reshape(3, 3), ext[0, :, :3]) and np.array_equal(a[0, 2, 9:], ext[2, :, 3])
    assert scan.pack_extrinsics(ext[None])[1]


@pytest.mark.parametrize("name, change", [
    ("too many views", lambda d, k, e: dict(depth=np.repeat(d, 17, 0)[:33], extrinsics=np.repeat(e, 17, 0)[:33])),
    ("depth and extrinsics disagree", lambda d, k, e: dict(depth=d[:1])),
    ("batch axis on one only", lambda d, k, e: dict(depth=d[None])),
    ("depth dtype", lambda d, k, e: dict(depth=d.astype(np.float64))),
    ("intrinsics shape", lambda d, k, e: dict(intrinsics=np.ones((3, 4)))),
    ("fx", lambda d, k, e: dict(intrinsics=(0.0, 6.0, 2.0, 1.5))),
    ("mask shape", lambda d, k, e: dict(mask=np.ones((2, 4, 4), bool))),
    ("mask dtype", lambda d, k, e: dict(mask=np.ones(d.shape, np.float32))),
    ("z_range", lambda d, k, e: dict(z_range=(3.0, 1.0))),
    ("max_step", lambda d, k, e: dict(max_step=-1.0)),
    ("stride", lambda d, k, e: dict(stride=0)),
])
def test_bad_arguments_are_refused_before_the_device(name, change):
    d, k, e = rig(2)
    kw = dict(depth=d, intrinsics=k, extrinsics=e)
    kw.update(change(d, k, e))
    depth, intrinsics, extrinsics = kw.pop("depth"), kw.pop("intrinsics"), kw.pop("extrinsics")
    with pytest.raises(ValueError):
        scan.unproject_depth_views(depth, intrinsics, extrinsics, **kw)
    with pytest.raises(ValueError):
        scan.ScanBatch.from_depth(depth, intrinsics, "cuda:0", extrinsics=extrinsics, **kw)


@pytest.mark.parametrize("shape", [(2, 0, 3), (2, 33, 3), (3, 2, 3), (2, 2, 2)])
def test_bad_rig_viewpoints_are_refused_before_the_device(shape):
    x = torch.zeros((2, 5, 3))
    with pytest.raises(ValueError):
        scan.visible_vertices(x, np.array([[0, 1, 2]]), np.zeros(shape, np.float32))
    with pytest.raises(ValueError):
        scan.ScanBatch([np.zeros((4, 3), np.float32)] * 2, "cuda:0", rig_viewpoints=np.zeros(shape, np.float32))


def test_rig_viewpoints_may_hold_nan_rows_but_no_inf():
    v = np.zeros((2, 3, 3), np.float32)
    v[0, 1] = np.nan
    assert tuple(scan._view_arg("t", v, 2, None, rig=True).shape) == (2, 3, 3)
    assert tuple(scan._view_arg("t", v[0], 2, None, rig=True).shape) == (2, 3, 3)      # one rig for every body
    with pytest.raises(ValueError, match="device tensor"):                             # a host array of rank 3 is no per-body viewpoint, as ever
        scan._view_arg("t", v, 2, None)
    v[1, 0, 0] = np.inf
    with pytest.raises(ValueError):
        scan._view_arg("t", v, 2, None, rig=True)


# ------------------------------------------------------------------------------------------------ refusals, C ABI
def test_c_entry_points_validate_without_gpu():
    """Every SH_ERR_INVALID_ARG of the three new entry points, in the manner of test_cabi.py: the pointers are host addresses
    that a call which got as far as the device would fault on."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    inf = float("inf")

    def count(depth=p, dtype=0, intr=p, ext=p, B=1, V=2, H=4, W=4, stride=1, counts=p):
        return lib.sh_depth_views_count(depth, dtype, 1.0, intr, null, ext, B, V, H, W, -inf, inf, inf, 0, stride, counts, p, 4096, null)

    def points(depth=p, dtype=0, intr=p, ext=p, B=1, V=2, H=4, W=4, stride=1, counts=p, max_count=3, M=3, out=(p, p, p, p, p)):
        return lib.sh_depth_views_points(depth, dtype, 1.0, intr, null, ext, B, V, H, W, -inf, inf, inf, 0, stride, counts, max_count, M, p, 4096,
                                         *out, null)

    def views(x=p, x_sb=30, n=10, faces=p, nF=4, tn=null, view=p, V=2, cos_g=0.0, mask_sb=0, B=1, chunks=1, vis=p):
        return lib.sh_vertex_visibility_views(x, x_sb, n, faces, nF, tn, view, V, cos_g, null, mask_sb, B, chunks, null, 0, vis, null, null)

    shared = [dict(depth=null), dict(intr=null), dict(ext=null), dict(dtype=7), dict(V=0), dict(V=33), dict(V=-1), dict(B=-1), dict(H=-1),
              dict(W=-2), dict(stride=0)]
    for kw in shared + [dict(counts=null)]:
        assert count(**kw) == -1, kw
        assert lib.sh_last_error()
    for kw in shared + [dict(counts=null), dict(M=2), dict(M=-1, max_count=-1), dict(max_count=-1)] + \
            [dict(out=tuple(null if j == i else p for j in range(5))) for i in range(5)]:
        assert points(**kw) == -1, kw
    for kw in [dict(x=null), dict(view=null), dict(vis=null), dict(faces=null), dict(V=0), dict(V=33), dict(V=-3), dict(B=-1), dict(n=-1),
               dict(nF=-1), dict(chunks=-1), dict(tn=p, cos_g=1.0), dict(tn=p, cos_g=-0.1), dict(tn=p, cos_g=float("nan")), dict(x_sb=29)]:
        assert views(**kw) == -1, kw
    assert b"V = 33" in lib.sh_last_error() or lib.sh_last_error()
    # nothing to do is no error, and launches nothing
    assert count(B=0) == 0 and points(B=0) == 0 and views(B=0) == 0 and views(n=0) == 0
    assert lib.sh_depth_views_workspace(2, 3, 17, 33) == 2 * 3 * 2 * 3 * 4 and lib.sh_depth_views_workspace(2, 33, 17, 33) == 0
    assert lib.sh_vertex_visibility_views_workspace(1, 642, 1280, 5, 1) == 0
    assert lib.sh_vertex_visibility_views_workspace(1, 642, 1280, 5, 3) == 3 * 642 * 4
