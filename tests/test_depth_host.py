"""Depth images without a GPU: the host reference of tests/depth_ref.py against analytic truth (planes, a sphere in front of a
plane, isolated pixels), the Z-rank, the argument checks of the three C entry points and the ValueErrors scan.unproject_depth
raises before any device use."""
import ctypes
import math

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, scan
from tests import depth_ref as R


def test_fronto_parallel_plane_normals_are_exact():
    """fx = fy = 64, cx = cy = 8, z = 2 everywhere: the tangents are (2 z / 64, 0, 0) and (0, 2 z / 64, 0) up to one exact
    halving at the border, the cross product lies along +z, points away from the camera and is negated: (0, 0, -1) exactly."""
    ref = R.unproject(R.fronto_plane(17, 17), (64.0, 64.0, 8.0, 8.0))
    assert ref.known.all() and ref.kept.all() and len(ref.pixel) == 17 * 17
    assert (ref.normal == np.array([0.0, 0.0, -1.0], np.float32)).all()
    assert (ref.normals == np.array([0.0, 0.0, -1.0], np.float32)).all()


def test_tilted_plane_normals_within_the_derived_bound():
    """24 x 24, fx = fy = 64, cx = cy = 11.5, the plane through (0, 0, 1.5) with normal along (0.3, -0.2, -1); every normal, the
    one-sided ones at the border included, within `bound` of the plane's.

    The bound, from the scene's numbers.  |x'|, |y'| <= 11.5 / 64 = 0.18 and z = 1.5 / (1 - 0.3 x' + 0.2 y') lies in [1.37, 1.65]
    (measured below on the float64 scene).  z is rounded to fp32 once: e_z <= 2^-24 (half an ulp below 2).  X = ((u - cx) z) / fx:
    (u - cx) is exact, the product is below 32 and rounds by <= 2^-20, which the division by 64 carries to 2^-26, and the quotient
    is below 0.5 and rounds by <= 2^-26; against the true point x' z_true that is e_xy <= 0.18 e_z + 2^-25, and likewise Y.  A
    computed point is therefore within eps = sqrt(2 e_xy^2 + e_z^2) ~ 8.3e-8 of a point ON the plane.  A tangent is the fp32
    difference of two such points: off by delta <= 2 eps + 2^-24 |t| from a true tangent t that lies in the plane.  With c = tx x ty
    (along the plane's normal, |c| = |tx| |ty| sin(phi)) the computed cross product is off by at most |tx| delta + |ty| delta +
    delta^2, so the angle is at most asin of that over |c|: about delta (1 / |tx| + 1 / |ty|) / sin(phi).  The shortest tangents
    are the one-sided ones, |t| >= z_min / 64 ~ 0.0215, and sin(phi) >= 0.99: bound ~ 1.6e-5 rad, plus 2^-23 for the fp64
    arithmetic and the final rounding of three components.  That is above the 1e-5 one would guess for central differences
    alone - the border's one-sided tangents are half as long - so the derived value is the one asserted, computed below from
    the float64 scene and not from the code under test."""
    H = W = 24
    intr = (64.0, 64.0, 11.5, 11.5)
    n_true = np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0])
    z64 = R.tilted_plane(H, W, intr, n_true, (0.0, 0.0, 1.5))
    P64 = R.rays(H, W, intr) * z64[..., None]
    assert 1.37 <= z64.min() and z64.max() <= 1.65 and np.abs(P64[..., :2]).max() < 0.5 and (11.5 * z64.max()) < 32
    e_z = 2.0 ** -24
    e_xy = 11.5 / 64 * e_z + 2.0 ** -25
    eps = math.sqrt(2 * e_xy ** 2 + e_z ** 2)
    tx1, ty1 = np.linalg.norm(np.diff(P64, axis=1), axis=-1), np.linalg.norm(np.diff(P64, axis=0), axis=-1)     # one-sided: the shortest
    t_max = 2 * max(tx1.max(), ty1.max())
    delta = 2 * eps + 2.0 ** -24 * t_max
    ux = np.diff(P64, axis=1)[:-1] / tx1[:-1, :, None]
    uy = np.diff(P64, axis=0)[:, :-1] / ty1[:, :-1, None]
    sin_phi = np.linalg.norm(np.cross(ux, uy), axis=-1).min()
    worst_c = tx1.min() * ty1.min() * sin_phi
    bound = math.asin((tx1.min() * delta + ty1.min() * delta + delta * delta) / worst_c) + 2.0 ** -23
    assert 1e-5 < bound < 2e-5, bound
    ref = R.unproject(z64.astype(np.float32), intr)
    assert ref.known.all()
    cos = np.clip(ref.normal.astype(np.float64) @ n_true, -1, 1)
    sin = np.linalg.norm(np.cross(ref.normal.astype(np.float64), n_true), axis=-1)
    ang = np.arctan2(sin, cos)
    print("tilted plane: bound %.3e rad, largest angle %.3e rad (interior %.3e)" % (bound, ang.max(), ang[1:-1, 1:-1].max()))
    assert ang.max() <= bound


def test_no_tangent_crosses_the_silhouette():
    """The sphere ends about 0.5 in front of the plane; with max_step = 0.3 no usable neighbour pairs a sphere pixel with a plane
    pixel, and without max_step some do."""
    H, W = 48, 80
    intr = R.intrinsics_for(H, W)
    depth, on_sphere = R.sphere_over_plane(H, W, intr)
    assert on_sphere.any() and not on_sphere.all()
    assert 2.0 - depth[on_sphere].max() > 0.3
    shifts = {"L": (-1, 0), "R": (1, 0), "U": (0, -1), "D": (0, 1)}

    def crossing(ref):
        return sum(int((ref.usable[k] & (R._neighbour(on_sphere, du, dv, False) != on_sphere)
                        & R._neighbour(np.ones_like(on_sphere), du, dv, False)).sum()) for k, (du, dv) in shifts.items())

    assert crossing(R.unproject(depth, intr)) > 0
    cut = R.unproject(depth, intr, max_step=0.3)
    assert crossing(cut) == 0
    assert cut.known[~on_sphere].all()                       # the plane keeps a one-sided tangent at the silhouette
    ang = np.arccos(np.clip(-(cut.normal[~on_sphere].astype(np.float64) @ [0, 0, 1.0]), -1, 1))
    assert ang.max() < 1e-5                                  # and stays the plane: no normal bent towards the sphere


def test_drop_isolated_drops_a_pixel_among_holes():
    depth = np.zeros((9, 9), np.float32)
    depth[4, 4] = 1.0                                        # alone
    depth[0, 0:2] = 1.0                                      # a pair: a horizontal tangent only
    depth[6:8, 0:2] = 1.0                                    # a 2 x 2 block: both tangents, one-sided
    intr = (10.0, 10.0, 4.0, 4.0)
    loose, strict = R.unproject(depth, intr), R.unproject(depth, intr, drop_isolated=True)
    assert len(loose.pixel) == 7 and loose.valid[4, 4] and not loose.known[4, 4] and not loose.known[0, 0]
    assert (loose.normals[loose.pixel == 4 * 9 + 4] == 0).all()
    assert sorted(strict.pixel.tolist()) == [6 * 9, 6 * 9 + 1, 7 * 9, 7 * 9 + 1]
    assert (np.abs(strict.normals).sum(1) > 0).all()


def test_holes_are_not_valid():
    depth = np.full((4, 5), 2.0, np.float32)
    depth.reshape(-1)[:5] = R.HOLES
    ref = R.unproject(depth, (10.0, 10.0, 2.0, 2.0), z_range=R.Z_RANGE)
    assert not ref.valid.reshape(-1)[:5].any() and ref.valid.reshape(-1)[5:].all()
    assert R.unproject(depth, (10.0, 10.0, 2.0, 2.0)).valid.reshape(-1)[:5].tolist() == [False, False, False, False, True]
    words = R.to_words(depth)
    assert words.reshape(-1)[:5].tolist() == [0, 0, 0, 0, 9000]
    a, b = R.unproject(words, (10.0, 10.0, 2.0, 2.0), depth_scale=0.001), R.unproject(words.astype(np.float32), (10.0, 10.0, 2.0, 2.0), depth_scale=0.001)
    assert np.array_equal(a.points.view(np.int32), b.points.view(np.int32)) and np.array_equal(a.pixel, b.pixel)


def test_z_rank_is_a_bijection():
    lu, lv = np.meshgrid(np.arange(16), np.arange(16))
    r = R.z_rank(lu, lv)
    assert sorted(r.reshape(-1).tolist()) == list(range(256))
    assert r[0, 1] == 1 and r[1, 0] == 2 and r[1, 1] == 3 and r[0, 2] == 4 and r[15, 15] == 255 and r[8, 0] == 128
    ref = R.unproject(R.fronto_plane(16, 32), (64.0, 64.0, 8.0, 8.0))        # two tiles side by side: rows 0..255, then 256..511
    v, u = np.divmod(ref.pixel, 32)
    assert (u[:256] < 16).all() and (u[256:] >= 16).all()
    assert np.array_equal(R.z_rank(u % 16, v % 16), np.tile(np.arange(256), 2))


def test_argument_validation_without_gpu():
    """The three entry points refuse bad arguments before they touch the device."""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)                        # `p`: not null, never dereferenced on these paths
    inf = math.inf
    count = lambda depth=p, dtype=0, intr=p, B=1, H=4, W=4, stride=1, counts=p: lib.sh_depth_count(
        depth, dtype, 1.0, intr, null, B, H, W, -inf, inf, inf, 0, stride, counts, p, 1 << 20, null)
    points = lambda depth=p, dtype=0, B=1, H=4, W=4, stride=1, counts=p, most=3, M=3, out=p: lib.sh_depth_points(
        depth, dtype, 1.0, p, null, B, H, W, -inf, inf, inf, 0, stride, counts, most, M, p, 1 << 20, out, p, p, null)
    for rc in (count(depth=null), count(intr=null), count(counts=null), points(depth=null), points(counts=null), points(out=null)):
        assert rc == -1 and b"null pointer" in lib.sh_last_error()
    for rc in (count(B=-1), count(H=-1), points(W=-1), points(M=-1, most=-2)):
        assert rc == -1 and b"negative size" in lib.sh_last_error()
    for rc in (count(stride=0), points(stride=-3)):
        assert rc == -1 and b"stride" in lib.sh_last_error()
    for rc in (count(dtype=2), points(dtype=-1)):
        assert rc == -1 and b"dtype" in lib.sh_last_error()
    assert points(most=4, M=3) == -1 and b"cannot hold" in lib.sh_last_error()
    assert count(B=0) == 0 and count(H=0) == 0 and points(W=0) == 0 and points(B=0) == 0        # nothing to do, nothing launched
    assert lib.sh_depth_workspace(2, 17, 33) == 2 * 2 * 3 * 4 and lib.sh_depth_workspace(0, 17, 33) == 0
    assert lib.sh_depth_workspace(1, 16, 16) == 4 and lib.sh_depth_workspace(1, 0, 16) == 0


@pytest.mark.parametrize("kwargs, match", [
    (dict(depth=np.zeros((2, 3, 4, 5), np.float32)), "depth must be"),
    (dict(depth=np.zeros((3, 4), np.float64)), "depth must be"),
    (dict(depth=np.zeros((3, 4), np.int32)), "depth must be"),
    (dict(depth=np.zeros((0, 4), np.float32)), "depth must be"),
    (dict(depth=torch.zeros((3, 4), dtype=torch.float64)), "depth must be"),
    (dict(intrinsics=(1.0, 1.0, 0.0)), "intrinsics must be"),
    (dict(intrinsics=np.ones((3, 4))), "intrinsics must be"),
    (dict(intrinsics=(0.0, 1.0, 0.0, 0.0)), "fx and fy"),
    (dict(intrinsics=(1.0, -2.0, 0.0, 0.0)), "fx and fy"),
    (dict(intrinsics=(math.nan, 1.0, 0.0, 0.0)), "fx and fy"),
    (dict(intrinsics=(1.0, math.inf, 0.0, 0.0)), "fx and fy"),
    (dict(mask=np.ones((4, 3), bool)), "mask must be"),
    (dict(mask=np.ones((3, 4), np.float32)), "mask must be"),
    (dict(z_range=(2.0, 1.0)), "z_range"),
    (dict(z_range=(1.0,)), "z_range"),
    (dict(max_step=-0.1), "max_step"),
    (dict(max_step=math.nan), "max_step"),
    (dict(stride=0), "stride"),
    (dict(stride=1.5), "stride"),
])
def test_unproject_depth_value_errors_before_any_device_use(kwargs, match):
    args = dict(depth=np.ones((3, 4), np.float32), intrinsics=(10.0, 10.0, 2.0, 1.5))
    args.update(kwargs)
    depth, intrinsics = args.pop("depth"), args.pop("intrinsics")
    with pytest.raises(ValueError, match=match):
        scan.unproject_depth(depth, intrinsics, **args)
    with pytest.raises(ValueError, match=match):
        scan.ScanBatch.from_depth(depth, intrinsics, "cuda:0", **args)


def test_pixels_default_and_select():
    """`pixels` is None on batches made any other way, and select() carries it."""
    assert scan.ScanBatch.pixels is None
    pts, cnt = torch.zeros((2, 3, 3)), torch.tensor([3, 2], dtype=torch.int32)
    plain = scan.ScanBatch._from_parts(pts, cnt, cnt.numpy(), None, None)
    assert plain.pixels is None and plain.select(slice(0, 1)).pixels is None
    pix = torch.tensor([[0, 1, 2], [5, 4, -1]], dtype=torch.int32)
    with_pix = scan.ScanBatch._from_parts(pts, cnt, cnt.numpy(), None, None, pixels=pix)
    assert torch.equal(with_pix.select(slice(1, 2)).pixels, pix[1:2])
