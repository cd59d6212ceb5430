"""The rig form of the free-space term without a GPU: tests/field_views_ref.py against truth (the float64 inverse of
`pose.compose(E_v)`, the one-view reference under identity cameras, the float64 derivative), the new ValueErrors of scan and the
fits, and the argument checks of the three C entry points, which return before the device is touched."""
import ctypes
import math

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, scan
from tests import field_ref as R
from tests import field_views_ref as RV
from tests.test_field_host import constructed_vertices


def test_cameras_are_the_float64_inverse_of_pose_compose_extrinsic():
    """200 random rigid extrinsics under random similarity poses (scale 0.5 - 2, |t| ~ 1).  Truth: numpy's float64 inverse of the
    4 x 4 product P E_v of the SAME float32 inputs.  Three things separate the two.  (1) The one rounding of every word to
    float32: 2^-24 |truth|.  (2) The header inverts R_v by transposing it, and a rotation rounded to float32 is orthogonal only to
    |R^T R - I| <= 2 * 3 * 2^-25 (nine entries below 1, each off by at most 2^-25, Frobenius norm 3 * 2^-25, twice in the product):
    R^T - R^-1 = (R^T R - I) R^-1 moves a word by at most 3 * 2^-24 times the size of what it multiplies - the spectral norm of
    M = 1 / scale for the nine words of M, |c| for the three of c.  (3) float64 noise of an adjugate inverse of a matrix of
    condition 1 and a few products of numbers below 10: far under the 1e-12 allowed.  Asserted per word:
    |cam - truth| <= 2^-24 (|truth| + 3 size) + 1e-12.  The largest |cam - truth| / bound seen (printed): 0.499."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(200):
        Rp, tp = RV.rigid(rng, 1.0)
        pose = RV.pack(rng.uniform(0.5, 2.0) * Rp, tp)
        ext = np.stack([RV.pack(*RV.rigid(rng, 1.0)) for _ in range(3)])
        cam = RV.cameras(pose, ext)
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = pose[:9].astype(np.float64).reshape(3, 3), pose[9:]
        for v in range(3):
            E = np.eye(4)
            E[:3, :3], E[:3, 3] = ext[v, :9].astype(np.float64).reshape(3, 3), ext[v, 9:]
            truth = np.linalg.inv(P @ E)
            want = np.concatenate([truth[:3, :3].reshape(9), truth[:3, 3]])
            size = np.concatenate([np.full(9, np.linalg.norm(truth[:3, :3], 2)), np.full(3, np.linalg.norm(truth[:3, 3]))])
            ratio = np.abs(cam[v].astype(np.float64) - want) / (2.0 ** -24 * (np.abs(want) + 3.0 * size) + 1e-12)
            worst = max(worst, float(ratio.max()))
    print("cameras: largest |cam - truth| / bound = %.4f" % worst)
    assert worst <= 1.0


def test_cameras_edge_rows():
    ext = np.stack([RV.IDENTITY, np.full(12, np.nan, np.float32), RV.pack(np.eye(3), [1.0, 2.0, 3.0])])
    cam = RV.cameras(None, ext)
    assert np.array_equal(cam[0], RV.IDENTITY) and np.isnan(cam[1]).all()           # -0 == 0: the translation may be -0
    assert cam[2].tolist() == RV.IDENTITY[:9].tolist() + [-1.0, -2.0, -3.0]
    singular = np.asarray([1, 2, 3, 2, 4, 6, 0, 0, 1, 0, 0, 0], np.float32)
    assert np.isnan(RV.cameras(singular, ext)).all()
    assert np.isnan(RV.cameras(np.full(12, np.inf, np.float32), ext)).all()
    half = RV.cameras(np.asarray([2, 0, 0, 0, 2, 0, 0, 0, 2, 4, 6, 8], np.float32), ext[:1])   # model = 2 rig + t: rig = (model - t) / 2
    assert half[0].tolist() == [0.5, 0, 0, 0, 0.5, 0, 0, 0, 0.5, -2.0, -3.0, -4.0]


def scene(seed=5):
    H, W = 24, 32
    intr = (40.0, 42.0, 15.25, 11.5)
    rng = np.random.default_rng(seed)
    cls = np.zeros((H, W), np.uint8)
    cls[6:18, 10:22] = R.SURFACE
    cls[0:3, 0:5] = R.UNKNOWN
    return R.field_of_classes(cls, intr, z=2.0 + 0.01 * rng.standard_normal((H, W))), rng


def test_identity_cameras_reproduce_the_one_view_reference_bitwise():
    f, rng = scene()
    n = 300
    x = constructed_vertices(f, rng, n)
    x[7] = [0.1, 0.1, -1.0]
    x[8] = [0.1, 0.1, np.nan]
    mask = rng.random(n) > 0.1
    cam = RV.IDENTITY[None]
    q, finite = RV.transform(x, cam[0]), np.isfinite(x).all(1)
    assert np.array_equal(q[finite].view(np.int32), x[finite].view(np.int32)) and np.isnan(q[8, 2])      # Q == x for finite x
    for margin, m in ((0.0, None), (0.03125, mask)):
        one = R.terms(x, n, f, m, margin)
        rig = RV.terms(x, n, [f], cam, m, margin)
        for a, b in zip(one, rig):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b[0]).view(np.uint8))
        assert RV.losses(rig[0], rig[1], rig[3]) == R.losses(one[0], one[1], one[3])
        gL = (0.5, 2.0)
        g1 = R.gradient(one[1], one[2], one[3], gL, n + 2)
        gv = RV.gradient(rig[1], rig[2], rig[3], gL, n + 2, cam)
        assert np.array_equal(g1.view(np.int32), gv.view(np.int32)) and (np.signbit(g1) == np.signbit(gv)).all()


def test_float32_gradient_is_the_derivative_of_the_float64_restatement():
    """Two cameras on one body: camera 0's frame is a rigid move of the model's, camera 1 a second rigid move; the vertices are
    constructed as in tests/test_field_host.py for camera 0 and kept only where camera 1 either does not see them or sees them at
    least 0.2 pixel from a pixel boundary, so that no pixel choice can differ between the float32 and the float64 path or change
    within the step h.  Tolerance 2.5e-6, that of the one-view test: the same handful of fp32 operations, preceded by the four
    roundings of Q (|Q| <= 3: 7e-7 at the very worst, 2e-7 typical) and followed by M^T w with |m| <= 1."""
    f, rng = scene()
    f2 = R.field_of_classes(np.roll(f.cls, 3, axis=1), f.intr, z=np.roll(f.z, 3, axis=1))
    H, W = f.cls.shape
    e0, e1 = RV.rigid(rng, 0.2), (np.linalg.qr(np.eye(3) + 0.05 * rng.standard_normal((3, 3)))[0], 0.05 * rng.standard_normal(3))
    e1 = (e1[0] * np.sign(np.diag(e1[0]))[None, :], e1[1])                  # near the identity, proper
    assert np.linalg.det(e1[0]) > 0
    ext = np.stack([RV.pack(*e0), RV.pack(e0[0] @ e1[0], e0[0] @ e1[1] + e0[1])])
    cam = RV.cameras(None, ext)
    cand = constructed_vertices(f, rng, 1600).astype(np.float64) @ e0[0].T + e0[1]   # camera 0's frame -> the model's
    cand = cand.astype(np.float32)
    q1 = RV.transform(cand, cam[1])
    uf, vf, inside, u, v = R.project(q1, f2.intr, H, W)
    seen = inside & (np.abs(uf - u) <= 0.3) & (np.abs(vf - v) <= 0.3) & ((f2.cls[v, u] != R.SURFACE) | (np.abs(f2.z[v, u] - q1[:, 2]) > 1e-3))
    away = (uf < -0.7) | (uf > W - 0.3) | (vf < -0.7) | (vf > H - 0.3)
    x = cand[(q1[:, 2] > 0.5) & (seen | away)][:400]
    n = len(x)
    assert n == 400
    fields = [f, f2]
    term, kind, g, counts = RV.terms(x, n, fields, cam)
    assert set(kind[0].tolist()) == {R.NONE, R.FREE, R.SILHOUETTE} and {R.FREE, R.SILHOUETTE} <= set(kind[1].tolist())
    uf0, vf0, in0, u0, v0 = R.project(RV.transform(x, cam[0]), f.intr, H, W)
    assert in0.all() and (np.abs(uf0 - u0) <= 0.26).all() and (np.abs(vf0 - v0) <= 0.26).all()
    gx = RV.gradient(kind, g, counts, (float(n), float(n)), n, cam)          # gL = n_act: the factor fl(n * fl(1 / n)) is 1 to an ulp
    h = 1e-6
    x64 = x.astype(np.float64)
    worst = 0.0
    for k in range(3):
        step = np.zeros(3)
        step[k] = h
        hi, lo = RV.terms64(x64 + step, n, fields, cam), RV.terms64(x64 - step, n, fields, cam)
        d = ((hi[0] + hi[1]) - (lo[0] + lo[1])).sum(0) / (2 * h)
        worst = max(worst, float(np.abs(gx[:, k].astype(np.float64) - d).max()))
    t64 = RV.terms64(x64, n, fields, cam)
    worst_term = float(np.abs(term.astype(np.float64) - (t64[0] + t64[1])).max())
    print("gradient: largest |g_x - d/dx| = %.3g, term: %.3g" % (worst, worst_term))
    assert worst <= 2.5e-6 and worst_term <= 2.5e-6


def rig_field(B=2, V=3, H=3, W=4, device="cpu"):
    return scan.DepthField(torch.zeros((B, V, H, W), dtype=torch.uint8, device=device), torch.zeros((B, V, H, W), device=device),
                           torch.zeros((B, V, H, W), dtype=torch.int32, device=device), torch.ones((B, V, 4), device=device),
                           torch.zeros((B, V, 12), device=device))


def test_rig_field_members_and_select():
    fld = rig_field()
    assert len(fld) == 2 and fld.shape == (3, 4) and fld.views == 3
    one = fld.select(slice(1, 2))
    assert len(one) == 1 and one.views == 3 and one.shape == (3, 4) and one.extrinsics.shape == (1, 3, 12) and one.cls.shape == (1, 3, 3, 4)
    plain = scan.DepthField(fld.cls[:, 0], fld.z[:, 0], fld.nearest[:, 0], fld.intrinsics[:, 0])
    assert plain.views is None and plain.extrinsics is None and plain.select(slice(0, 1)).extrinsics is None


@pytest.mark.parametrize("kwargs, match", [
    (dict(extrinsics=np.zeros((2, 3, 3))), "must be .V, 3, 4."),
    (dict(extrinsics=np.tile(2 * np.eye(3, 4), (2, 1, 1))), "proper rotation"),
    (dict(extrinsics=np.tile(np.eye(3, 4), (33, 1, 1)), depth=np.ones((33, 3, 4), np.float32)), "33 views, at most 32"),
    (dict(depth=np.ones((3, 3, 4), np.float32)), "depth must be .2, H, W."),
    (dict(depth=np.ones((1, 2, 3, 4), np.float32)), "depth must be .2, H, W."),
    (dict(intrinsics=np.ones((3, 4))), "intrinsics must be"),
    (dict(intrinsics=(0.0, 1.0, 0.0, 0.0)), "fx and fy"),
    (dict(mask=np.ones((3, 4), bool)), "mask must have the depth's shape"),
    (dict(z_range=(2.0, 1.0)), "z_range"),
    (dict(depth=np.ones((2, 3, 4), np.float64)), "depth must be"),
])
def test_rig_field_value_errors_before_any_device_use(kwargs, match):
    """The checks and messages of unproject_depth_views: the same helpers serve both."""
    args = dict(depth=np.ones((2, 3, 4), np.float32), intrinsics=(10.0, 10.0, 2.0, 1.5), extrinsics=np.tile(np.eye(3, 4), (2, 1, 1)))
    args.update(kwargs)
    depth, intrinsics, extrinsics = args.pop("depth"), args.pop("intrinsics"), args.pop("extrinsics")
    with pytest.raises(ValueError, match=match) as ours:
        scan.DepthField.from_depth(depth, intrinsics, "cuda:0", extrinsics=extrinsics, **args)
    with pytest.raises(ValueError, match=match) as theirs:
        scan.unproject_depth_views(depth, intrinsics, extrinsics, **args)
    assert str(ours.value).split(": ", 1)[1] == str(theirs.value).split(": ", 1)[1]


def test_free_space_cameras_and_fit_value_errors_before_any_device_use():
    fld = rig_field()
    plain = scan.DepthField(fld.cls[:, 0], fld.z[:, 0], fld.nearest[:, 0], fld.intrinsics[:, 0])
    with pytest.raises(ValueError, match="must be a rig field"):
        scan.free_space_cameras(plain)
    with pytest.raises(ValueError, match="pose must be a scan.Pose of 2 bodies"):
        scan.free_space_cameras(fld, scan.Pose.identity(3, "cpu"))
    with pytest.raises(ValueError, match="pose must be a scan.Pose of 2 bodies"):
        scan.free_space_cameras(fld, torch.zeros((2, 12)))
    z = torch.zeros((3, 4, 8))
    scans = scan.ScanBatch._from_parts(torch.zeros((3, 5, 3)), torch.full((3,), 5, dtype=torch.int32), np.full(3, 5), None, None)
    for fit in (editing.fit_scan, editing.register_scan):
        with pytest.raises(ValueError, match="3 bodies, a field of 2 images"):
            fit(None, z, None, scans, free_space=fld)
        with pytest.raises(ValueError, match="silhouette_weight must be >= 0"):
            fit(None, z, None, scans, free_space=rig_field(B=3), silhouette_weight=-0.5)


def test_argument_validation_without_gpu():
    """The three entry points refuse bad arguments before they touch the device."""
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)                      # `p`: not null, never dereferenced on these paths

    def cams(pose=null, ext=p, B=2, V=3, cam=p):
        return lib.sh_free_space_cameras(pose, ext, B, V, cam, null)

    for rc in (cams(ext=null), cams(cam=null)):
        assert rc == -1 and b"null pointer" in lib.sh_last_error()
    for rc in (cams(V=0), cams(V=33), cams(V=-1)):
        assert rc == -1 and b"views" in lib.sh_last_error()
    assert cams(B=-1) == -1 and b"bad size" in lib.sh_last_error()
    for rc in (cams(B=65536, V=1), cams(B=32768, V=2)):
        assert rc == -2 and b"65535" in lib.sh_last_error()
    assert cams(B=0) == 0 and cams(B=0, pose=p) == 0                        # nothing to do, nothing launched

    def fwd(x=p, x_sb=30, rows=10, n=9, cam=p, cls=p, nearest=p, intr=p, V=2, H=4, W=4, mask=null, mask_sb=0, margin=0.0, B=2, term=p, counts=p):
        return lib.sh_free_space_views_fwd(x, x_sb, rows, n, cam, cls, p, nearest, intr, V, H, W, mask, mask_sb, margin, B, term, p, p, counts, null)

    def bwd(x=p, x_sb=30, rows=10, n=9, cam=p, V=2, H=4, W=4, mask=null, mask_sb=0, margin=0.0, counts=p, gL=p, B=2, g=p):
        return lib.sh_free_space_views_bwd(x, x_sb, rows, n, cam, p, p, p, p, V, H, W, mask, mask_sb, margin, counts, gL, B, g, null)

    for rc in (fwd(x=null), fwd(cam=null), fwd(cls=null), fwd(nearest=null), fwd(intr=null), fwd(term=null), fwd(counts=null), bwd(x=null),
               bwd(cam=null), bwd(counts=null), bwd(gL=null), bwd(g=null)):
        assert rc == -1 and b"null pointer" in lib.sh_last_error()
    for rc in (fwd(V=0), fwd(V=33), bwd(V=0), bwd(V=40)):
        assert rc == -1 and b"views" in lib.sh_last_error()
    for rc in (fwd(B=-1), fwd(n=11), fwd(rows=-1, n=-1), fwd(H=-1), bwd(n=11), bwd(W=-1)):
        assert rc == -1 and b"bad size" in lib.sh_last_error()
    for rc in (fwd(margin=-1.0), fwd(margin=math.nan), bwd(margin=-0.5), bwd(margin=math.nan)):
        assert rc == -1 and b"margin" in lib.sh_last_error()
    for rc in (fwd(x_sb=26), bwd(x_sb=0)):
        assert rc == -1 and b"batch stride" in lib.sh_last_error()
    for rc in (fwd(mask=p, mask_sb=8), bwd(mask=p, mask_sb=1)):
        assert rc == -1 and b"mask stride" in lib.sh_last_error()
    for rc in (fwd(H=0), bwd(W=0)):
        assert rc == -1 and b"empty image" in lib.sh_last_error()
    for rc in (fwd(H=16385), bwd(W=20000)):
        assert rc == -2 and b"16384" in lib.sh_last_error()
    for rc in (fwd(B=65536), bwd(B=65536)):
        assert rc == -2 and b"65535" in lib.sh_last_error()
    for rc in (fwd(B=32768, V=2), bwd(B=2048, V=32), fwd(V=8, H=16384, W=16384), bwd(V=32, H=8192, W=8192)):
        assert rc == -2 and b"B * V" in lib.sh_last_error()
    assert fwd(B=0) == 0 and bwd(B=0) == 0 and bwd(rows=0, n=0) == 0       # nothing to do, nothing launched
