"""The free-space term through a lens on the GPU (sh_free_space_views_rays_fwd / _bwd) against tests/camera_ref.py: the 170-vertex
bodies of small_ae.npz before a distorted camera and before a two-camera rig with a pose - term, kind, counts and the gradient
bit for bit, the two sums to one fp32 ulp -, vertices placed by hand on every new edge of the case list, and the gradient against
central differences of the float64 restatement."""
import functools
import os

import numpy as np
import pytest
import torch

from semantichuman_amd import scan
from tests import camera_ref as C
from tests import field_ref as RF
from tests import field_views_ref as RFV
from tests.launch_record import launches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, W = C.H, C.W
GL = np.asarray([[1.0, 1.0], [0.5, -3.0]], np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.int32)


def ulp_apart(got, want64):
    want = np.float32(want64)
    return 0.0 if got == want else abs(float(got) - want64) / float(np.spacing(np.abs(want)))


@functools.lru_cache(maxsize=None)
def model():
    """The two bodies of small_ae.npz scaled to about a metre -> (x float64 [2, 171, 3], faces, n = 170)."""
    gs = np.load(os.path.join(GOLD, "small_ae.npz"))
    x = np.asarray(gs["x"], np.float64)
    size = float((x[:, :-1].max(1) - x[:, :-1].min(1)).max())
    return x / size, np.asarray(gs["faces"], np.int64), x.shape[1] - 1


def place(x, n, distance=1.25):
    """A body in front of the camera at the origin: its smallest extent along z, its largest upright (field_ref.camera_for)."""
    Rm, t, _, size = RF.camera_for(x[:n], H, W, distance=distance)
    return x @ Rm.T + t


@functools.lru_cache(maxsize=None)
def one_camera():
    """Both bodies before the AZURE camera, rendered through the lens; x is the body grown by 15 %: it overshoots silhouette and
    surface -> (depth [2, H, W], lens, x float32 [2, 171, 3], n)."""
    xs, faces, n = model()
    lens = C.Lens(C.INTR, C.AZURE, H, W)
    depth, grown = [], []
    for b in range(2):
        cam = place(xs[b], n)
        depth.append(C.render_mesh(cam[:n], faces, lens, H, W, background=9.0))
        centre = cam[:n].mean(0)
        grown.append(((cam - centre) * 1.15 + centre).astype(np.float32))
    return np.stack(depth), lens, np.stack(grown), n


Z_RANGE = (0.3, 5.0)


def compare(got, ref, n):
    term, kind, loss, counts, gx = got
    for b, (t, k, c, g, L) in enumerate(ref):
        assert np.array_equal(kind[b], k), "kind of body %d" % b
        assert np.array_equal(counts[b], c), "counts of body %d" % b
        assert np.array_equal(bits(term[b]), bits(t)), "term of body %d" % b
        assert np.array_equal(bits(gx[b]), bits(g)), "gradient of body %d" % b
        assert (gx[b, n:] == 0).all()
        # an fp64 sum of fewer than 2^13 fp32 terms is exact to far below half an fp32 ulp: only the final rounding can differ
        assert ulp_apart(loss[b, 0], L[0]) <= 1.0 and ulp_apart(loss[b, 1], L[1]) <= 1.0, (loss[b], L)


def run(x, field, gL, **kw):
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    (free, sil), rec = launches(lambda: scan.free_space(xd, field, **kw))
    _, rec_b = launches(lambda: (free * torch.from_numpy(gL[:, 0]).to(DEV) + sil * torch.from_numpy(gL[:, 1]).to(DEV)).sum().backward())
    kind, counts = scan.free_space_kinds(xd, field, **kw)
    cam = None if field.views is None else scan.free_space_cameras(field, kw.get("pose"))
    term, kind2, loss, _ = scan._free_space_fwd(xd.detach(), field, cam, kw.get("n", x.shape[1] - 1), None, 0, 0.0)    # the term plane itself
    assert torch.equal(kind2, kind) and torch.equal(loss, torch.stack([free, sil], 1))
    return free, sil, kind.cpu().numpy(), counts.cpu().numpy(), xd.grad.cpu().numpy(), [k for k, _ in rec + rec_b], term.cpu().numpy()


def test_one_camera_bits():
    depth, lens, x, n = one_camera()
    field = scan.DepthField.from_depth(depth, C.INTR, DEV, z_range=Z_RANGE, distortion=C.AZURE)
    assert field.rays is not None and field.rays.complete and field.views is None
    refs = [RF.field(depth[b], C.INTR, z_range=Z_RANGE) for b in range(2)]
    for b in range(2):
        assert np.array_equal(field.cls[b].cpu().numpy(), refs[b].cls) and np.array_equal(field.nearest[b].cpu().numpy(), refs[b].nearest)
    free, sil, kind, counts, gx, names, term = run(x, field, GL)
    assert names[-2:] == ["free_space_views_rays_fwd_kernel", "free_space_views_rays_bwd_kernel"]
    ref = []
    for b in range(2):
        t, k, g, c = C.terms(x[b], n, refs[b], lens)
        ref.append((t, k, c, RF.gradient(k, g, c, GL[b], x.shape[1]), RF.losses(t, k, c)))
        assert (k == RF.FREE).sum() >= 10 and (k == RF.SILHOUETTE).sum() >= 10
    loss = torch.stack([free, sil], 1).detach().cpu().numpy()
    compare((term, kind, loss, counts, gx), ref, n)
    for b in range(2):                                                     # a body alone: the same bits
        f1 = scan.DepthField.from_depth(depth[b], C.INTR, DEV, z_range=Z_RANGE, distortion=field.rays)
        _, _, k1, c1, g1, _, _ = run(x[b:b + 1], f1, GL[b:b + 1])
        assert np.array_equal(k1[0], kind[b]) and np.array_equal(c1[0], counts[b]) and np.array_equal(bits(g1[0]), bits(gx[b]))
    sel = field.select(slice(1, 2))                                        # a shared table survives a cut of the bodies
    _, _, k2, _, g2, _, _ = run(x[1:2], sel, GL[1:2])
    assert np.array_equal(k2[0], kind[1]) and np.array_equal(bits(g2[0]), bits(gx[1]))


def test_rig_with_a_pose_bits():
    """Two cameras (AZURE, BARREL) to the left and right of the bodies, and a pose between the rig's frame and the model's."""
    xs, faces, n = model()
    intr = np.asarray([C.INTR, (27.0, 28.5, 18.0, 14.25)], np.float32)
    lenses = [C.Lens(intr[0], C.AZURE, H, W), C.Lens(intr[1], C.BARREL, H, W)]
    rng = np.random.default_rng(7)
    exts = []
    for angle in (0.35, -0.3):
        Ry = np.asarray([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]])
        centre = np.asarray([0.0, 0.0, 1.25])
        exts.append(RFV.pack(Ry, centre - Ry @ centre).reshape(12))       # the camera swung about the body's centre
    ext = np.stack([np.stack(exts)] * 2).astype(np.float32)
    Rp, tp = RFV.rigid(rng, spread=0.05)
    w = 0.05 * rng.standard_normal(3)
    Rp = np.eye(3) + np.asarray([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])                  # near the identity; A need not be a rotation
    pose = np.stack([RFV.pack(Rp, tp)] * 2)
    depth, x = np.zeros((2, 2, H, W), np.float32), []
    for b in range(2):
        rig_pts = place(xs[b], n)                                          # the body in the rig's frame
        for v in range(2):
            e = ext[b, v].astype(np.float64)
            cam_pts = (rig_pts - e[9:]) @ e[:9].reshape(3, 3)              # R^T (P - t)
            depth[b, v] = C.render_mesh(cam_pts[:n], faces, lenses[v], H, W, background=9.0)
        centre = rig_pts[:n].mean(0)
        grown = (rig_pts - centre) * 1.15 + centre
        x.append((grown @ Rp.T + tp).astype(np.float32))                   # in the model's frame: pose maps rig -> model
    x = np.stack(x)
    dist = np.stack([l.d for l in lenses])
    ext34 = ext.reshape(2, 2, 12)
    ext34 = np.concatenate([ext34[..., :9].reshape(2, 2, 3, 3), ext34[..., 9:, None]], -1)
    field = scan.DepthField.from_depth(depth, intr, DEV, extrinsics=ext34, z_range=Z_RANGE, distortion=dist)
    assert field.views == 2 and field.rays.lead == (2,)
    p = scan.Pose.from_packed(torch.from_numpy(pose).to(DEV), torch.ones(2, device=DEV))
    free, sil, kind, counts, gx, names, term = run(x, field, GL, pose=p)
    assert names == ["free_space_cameras_kernel", "free_space_views_rays_fwd_kernel", "free_space_views_rays_bwd_kernel"]
    ref = []
    for b in range(2):
        fields = [RF.field(depth[b, v], intr[v], z_range=Z_RANGE) for v in range(2)]
        cam = RFV.cameras(pose[b], ext[b])
        t, k, g, c = C.terms_views(x[b], n, fields, lenses, cam)
        ref.append((t, k, c, RFV.gradient(k, g, c, GL[b], x.shape[1], cam), RFV.losses(t, k, c)))
        assert all((k[v] == RF.FREE).sum() >= 5 and (k[v] == RF.SILHOUETTE).sum() >= 5 for v in range(2))
    compare((term, kind, torch.stack([free, sil], 1).detach().cpu().numpy(), counts, gx), ref, n)


def test_hand_placed_vertices():
    """The new edges of the case list under the FOLDING lens, whose table is incomplete: a vertex in the fold-back zone (its
    polynomial projection is inside the image), two in the half-pixel border (one on either side of it), one behind the camera,
    one onto an EMPTY pixel whose nearest pixel that is not EMPTY has no ray, one onto an EMPTY pixel with an ordinary neighbour."""
    lens = C.Lens(C.INTR, C.FOLDING, H, W)
    has = lens.has_ray()
    cls = np.zeros((H, W), np.uint8)
    assert not has[14, 0] and has[14, 3] and has[14, 18] and has[14, 15]
    cls[14, 0] = cls[14, 18] = RF.SURFACE                                  # allowed pixels: one without a ray, one with
    f = RF.field_of_classes(cls, C.INTR, z=np.full((H, W), 0.5))
    assert f.nearest[14, 3] == 14 * W and f.nearest[14, 15] == 14 * W + 18
    Z = 2.0
    bx, by, ok = C.invert(C.INTR, lens.d, [18.0, 18.0], [-0.3, -0.7])      # either side of the image's upper edge
    assert ok.all()
    ray = lambda u, v: lens.table[v, u].astype(np.float64)                 # noqa: E731
    x = np.asarray([[1.2 * Z, 0.0, Z], [bx[0] * Z, by[0] * Z, Z], [bx[1] * Z, by[1] * Z, Z], [0.1, 0.1, -1.0],
                    list(ray(3, 14) * Z) + [Z], list(ray(15, 14) * Z * 1.01) + [Z], [0.0, 0.0, 0.0]], np.float32)[None]
    n = 6
    t, k, g, c = C.terms(x[0], n, f, lens)
    # the second vertex is inside through the border: pixel (18, 0), EMPTY, and its nearest allowed pixel (18, 14) has a ray
    assert k.tolist() == [RF.OUTSIDE, RF.SILHOUETTE, RF.OUTSIDE, RF.OUTSIDE, RF.NONE, RF.SILHOUETTE]
    uf, vf, inside, u, v = C.project(x[0, :n], lens.intr, lens.d, lens.limit, H, W)
    assert -0.5 <= uf[0] < W - 0.5 and not inside[0]                       # folded back into the image, kept out by the limit
    assert inside[1] and v[1] == 0 and -0.5 <= vf[1] < 0 and vf[2] < -0.5  # pixel row 0 through the border; beyond it
    assert (u[4], v[4]) == (3, 14) and (u[5], v[5]) == (15, 14)
    cr = scan.camera_rays(C.INTR, C.pad8(C.FOLDING), (H, W), DEV)
    planes = [torch.from_numpy(a[None]).to(DEV) for a in (f.cls, f.z, f.nearest)]
    field = scan.DepthField(*planes, torch.from_numpy(np.asarray(C.INTR, np.float32)[None]).to(DEV), rays=cr, rays_lead=(1,))
    gL = np.asarray([[2.0, 0.5]], np.float32)
    free, sil, kind, counts, gx, _, term = run(x, field, gL, n=n)
    ref = [(t, k, c, RF.gradient(k, g, c, gL[0], x.shape[1]), RF.losses(t, k, c))]
    compare((term, kind, torch.stack([free, sil], 1).detach().cpu().numpy(), counts, gx), ref, n)


def test_gradient_against_central_differences():
    """The gradient of the one-camera scene against central differences of the float64 restatement, for the charged vertices whose
    kind and pixel stay as they are under the step - at least half of them.  The terms are quadratics in the vertex (the pixel,
    the nearest pixel and the ray are constants), so the central difference is exact up to float64 rounding, 1e-16 / h; the fp32
    gradient 2 s r, r = X - a Z, carries the rounding of r: at most 3 * 2^-24 (|X| + |a Z|), times (1 + |a| + |b|) in the z
    component, plus the roundings of the products: 8 * 2^-24 of the word itself."""
    depth, lens, x, n = one_camera()
    field = scan.DepthField.from_depth(depth, C.INTR, DEV, z_range=Z_RANGE, distortion=C.AZURE)
    ones = np.ones((2, 2), np.float32)
    _, _, kind, counts, gx, _, _ = run(x, field, ones)
    h, u24 = 1e-6, 2.0 ** -24
    for b in range(2):
        f = RF.field(depth[b], C.INTR, z_range=Z_RANGE)
        x0 = x[b].astype(np.float64)
        free0, sil0, kind0, pix0, n_act = C.terms64(x0, n, f, lens)
        charged = np.flatnonzero(kind0 != RF.NONE)
        assert np.array_equal(kind0[charged], kind[b][charged])
        num = np.zeros((n, 3))
        stable = np.ones(n, bool)
        for axis in range(3):
            per = []
            for sign in (1.0, -1.0):
                xs = x0.copy()
                xs[:n, axis] += sign * h
                fr, si, kd, px, _ = C.terms64(xs, n, f, lens)
                stable &= (kd == kind0) & (px == pix0)
                per.append(fr + si)
            num[:, axis] = (per[0] - per[1]) / (2 * h) / n_act
        ok = charged[stable[charged]]
        assert 2 * len(ok) >= len(charged) and len(ok) >= 20
        scale = np.abs(x0[ok]).sum(1)
        bound = (2.0 / n_act) * 3 * u24 * 2 * scale * 3.5 + 8 * u24 * np.abs(num[ok]).max(1) + 2 * 1e-16 / h / n_act
        assert (np.abs(gx[b][ok] - num[ok]).max(1) <= bound).all(), (np.abs(gx[b][ok] - num[ok]).max(1) / bound).max()
