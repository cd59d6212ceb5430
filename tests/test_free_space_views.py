"""The rig form of the free-space term on the GPU (sh_free_space_cameras, sh_free_space_views_fwd / _bwd) against
tests/field_views_ref.py: cam, term, kind, counts and the gradient bit for bit, the two loss values to one fp32 ulp of the exact
sum; against the one-view kernels (identity cameras, and per view on the transformed vertices); batches against single bodies;
the plumbing into scan.free_space, editing.fit_scan and editing.register_scan by their launch lists; and the two-view fit."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import editing, ops, scan
from tests import depth_ref as D
from tests import field_ref as R
from tests import field_views_ref as RV
from tests.launch_record import launch_counts, launches
from tests.test_free_space import DEV, bits, bodies, fields, model_scene, ulp_apart

pytestmark = pytest.mark.gpu
GL = np.asarray([[1.0, 1.0], [0.5, -3.0], [2.0, 0.25]], np.float32)


@functools.lru_cache(maxsize=None)
def big_fields():
    """Three fields of 48 x 80 from the scenes of tests/depth_ref.py and a constructed tie mask embedded in an EMPTY image."""
    out = []
    for seed in (1, 2):
        depth, intr = D.scene(48, 80, seed=seed)
        out.append(R.field(depth, intr, z_range=(0.5, 1.9) if seed == 1 else D.Z_RANGE))
    cls = np.zeros((48, 80), np.uint8)
    cls[20:33, 30:43] = R.tie_masks()["row_tie"]
    cls[3:8, 60:65] = R.tie_masks()["corners"]
    out.append(R.field_of_classes(cls, out[0].intr, z=np.full((48, 80), 1.5)))
    return out


def small_move(rng, angle=0.08, shift=0.05):
    """A rigid move near the identity -> the 12 words of an extrinsic: the bodies stay in front of the camera and mostly in the image."""
    w = angle * rng.standard_normal(3)
    K = np.asarray([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = np.linalg.norm(w)
    Rm = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    return RV.pack(Rm, shift * rng.standard_normal(3))


def rig(refs, V, seed, absent=True):
    """B = 3 bodies x V views: view v of body b is field (b + v) % 3; camera 0 is the identity (the special rows of the bodies
    hit every case there), the others small rigid moves; with `absent`, camera 1 of body 1 is a NaN row among live ones."""
    rng = np.random.default_rng(seed)
    ext = np.stack([np.stack([RV.IDENTITY if v == 0 else small_move(rng) for v in range(V)]) for _ in range(3)])
    if absent and V >= 2:
        ext[1, 1] = np.nan
    cam = np.stack([RV.cameras(None, e) for e in ext])
    return [[refs[(b + v) % 3] for v in range(V)] for b in range(3)], ext, cam


def device_field(views, ext, sel=slice(None)):
    planes = [torch.from_numpy(np.stack([np.stack([getattr(f, k) for f in body]) for body in views[sel]])).to(DEV) for k in ("cls", "z", "nearest", "intr")]
    return scan.DepthField(*planes, torch.from_numpy(np.ascontiguousarray(ext[sel])).to(DEV))


def reference(x, n, views, cam, masks, margin, gL):
    out = []
    for b, body in enumerate(views):
        term, kind, g, counts = RV.terms(x[b], n, body, cam[b], None if masks is None else masks[b], margin)
        out.append((term, kind, counts, RV.gradient(kind, g, counts, gL[b], x.shape[1], cam[b]), RV.losses(term, kind, counts)))
    return out


def run(x, n, fld, cam, mask, margin, gL):
    """The library on device tensors -> (term, kind, loss, counts, g_x) as numpy: ops for the outputs, the autograd function of
    scan.free_space(cameras=) for the gradient, scan.free_space_kinds in passing."""
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    camd = torch.from_numpy(np.ascontiguousarray(cam)).to(DEV)
    v_mask, mask_sb = ops._mask_arg(None if mask is None else torch.from_numpy(mask), x.shape[0], n, DEV)
    term, kind, loss, counts = ops.free_space_views_fwd(xd.detach(), n, camd, fld.cls, fld.z, fld.nearest, fld.intrinsics, v_mask, mask_sb, margin)
    vm = None if mask is None else torch.from_numpy(mask).to(DEV)
    free, sil = scan.free_space(xd, fld, n=n, vertex_mask=vm, margin=margin, cameras=camd)
    assert torch.equal(torch.stack([free, sil], 1), loss)
    (free * torch.from_numpy(gL[:, 0]).to(DEV) + sil * torch.from_numpy(gL[:, 1]).to(DEV)).sum().backward()
    kinds, counts2 = scan.free_space_kinds(xd, fld, n=n, vertex_mask=vm, margin=margin, cameras=camd)
    assert torch.equal(kinds, kind) and torch.equal(counts2, counts)
    return term.cpu().numpy(), kind.cpu().numpy(), loss.cpu().numpy(), counts.cpu().numpy(), xd.grad.cpu().numpy()


def compare(got, ref, n):
    term, kind, loss, counts, gx = got
    for b, (t, k, c, g, L) in enumerate(ref):
        assert np.array_equal(kind[b], k), "kind of body %d" % b
        assert np.array_equal(counts[b], c), "counts of body %d" % b
        assert np.array_equal(bits(term[b]), bits(t)), "term of body %d" % b
        assert np.array_equal(bits(gx[b]), bits(g)), "gradient of body %d" % b
        assert (gx[b, n:] == 0).all()
        # an fp64 sum of fewer than 2^15 fp32 terms is exact to far below half an fp32 ulp: only the final rounding can differ
        assert ulp_apart(loss[b, 0], L[0]) <= 1.0 and ulp_apart(loss[b, 1], L[1]) <= 1.0, (loss[b], L)


def masks_for(masked, n, rng):
    mask = None if masked is None else (rng.random(n) > 0.2) if masked == "n" else (rng.random((3, n)) > 0.2)
    if masked == "Bn":
        mask[1] = n < 256                                                  # a body without an active vertex: zeros, n_act == 0
    return mask, None if mask is None else np.broadcast_to(mask, (3, n))


@pytest.mark.parametrize("n, rows", [(1, 2), (255, 256), (256, 257), (257, 257), (600, 601)])
@pytest.mark.parametrize("V", [1, 2, 3])
@pytest.mark.parametrize("margin, masked", [(0.0, None), (0.03125, "n"), (0.01, "Bn")])
def test_bits_against_the_reference(n, rows, V, margin, masked):
    views, ext, cam = rig(fields(), V, seed=10 * V + 1)
    x = bodies(n, rows, margin, seed=n)
    mask, masks = masks_for(masked, n, np.random.default_rng(n + 1))
    got = run(x, n, device_field(views, ext), cam, mask, margin, GL)
    ref = reference(x, n, views, cam, masks, margin, GL)
    compare(got, ref, n)
    if n >= 255 and masked is None:                                        # every case is there, in the first view and beyond it
        assert set(np.concatenate([k[0] for _, k, _, _, _ in ref]).tolist()) == {0, 1, 2, 3, 4}
        if V >= 2:
            assert {1, 2, 4} <= set(np.concatenate([k[1:].ravel() for _, k, _, _, _ in ref]).tolist())
            assert (ref[1][1][1] == R.OUTSIDE).all() and ref[1][2][1].tolist() == [n, 0, 0, n]   # the absent camera


def test_thirty_two_views_and_the_larger_image():
    n, rows = 300, 301
    for refs, V, margin in ((fields(), 32, 0.01), (big_fields(), 2, 0.0), (big_fields(), 3, 0.03125)):
        views, ext, cam = rig(refs, V, seed=V)
        hh, ww = refs[0].cls.shape
        rng = np.random.default_rng(V)
        x = np.zeros((3, rows, 3), np.float32)
        for b in range(3):
            fx, fy, cx, cy = (float(t) for t in refs[b].intr)
            u, v, Z = rng.uniform(-2.0, ww + 1.0, rows), rng.uniform(-2.0, hh + 1.0, rows), rng.uniform(1.0, 2.2, rows)
            x[b] = np.stack([(u - cx) / fx * Z, (v - cy) / fy * Z, Z], 1)
        mask, masks = masks_for("n", n, rng)
        got = run(x, n, device_field(views, ext), cam, mask, margin, GL)
        ref = reference(x, n, views, cam, masks, margin, GL)
        compare(got, ref, n)
        assert {1, 2} <= set(np.concatenate([k.ravel() for _, k, _, _, _ in ref]).tolist())


def test_a_body_alone_permuted_and_in_a_wider_batch():
    n, rows, V, margin = 600, 601, 3, 0.01
    views, ext, cam = rig(fields(), V, seed=4)
    x = bodies(n, rows, margin, seed=9)
    mask, masks = masks_for("Bn", n, np.random.default_rng(2))
    whole = run(x, n, device_field(views, ext), cam, mask, margin, GL)
    for b in range(3):
        alone = run(x[b:b + 1], n, device_field(views, ext, slice(b, b + 1)), cam[b:b + 1], masks[b:b + 1].copy(), margin, GL[b:b + 1])
        for a, w in zip(alone, whole):
            assert np.array_equal(bits(a[0]), bits(w[b]))
    order = [2, 0, 1]
    perm = run(x[order], n, device_field([views[b] for b in order], ext[order]), cam[order], masks[order].copy(), margin, GL[order])
    for a, w in zip(perm, whole):
        assert np.array_equal(bits(a), bits(w[order]))
    wide = np.full((3, rows + 37, 3), 5.0, np.float32)                     # more padding rows, and a batch stride that is not the body's
    wide[:, :rows] = x
    wider = run(wide, n, device_field(views, ext), cam, mask, margin, GL)
    for k in range(4):
        assert np.array_equal(bits(wider[k]), bits(whole[k]))
    assert np.array_equal(bits(wider[4][:, :rows]), bits(whole[4])) and (wider[4][:, n:] == 0).all()


def test_one_identity_camera_is_the_one_view_kernel():
    refs = fields()
    fld1 = scan.DepthField(*(torch.from_numpy(np.stack([getattr(r, k) for r in refs])).to(DEV) for k in ("cls", "z", "nearest", "intr")))
    for n, rows, margin in ((257, 257, 0.0), (600, 601, 0.03125)):
        views, ext, cam = rig(refs, 1, seed=0)
        assert (cam == RV.IDENTITY).all()
        x = bodies(n, rows, margin, seed=n)
        mask, _ = masks_for("Bn", n, np.random.default_rng(n))
        got = run(x, n, device_field(views, ext), cam, mask, margin, GL)
        xd = torch.from_numpy(x).to(DEV)
        v_mask, mask_sb = ops._mask_arg(torch.from_numpy(mask), 3, n, DEV)
        one = ops.free_space_fwd(xd, n, fld1.cls, fld1.z, fld1.nearest, fld1.intrinsics, v_mask, mask_sb, margin)
        g1 = ops.free_space_bwd(xd, n, fld1.cls, fld1.z, fld1.nearest, fld1.intrinsics, v_mask, mask_sb, margin, one[3], torch.from_numpy(GL).to(DEV))
        term, kind, loss, counts = (t.cpu().numpy() for t in one)
        assert np.array_equal(bits(got[0][:, 0]), bits(term)) and np.array_equal(got[1][:, 0], kind) and np.array_equal(got[3][:, 0], counts)
        assert np.array_equal(bits(got[2]), bits(loss)) and np.array_equal(bits(got[4]), bits(g1.cpu().numpy()))


def test_every_view_is_the_one_view_kernel_on_the_transformed_vertices():
    n, rows, V, margin = 600, 601, 3, 0.01
    refs = fields()
    rng = np.random.default_rng(8)
    views = [[refs[(b + v) % 3] for v in range(V)] for b in range(3)]
    ext = np.stack([np.stack([small_move(rng, 0.15, 0.1) for _ in range(V)]) for _ in range(3)])
    pose = np.stack([RV.pack(rng.uniform(0.7, 1.4) * RV.rigid(rng)[0], 0.1 * rng.standard_normal(3)) for _ in range(3)])
    cam = np.stack([RV.cameras(pose[b], ext[b]) for b in range(3)])
    P = scan.Pose.from_packed(torch.from_numpy(pose).to(DEV), torch.ones(3, device=DEV))
    x = P.apply(torch.from_numpy(bodies(n, rows, margin, seed=6)).to(DEV)).cpu().numpy()       # the bodies in a model frame
    mask, _ = masks_for("n", n, rng)
    got = run(x, n, device_field(views, ext), cam, mask, margin, GL)
    v_mask, mask_sb = ops._mask_arg(torch.from_numpy(mask), 3, n, DEV)
    for v in range(V):
        moved = np.stack([np.concatenate([RV.transform(x[b, :n], cam[b, v]), x[b, n:]]) for b in range(3)])
        f = scan.DepthField(*(torch.from_numpy(np.stack([getattr(views[b][v], k) for b in range(3)])).to(DEV) for k in ("cls", "z", "nearest", "intr")))
        term, kind, _, counts = ops.free_space_fwd(torch.from_numpy(moved).to(DEV), n, f.cls, f.z, f.nearest, f.intrinsics, v_mask, mask_sb, margin)
        assert np.array_equal(bits(got[0][:, v]), bits(term.cpu().numpy())) and np.array_equal(got[1][:, v], kind.cpu().numpy())
        assert np.array_equal(got[3][:, v], counts.cpu().numpy())
    assert {1, 2} <= set(got[1].ravel().tolist())


def test_cameras_bitwise():
    rng = np.random.default_rng(21)
    B, V = 5, 4
    ext = np.stack([np.stack([RV.pack(*RV.rigid(rng, 1.0)) for _ in range(V)]) for _ in range(B)])
    ext[2, 1] = np.nan                                                     # an absent camera
    ext[0, 0] = RV.IDENTITY
    pose = np.stack([RV.pack(rng.uniform(0.5, 2.0) * RV.rigid(rng)[0], rng.standard_normal(3)) for _ in range(B)])
    pose[3] = [1, 2, 3, 2, 4, 6, 0, 0, 1, 0.5, 0.5, 0.5]                   # a singular A
    extd, posed = torch.from_numpy(ext).to(DEV), torch.from_numpy(pose).to(DEV)
    for p, pd in ((pose, posed), (None, None)):
        want = np.stack([RV.cameras(None if p is None else p[b], ext[b]) for b in range(B)])
        cam, rec = launches(lambda: ops.free_space_cameras(extd, pd))
        assert [k for k, _ in rec] == ["free_space_cameras_kernel"]
        got = cam.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(np.nan_to_num(got)), bits(np.nan_to_num(want)))
        assert np.isnan(got[2, 1]).all() and (p is None or np.isnan(got[3]).all()) and np.isfinite(got[[0, 1, 4]]).all()
    assert np.array_equal(got[0, 0], RV.IDENTITY)


# ------------------------------------------------------------------------------------------------ plumbing
def test_scan_free_space_on_a_rig_field():
    """DepthField.from_depth(extrinsics=) is the one-view field per image; scan.free_space computes the cameras itself (one launch)
    and equals the call with cameras= given; the pose enters through the cameras and scale^2; the new ValueErrors."""
    refs, x, n = model_scene()                                             # two bodies of 170 vertices, 64 x 48
    hh, ww = refs[0].cls.shape
    rng = np.random.default_rng(5)
    depth = np.stack([np.stack([np.where(r.cls == R.SURFACE, r.z, np.float32(50.0)) for r in (refs[b], refs[1 - b])]) for b in range(2)])
    intr = np.stack([np.stack([r.intr for r in (refs[b], refs[1 - b])]) for b in range(2)])
    ext = np.stack([np.stack([RV.IDENTITY, small_move(rng, 0.05, 0.02)]) for _ in range(2)])
    z_range = (0.1, 40.0)
    matrices = np.concatenate([ext[..., :9].reshape(2, 2, 3, 3), ext[..., 9:, None]], -1)              # [B, V, 3, 4] = (R | t)
    fld = scan.DepthField.from_depth(depth, intr, DEV, extrinsics=matrices, z_range=z_range)
    assert fld.views == 2 and len(fld) == 2 and fld.shape == (hh, ww) and tuple(fld.cls.shape) == (2, 2, hh, ww)
    assert np.array_equal(fld.extrinsics.cpu().numpy(), ext) and tuple(fld.intrinsics.shape) == (2, 2, 4)
    for v in range(2):
        one = scan.DepthField.from_depth(depth[:, v], intr[:, v], DEV, z_range=z_range)
        assert torch.equal(one.cls, fld.cls[:, v]) and torch.equal(one.z, fld.z[:, v]) and torch.equal(one.nearest, fld.nearest[:, v])
    views = [[R.field(depth[b, v], intr[b, v], z_range=z_range) for v in range(2)] for b in range(2)]
    A = np.stack([RV.rigid(rng)[0] * s for s in (0.7, 1.9)])
    pose = scan.Pose(torch.from_numpy(A.astype(np.float32)).to(DEV), torch.from_numpy(rng.standard_normal((2, 3)).astype(np.float32)).to(DEV))
    model = pose.apply(torch.from_numpy(x).to(DEV)).requires_grad_(True)
    (free, sil), rec = launches(lambda: scan.free_space(model, fld, pose=pose, margin=0.01))
    assert [k for k, _ in rec] == ["free_space_cameras_kernel", "free_space_views_fwd_kernel"]
    _, rec = launches(lambda: (free + 2 * sil).sum().backward())
    assert [k for k, _ in rec] == ["free_space_views_bwd_kernel"]
    cam = scan.free_space_cameras(fld, pose)
    want = np.stack([RV.cameras(pose.packed[b].cpu().numpy(), ext[b]) for b in range(2)])
    assert np.array_equal(bits(cam.cpu().numpy()), bits(want))
    again = model.detach().clone().requires_grad_(True)
    (f2, s2), rec = launches(lambda: scan.free_space(again, fld, pose=pose, margin=0.01, cameras=cam))
    assert [k for k, _ in rec] == ["free_space_views_fwd_kernel"]
    (f2 + 2 * s2).sum().backward()
    assert torch.equal(free, f2) and torch.equal(sil, s2) and torch.equal(model.grad, again.grad) and not pose.packed.requires_grad
    xm = model.detach().cpu().numpy()
    s2c = (pose.scale * pose.scale).cpu().numpy()                          # fp32, as scan.free_space forms it
    kind, counts = scan.free_space_kinds(model, fld, pose=pose, margin=0.01)
    assert tuple(kind.shape) == (2, 2, n) and tuple(counts.shape) == (2, 2, 4)
    for b in range(2):
        t, k, g, c = RV.terms(xm[b], n, views[b], want[b], None, 0.01)
        L = RV.losses(t, k, c)
        assert np.array_equal(kind[b].cpu().numpy(), k) and np.array_equal(counts[b].cpu().numpy(), c) and c[0][1] > 10 and c[0][2] > 10
        assert ulp_apart(free[b].item() / float(s2c[b]), L[0]) <= 2.0 and ulp_apart(sil[b].item() / float(s2c[b]), L[1]) <= 2.0   # one more rounding: * scale^2
        gx = RV.gradient(k, g, c, (s2c[b], np.float32(2) * s2c[b]), xm.shape[1], want[b])
        assert np.array_equal(bits(model.grad[b].cpu().numpy()), bits(gx))
    with pytest.raises(ValueError, match="2 bodies, a field of 1 images"):
        scan.free_space(model, fld.select(slice(0, 1)))
    with pytest.raises(ValueError, match=r"cameras must be an fp32 tensor \[2, 2, 12\]"):
        scan.free_space(model, fld, cameras=cam[:, :1])
    with pytest.raises(ValueError, match="cameras must be"):
        scan.free_space_kinds(model, fld, cameras=cam.double())
    with pytest.raises(ValueError, match="cameras= goes with a rig field"):
        scan.free_space(model, scan.DepthField(fld.cls[:, 0], fld.z[:, 0], fld.nearest[:, 0], fld.intrinsics[:, 0]), cameras=cam)


@functools.lru_cache(maxsize=None)
def two_views():
    """tests/test_free_space_fit.setup's model, start and front cameras, plus a camera behind every body (the front camera turned
    half round about the body's upright axis through its centre): the rig's frame is the front camera's, so the front extrinsic
    is the identity and `pose` (front camera -> model) is the rig's pose.  -> the rig field, the rig scans in the model's frame,
    and per body the two float64 (R | t) model -> camera maps and the two reference fields."""
    from tests.test_free_space_fit import H as hh, W as ww, setup
    from semantichuman_amd.hierarchy import load_hierarchy
    from tests.test_scan import GOLD, semantic_setup
    import os
    m, z0, z_kps, dummy, n, field, pose, in_camera, scans, cams, refs = setup()
    x_star = semantic_setup()[5].cpu().numpy().astype(np.float64)
    faces = np.asarray(load_hierarchy(os.path.join(GOLD, "semantic.npz")).faces, np.int64)
    z_range = (0.5 * min(c[3] for c in cams), 5.0 * max(c[3] for c in cams))
    S = np.diag([-1.0, 1.0, -1.0])
    depth, intr, ext, maps, fields2 = [], [], [], [], []
    for b, (Rm, tc, k, size) in enumerate(cams):
        far = np.asarray([0.0, 0.0, 2.5 * size])
        Rb, tb = S @ Rm, S @ (tc - far) + far
        back = R.render(x_star[b, :n] @ Rb.T + tb, faces, k, hh, ww, background=10.0 * size)
        front = R.render(x_star[b, :n] @ Rm.T + tc, faces, k, hh, ww, background=10.0 * size)
        depth.append(np.stack([front, back])), intr.append(np.stack([k, k]))
        ext.append(np.stack([np.eye(3, 4), np.concatenate([S, (tc - S @ tb)[:, None]], 1)]))     # back camera -> front camera
        maps.append(((Rm, tc), (Rb, tb)))
        fields2.append([R.field(front, k, z_range=z_range), R.field(back, k, z_range=z_range)])
    depth, intr, ext = np.stack(depth), np.asarray(intr, np.float32), np.stack(ext)
    rig_field = scan.DepthField.from_depth(depth, intr, DEV, extrinsics=ext, z_range=z_range)
    rig_scans = pose.apply(scan.ScanBatch.from_depth(depth, intr, DEV, extrinsics=ext, z_range=z_range))
    return m, z0, z_kps, dummy, n, field, rig_field, pose, scans, rig_scans, maps, fields2, in_camera


def test_fits_launch_the_rig_kernels_and_nothing_else_new():
    from tests.test_scan import PARTS
    m, z0, z_kps, dummy, n, field, rig_field, pose, scans, _, _, _, in_camera = two_views()
    steps = 4
    kw = dict(parts=PARTS, steps=steps, lr=1e-2, trunc=1.0, dummy=dummy)
    new = ("free_space_cameras_kernel", "free_space_views_fwd_kernel", "free_space_views_bwd_kernel")
    plain, rec_plain = launches(lambda: editing.fit_scan(m, z0, z_kps, scans, **kw))
    with_rig, rec_rig = launches(lambda: editing.fit_scan(m, z0, z_kps, scans, free_space=rig_field, free_space_pose=pose, **kw))
    names = [k for k, _ in rec_rig]
    assert [r for r in rec_rig if r[0] not in new] == rec_plain               # the plain list, in order, plus:
    assert [names.count(k) for k in new] == [1, steps, steps] and names.index(new[0]) < names.index(new[1])
    assert not torch.equal(plain[2], with_rig[2])
    _, rec_one = launches(lambda: editing.fit_scan(m, z0, z_kps, scans, free_space=field, free_space_pose=pose, **kw))
    assert not any(k in new for k, _ in rec_one) and [k for k, _ in rec_one].count("free_space_fwd_kernel") == steps

    def objective(x_hat):                                                      # the steps are the objective written by hand
        free, silhouette = scan.free_space(x_hat, rig_field, pose=pose)
        return scan.chamfer(x_hat, scans, trunc=1.0) + (free + silhouette)

    zh, lh = editing.fit_latents(m, z0, z_kps, objective, PARTS, steps=steps, lr=1e-2, dummy=dummy)
    assert torch.equal(lh, with_rig[2]) and torch.equal(zh, with_rig[0])
    kw.update(mode="rigid", init=pose, align_iters=1)
    for every, updates in ((1, steps), (2, steps // 2), (0, 0)):
        _, counts = launch_counts(lambda: editing.register_scan(m, z0, z_kps, in_camera, free_space=rig_field, align_every=every, **kw))
        assert [counts.get(k, 0) for k in new] == [1 + updates, steps, steps], every   # stage 1's pose, then one per pose update


def test_two_view_fit_with_the_term():
    """The one-view experiment of tests/test_free_space_fit.py with a second camera behind every body, through the rig field: scan
    -> model only from the 1.3x start on the rig's scans, 60 steps, both weights 30, with and without the term; free + silhouette
    of the final bodies summed over both cameras by the float64 reference.  Measured: see DESIGN 4z.  Asserted: the direction -
    lower on every body - and a Chamfer value within 1.1 times the plain fit's."""
    from tests.test_free_space_fit import CHAMFER_FACTOR, WEIGHT
    from tests.test_scan import PARTS
    m, z0, z_kps, dummy, n, _, rig_field, pose, _, rig_scans, maps, fields2, _ = two_views()
    kw = dict(parts=PARTS, steps=60, lr=1e-2, trunc=1.0, dummy=dummy)
    plain = editing.fit_scan(m, z0, z_kps, rig_scans, **kw)
    term = editing.fit_scan(m, z0, z_kps, rig_scans, free_space=rig_field, free_space_pose=pose, free_space_weight=WEIGHT, silhouette_weight=WEIGHT,
                            **kw)

    def violation(z):
        with torch.no_grad():
            x = m.decode(z, z_kps, dummy).cpu().numpy().astype(np.float64)
        return [sum(sum(R.losses64(x[b] @ Rc.T + tc, n, fields2[b][v])) for v, (Rc, tc) in enumerate(maps[b])) for b in range(3)]

    v_start, v_plain, v_term = violation(z0), violation(plain[0]), violation(term[0])
    print("two views, violation (free + silhouette): start %s  plain fit %s  with the term %s" % (v_start, v_plain, v_term))
    print("two views, chamfer: plain fit %s  with the term %s" % (plain[1].tolist(), term[1].tolist()))
    for b in range(3):
        assert v_term[b] < v_plain[b]
        assert term[1][b].item() <= CHAMFER_FACTOR * plain[1][b].item()
