"""scan.free_space / free_space_kinds against tests/field_ref.py: term, kind, counts and the gradient bit for bit, the two loss
values to one fp32 ulp of the exact sum, on vertices constructed to hit every case of the header's list."""
import functools
import os

import numpy as np
import pytest
import torch

from semantichuman_amd import ops, scan
from semantichuman_amd.hierarchy import load_hierarchy
from tests import depth_ref as D
from tests import field_ref as R
from tests.launch_record import launches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, W = 17, 33
POW2 = (32.0, 16.0, 15.25, 8.5)            # a camera whose projection is exact for dyadic points: the boundary cases can be hit


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.int32)


@functools.lru_cache(maxsize=None)
def fields():
    """Three reference fields of one shape: the scene with mask and z_range under the exact camera (all three classes), the scene
    shifted under its own camera, and an image that is EMPTY everywhere (no allowed pixel)."""
    depth, intr = D.scene(H, W, seed=1)
    on_sphere = D.sphere_over_plane(H, W, intr)[1]
    mask = on_sphere | (np.random.default_rng(0).random((H, W)) < 0.05)
    out = [R.field(depth, POW2, mask=mask, z_range=(0.5, 1.9)), R.field(np.roll(depth, 4, axis=1), intr, z_range=D.Z_RANGE),
           R.field(np.full((H, W), 9.0, np.float32), intr, z_range=D.Z_RANGE)]
    assert set(np.unique(out[0].cls)) == {0, 1, 2} and (out[2].nearest == -1).all()
    return out


def device_field(refs):
    return scan.DepthField(*(torch.from_numpy(np.stack([getattr(r, k) for r in refs])).to(DEV) for k in ("cls", "z", "nearest", "intr")))


def specials(f, margin):
    """The edge cases, as camera-frame points of field f (its camera must be POW2 for the two boundary rows to be exact)."""
    fx, fy, cx, cy = (float(t) for t in f.intr)
    m32 = np.float32(margin)

    def at(u, v, Z):
        return [(u - cx) / fx * Z, (v - cy) / fy * Z, Z]

    sv, su = np.nonzero(f.cls == R.SURFACE)
    ev, eu = np.nonzero(f.cls == R.EMPTY)
    kv, ku = np.nonzero(f.cls == R.UNKNOWN)
    zs = float(f.z[sv[0], su[0]] - m32)
    return np.asarray([
        at(su[0], sv[0], zs),                  # e == 0: no term
        at(su[0], sv[0], 2.0 ** -3),           # in front of the surface: free space
        at(su[0], sv[0], 4.0),                 # behind it: no term
        at(eu[0], ev[0], 2.0),                 # an EMPTY pixel: silhouette
        at(ku[0], kv[0], 2.0),                 # an UNKNOWN pixel
        [0.1, 0.1, 0.0], [0.1, 0.1, -1.0], [0.1, 0.1, np.nan],
        at(-0.5, 3.0, 2.0),                    # uf == -0.5: inside, pixel 0
        at(W - 0.5, 3.0, 2.0),                 # uf == W - 0.5: outside
        at(5.0, -0.5, 2.0),                    # vf == -0.5: inside
        at(5.0, H - 0.5, 2.0),                 # vf == H - 0.5: outside
    ], np.float32)


def bodies(n, rows, margin, seed, edge=False):
    """x float32 [3, rows, 3]: random projections over the image and a border around it, depths around the surface, with the
    special rows spread over the bodies (rotated, so that n = 1 still meets three different ones).  edge: R.edge_rows come first
    in every body."""
    rng = np.random.default_rng(seed)
    x = np.zeros((3, rows, 3), np.float32)
    for b, f in enumerate(fields()):
        fx, fy, cx, cy = (float(t) for t in f.intr)
        u, v = rng.uniform(-2.0, W + 1.0, rows), rng.uniform(-2.0, H + 1.0, rows)
        Z = rng.uniform(1.0, 2.2, rows)
        x[b] = np.stack([(u - cx) / fx * Z, (v - cy) / fy * Z, Z], 1)
        sp = np.roll(specials_none(f) if b == 2 else specials(fields()[0], margin), -4 * b, axis=0)    # body 1: body 0's rows, as plain points
        if edge:
            sp = np.concatenate([R.edge_rows(f if b == 2 else fields()[0]), sp])
        k = min(len(sp), n)
        x[b, :k] = sp[:k]
    x[:, n:] = 7.0                                                         # rows >= n: never read
    return x


def specials_none(f):
    """Body 2's field has no SURFACE and no allowed pixel: its special rows are projections onto EMPTY pixels and the boundary."""
    fx, fy, cx, cy = (float(t) for t in f.intr)
    return np.asarray([[(u - cx) / fx * 2.0, (v - cy) / fy * 2.0, 2.0] for u, v in ((3, 3), (0, 0), (W - 1, H - 1), (-3, 2), (5, 5), (8, 2),
                                                                                     (9, 9), (20, 3), (1, 16), (30, 1), (31, 15), (12, 8))], np.float32)


def reference(x, n, refs, masks, margin, gL):
    out = []
    for b, f in enumerate(refs):
        term, kind, g, counts = R.terms(x[b], n, f, None if masks is None else masks[b], margin)
        out.append((term, kind, counts, R.gradient(kind, g, counts, gL[b], x.shape[1]), R.losses(term, kind, counts)))
    return out


def run(x, n, fld, mask, margin, gL):
    """The library on device tensors -> (term, kind, loss, counts, g_x) as numpy, through ops for term and through the autograd
    function for the gradient."""
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    v_mask, mask_sb = ops._mask_arg(None if mask is None else torch.from_numpy(mask), x.shape[0], n, DEV)
    term, kind, loss, counts = ops.free_space_fwd(xd.detach(), n, fld.cls, fld.z, fld.nearest, fld.intrinsics, v_mask, mask_sb, margin)
    free, sil = scan.free_space(xd, fld, n=n, vertex_mask=None if mask is None else torch.from_numpy(mask).to(DEV), margin=margin)
    assert torch.equal(torch.stack([free, sil], 1), loss)
    (free * torch.from_numpy(gL[:, 0]).to(DEV) + sil * torch.from_numpy(gL[:, 1]).to(DEV)).sum().backward()
    kinds, counts2 = scan.free_space_kinds(xd, fld, n=n, vertex_mask=None if mask is None else mask, margin=margin)
    assert torch.equal(kinds, kind) and torch.equal(counts2, counts)
    return term.cpu().numpy(), kind.cpu().numpy(), loss.cpu().numpy(), counts.cpu().numpy(), xd.grad.cpu().numpy()


def ulp_apart(got, want64):
    """|got - want| in units of the fp32 spacing at want (0 when equal)."""
    want = np.float32(want64)
    return 0.0 if got == want else abs(float(got) - want64) / float(np.spacing(np.abs(want)))


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


@pytest.mark.parametrize("n, rows", [(1, 2), (255, 256), (256, 257), (257, 257), (600, 601)])
@pytest.mark.parametrize("margin, masked", [(0.0, None), (0.03125, "n"), (0.01, "Bn")])
def test_bits_against_the_reference(n, rows, margin, masked):
    refs = fields()
    x = bodies(n, rows, margin, seed=n)
    rng = np.random.default_rng(n + 1)
    mask = None if masked is None else (rng.random(n) > 0.2) if masked == "n" else (rng.random((3, n)) > 0.2)
    if masked == "Bn":
        mask[1] = n < 256                                                  # a body without an active vertex: zeros, n_act == 0
    masks = None if mask is None else np.broadcast_to(mask, (3, n))
    gL = np.asarray([[1.0, 1.0], [0.5, -3.0], [2.0, 0.25]], np.float32)
    got = run(x, n, device_field(refs), mask, margin, gL)
    ref = reference(x, n, refs, masks, margin, gL)
    compare(got, ref, n)
    if n >= 255 and masked is None:                                        # the cases are all there
        kinds = np.concatenate([k for _, k, _, _, _ in ref])
        assert set(kinds.tolist()) == {0, 1, 2, 3, 4}
        sp = specials(refs[0], margin)
        t, k, g, _ = R.terms(sp, len(sp), refs[0], None, margin)
        assert k.tolist() == [0, 1, 0, 2, 3, 4, 4, 4, k[8], 4, k[10], 4] and k[8] != 4 and k[10] != 4
        assert (ref[2][1] != R.FREE).all() and (ref[2][1] != R.SILHOUETTE).all() and ref[2][4] == (0.0, 0.0)   # no allowed pixel
    # a body alone: the same bits as in the batch
    for b in (0, 2):
        alone = run(x[b:b + 1], n, device_field(refs[b:b + 1]), None if mask is None else masks[b:b + 1].copy(), margin, gL[b:b + 1])
        for a, whole in zip(alone, got):
            assert np.array_equal(bits(a[0]), bits(whole[b]))


@pytest.mark.parametrize("n, rows", [(1, 2), (257, 257), (600, 601)])
def test_bits_where_an_identity_camera_would_differ(n, rows):
    """One camera runs the rig's kernels without a cam, and that must mean the vertex as it is, not an identity record: on
    R.edge_rows (Z = +inf over a SURFACE pixel in bodies 0 and 1 and over an EMPTY one in body 2, X = -inf, X = NaN, and a kind-1
    term whose zero gradient words a negative gL makes -0) ops.free_space_fwd / _bwd and scan.free_space give the reference's bits."""
    refs, margin = fields(), 0.01
    x = bodies(n, rows, margin, seed=n, edge=True)
    gL = np.asarray([[-1.0, 1.0], [0.5, -3.0], [-2.0, -0.25]], np.float32)
    fld = device_field(refs)
    got = run(x, n, fld, None, margin, gL)
    ref = reference(x, n, refs, None, margin, gL)
    compare(got, ref, n)
    xd = torch.from_numpy(x).to(DEV)
    g = ops.free_space_bwd(xd, n, fld.cls, fld.z, fld.nearest, fld.intrinsics, None, 0, margin, torch.from_numpy(got[3]).to(DEV),
                           torch.from_numpy(gL).to(DEV))
    assert np.array_equal(bits(g.cpu().numpy()), bits(got[4]))
    assert np.isposinf(x[:, 0, 2]).all() and [int(r[1][0]) for r in ref] == [R.NONE] * 3           # not kind 4: 0 * inf never happened
    if n >= 4:                                                             # the rows are all there, and are the cases they stand for
        assert np.isneginf(x[:, 1, 0]).all() and np.isnan(x[:, 2, 0]).all() and np.signbit(x[:, 3, 0]).all()
        assert [r[1][:4].tolist() for r in ref] == [[R.NONE, R.OUTSIDE, R.OUTSIDE, R.FREE]] * 2 + [[R.NONE, R.OUTSIDE, R.OUTSIDE, R.NONE]]
        g0 = ref[0][3][3]
        assert (g0[:2] == 0).all() and np.signbit(g0[:2]).all() and g0[2] > 0                     # -0, -0 under gL[0][0] < 0


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_an_infinite_silhouette_term_keeps_the_case_list(sign):
    """Z = +inf over an EMPTY pixel that has an allowed neighbour (R.edge_fields' "empty"): kind 2 with an infinite offset from the
    ray, so term, loss and gradient hold infinities - bitwise the reference's, no NaN; an identity record would say kind 4."""
    f, margin = R.edge_fields()["empty"], 0.01
    x = np.concatenate([R.edge_rows(f), np.full((1, 3), 7.0, np.float32)])[None]
    n, gL = 4, np.asarray([[sign * 2.0, sign * 0.5]], np.float32)
    got = run(x, n, device_field([f]), None, margin, gL)
    ref = reference(x, n, [f], None, margin, gL)
    compare(got, ref, n)
    assert ref[0][1].tolist() == [R.SILHOUETTE, R.OUTSIDE, R.OUTSIDE, R.SILHOUETTE] and np.isposinf(ref[0][0][0])
    assert np.isposinf(got[2][0, 1]) and got[2][0, 0] == 0 and np.isinf(got[4][0, 0]).all() and not np.isnan(got[4]).any()


@functools.lru_cache(maxsize=None)
def model_scene():
    """The two bodies of small_ae.npz (170 vertices and the dummy row) in front of a camera, each rendered to a 64 x 48 depth
    image by the scene helper, and the same bodies grown by 15 % about their centres: they overshoot silhouette and surface."""
    gs = np.load(os.path.join(GOLD, "small_ae.npz"))
    faces = np.asarray(load_hierarchy(os.path.join(GOLD, "small_ae.npz")).faces, np.int64)
    x = np.asarray(gs["x"], np.float64)
    n = x.shape[1] - 1
    hh, ww = 64, 48
    refs, grown = [], []
    for b in range(x.shape[0]):
        Rm, t, intr, size = R.camera_for(x[b, :n], hh, ww)
        cam = x[b] @ Rm.T + t
        depth = R.render(cam[:n], faces, intr, hh, ww, background=10.0 * size)
        refs.append(R.field(depth, intr, z_range=(0.5 * size, 5.0 * size)))
        centre = np.asarray([0.0, 0.0, 2.5 * size])
        grown.append(((cam - centre) * 1.15 + centre).astype(np.float32))
    return refs, np.stack(grown), n


def test_bits_on_the_model():
    refs, x, n = model_scene()
    assert n == 170 and all(set(np.unique(r.cls)) == {0, 2} for r in refs)
    gL = np.ones((2, 2), np.float32)
    fld = device_field(refs)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    (free, sil), rec = launches(lambda: scan.free_space(xd, fld))          # n = None: rows - 1
    assert [k for k, _ in rec] == ["free_space_fwd_kernel"]
    _, rec = launches(lambda: (free + sil).sum().backward())
    assert [k for k, _ in rec] == ["free_space_bwd_kernel"]
    kind, counts = scan.free_space_kinds(xd, fld)
    ref = reference(x, n, refs, None, 0.0, gL)
    for b, (t, k, c, g, L) in enumerate(ref):
        assert c[1] > 10 and c[2] > 10                                     # the grown body does violate both
        assert np.array_equal(kind[b].cpu().numpy(), k) and np.array_equal(counts[b].cpu().numpy(), c)
        assert np.array_equal(bits(xd.grad[b].cpu().numpy()), bits(g))
        assert ulp_apart(free[b].item(), L[0]) <= 1.0 and ulp_apart(sil[b].item(), L[1]) <= 1.0


def test_pose_is_to_scan_frame_by_hand_times_scale_squared():
    refs, x, n = model_scene()
    fld = device_field(refs)
    rng = np.random.default_rng(3)
    A = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(2)])
    A = A * np.sign(np.linalg.det(A))[:, None, None] * np.asarray([0.7, 1.9])[:, None, None]
    t = rng.standard_normal((2, 3))
    pose = scan.Pose(torch.from_numpy(A.astype(np.float32)).to(DEV), torch.from_numpy(t.astype(np.float32)).to(DEV))
    model = pose.apply(torch.from_numpy(x).to(DEV)).requires_grad_(True)    # the camera-frame bodies in a model frame
    free, sil = scan.free_space(model, fld, pose=pose, margin=0.01)
    (free + 2 * sil).sum().backward()
    by_hand = model.detach().clone().requires_grad_(True)
    f2, s2 = scan.free_space(pose.to_scan_frame(by_hand), fld, margin=0.01)
    f2, s2 = f2 * (pose.scale * pose.scale), s2 * (pose.scale * pose.scale)
    (f2 + 2 * s2).sum().backward()
    assert torch.equal(free, f2) and torch.equal(sil, s2) and torch.equal(model.grad, by_hand.grad)
    assert float(free.detach().min()) > 0 and float(sil.detach().min()) > 0 and float(model.grad.abs().max()) > 0
    assert pose.packed.grad is None and not pose.packed.requires_grad


def test_value_errors():
    refs, x, n = model_scene()
    fld, xd = device_field(refs), torch.from_numpy(x).to(DEV)
    with pytest.raises(ValueError, match="2 bodies, a field of 1 images"):
        scan.free_space(xd, fld.select(slice(0, 1)))
    with pytest.raises(ValueError, match="margin must be >= 0"):
        scan.free_space(xd, fld, margin=-0.1)
    with pytest.raises(ValueError, match="2 bodies, 3 poses"):
        scan.free_space(xd, fld, pose=scan.Pose.identity(3, DEV))
    with pytest.raises(ValueError, match="outside"):
        scan.free_space_kinds(xd, fld, n=n + 2)
