"""Any-view visibility on the GPU (sh_vertex_visibility_views, scan.visible_vertices with rig viewpoints [B, V, 3],
visibility="viewpoint" on a rig batch).  THE test: bit v of `seen` equals, bit for bit, what sh_vertex_visibility returns for
view v alone - over V, geometry, masks, the facing test, every split and batch.  Then the float64 reference per view, an analytic
two-camera sphere, absent cameras, the refusals, and the plumbing into chamfer, align and fit_scan."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, ops, scan
from tests import normals_ref as N
from tests import scan_ref as R
from tests import visibility_ref as V
from tests.launch_record import recorded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIX = np.concatenate([V.DIRECTIONS, -V.DIRECTIONS])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(x float32 [n, 3], faces) of one test body, computed once and shared read-only."""
    if name == "screen":
        v, f, _, _ = V.screen_scene()
    else:
        v, f = V.icosphere(int(name[-1]))
    return v.astype(np.float32), f


def viewpoints(x, count):
    """`count` viewpoints around x: visibility_ref.viewpoint over DIRECTIONS and their negatives, further rounds further out."""
    return np.stack([V.viewpoint(x, SIX[k % 6], 3.0 + 0.25 * (k // 6)) for k in range(count)]).astype(np.float32)


def normals_for(x, ft, angle):
    if angle is None:
        return None, 0.0
    return ops.vertex_normals(x, ft.faces, ft.vf_ptr, ft.vf_idx, ft.n), (0.0 if angle == 90.0 else float(np.cos(np.deg2rad(angle))))


def views_run(x, ft, views, mask=None, angle=None, chunks=0):
    """ops.vertex_visibility_views -> (vis bool [B, n], seen uint32 [B, n]) on the host."""
    tn, cos_g = normals_for(x, ft, angle)
    vis, seen = ops.vertex_visibility_views(x, ft.faces, ft.n, dev(views), mask, tn, cos_g, chunks=chunks, seen=True)
    return vis.cpu().numpy() != 0, seen.cpu().numpy().view(np.uint32)


def single_run(x, ft, view, mask=None, angle=None):
    """ops.vertex_visibility for one viewpoint per body -> bool [B, n] on the host."""
    tn, cos_g = normals_for(x, ft, angle)
    return ops.vertex_visibility(x, ft.faces, ft.n, dev(view), mask, tn, cos_g).cpu().numpy() != 0


def bit(seen, v):
    return (seen >> np.uint32(v)) & np.uint32(1) != 0


# ------------------------------------------------------------------------------------------------ the test proper
@pytest.mark.parametrize("angle", [None, 90.0, 60.0])
@pytest.mark.parametrize("count", [1, 2, 5, 32])
@pytest.mark.parametrize("name", ["ico2", "ico3", "screen"])
def test_bit_v_is_the_single_view_kernel_for_view_v(name, count, angle):
    xh, f = geometry(name)
    n = len(xh)
    x, ft = dev(xh[None]), scan.FaceTable(f, n, DEV)
    views = viewpoints(xh, count)[None]
    mask = dev(np.random.default_rng(count).random((1, n)) > 0.25)
    vis, seen = views_run(x, ft, views, mask, angle)
    union = np.zeros((1, n), bool)
    for v in range(count):
        alone = single_run(x, ft, views[:, v], mask, angle)
        assert np.array_equal(bit(seen, v), alone), (name, count, angle, v)
        union |= alone
    assert (seen >> np.uint32(count) == 0).all() if count < 32 else True
    assert np.array_equal(vis, union) and np.array_equal(vis, seen != 0)
    assert 0 < vis.sum() < n                                               # the mask hides some, the cameras see some
    if count == 1:
        assert np.array_equal(vis, single_run(x, ft, views[:, 0], mask, angle))


def test_per_view_against_the_float64_reference():
    xh, f = geometry("ico2")
    views = viewpoints(xh, 2)
    _, seen = views_run(dev(xh[None]), scan.FaceTable(f, len(xh), DEV), views[None])
    for v in range(2):
        ref_vis, cls = V.visibility(xh, f, views[v])
        V.agree(bit(seen[0], v), ref_vis, cls)                             # its own cap of 0.01


def test_two_cameras_on_opposite_sides_of_a_sphere():
    """A unit icosphere (level 3) at the origin, cameras at +3u and -3u.  For the SMOOTH unit sphere camera 0 sees exactly the
    points with n . u > 1/3 (the tangent cone from distance 3) and camera 1 those with n . u < -1/3.  The faceted sphere is a convex
    polytope inscribed in it: every vertex with n . u > 1/3 is seen (the segment to the camera leaves the ball at once), and so
    are the vertices just below the cone whose own fan still turns a face to the camera - visible iff some incident face faces the
    camera, the rule of visibility_ref.sphere_expected.  On this mesh and this u that adds 25 vertices per camera (239 seen against
    214 inside the cone; host arithmetic), so "exactly n . u > 1/3" is asserted as the inclusion it is, the exact set against the
    polytope's rule, and the band seen by neither camera is asserted non-empty and to hold every vertex with |n . u| <= 1/4.
    u is chosen so that no vertex lies within 1e-3 of either cone boundary, nor within 1e-3 (as a cosine) of the polytope's."""
    v, f = V.icosphere(3)
    u = np.array([-0.51, -0.35, 0.53])
    u /= np.linalg.norm(u)
    d = v @ u
    assert min(np.abs(d - 1 / 3).min(), np.abs(d + 1 / 3).min()) > 1e-3
    want0, m0 = V.sphere_expected(v, f, 3 * u)
    want1, m1 = V.sphere_expected(v, f, -3 * u)
    assert min(np.abs(m0).min(), np.abs(m1).min()) > 1e-3
    views = np.stack([3 * u, -3 * u]).astype(np.float32)[None]
    vis, seen = views_run(dev(v[None].astype(np.float32)), scan.FaceTable(f, len(v), DEV), views)
    s0, s1 = bit(seen[0], 0), bit(seen[0], 1)
    print("cone: %d / %d, polytope: %d / %d, GPU: %d / %d, neither: %d" % ((d > 1 / 3).sum(), (d < -1 / 3).sum(), want0.sum(), want1.sum(), s0.sum(),
                                                                          s1.sum(), (~vis[0]).sum()))
    assert s0[d > 1 / 3].all() and s1[d < -1 / 3].all()
    assert np.array_equal(s0, want0) and np.array_equal(s1, want1)
    assert np.array_equal(vis[0], s0 | s1) and not (s0 & s1).any()
    band = np.abs(d) <= 0.25
    assert band.sum() > 0 and not vis[0][band].any() and (~vis[0]).sum() >= band.sum()


# ------------------------------------------------------------------------------------------------ splits, batches, NaN rows
@functools.lru_cache(maxsize=None)
def batch():
    """Three bodies of 642 vertices - the icosphere squeezed differently - and 5 viewpoints each, with a vertex mask."""
    xh, f = geometry("ico3")
    x = np.stack([xh * np.array(s, np.float32) for s in ((1, 1, 1), (1.3, 0.8, 1.0), (0.7, 1.1, 1.4))])
    views = np.stack([viewpoints(x[b], 5 + b)[b:b + 5] for b in range(3)])
    mask = np.random.default_rng(9).random((3, x.shape[1])) > 0.2
    return x, f, views, mask


@pytest.mark.parametrize("angle", [None, 60.0])
def test_every_split_and_every_batch_give_the_same_bits(angle):
    x, f, views, mask = batch()
    n = x.shape[1]
    ft = scan.FaceTable(f, n, DEV)
    full = views_run(dev(x), ft, views, dev(mask), angle, chunks=1)
    for chunks in (2, 3, 0):
        got = views_run(dev(x), ft, views, dev(mask), angle, chunks=chunks)
        assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1]), chunks
    for b in range(3):
        for chunks in (1, 0):                                              # alone the automatic split has many chunks
            got = views_run(dev(x[b:b + 1]), ft, views[b:b + 1], dev(mask[b:b + 1]), angle, chunks=chunks)
            assert np.array_equal(got[0][0], full[0][b]) and np.array_equal(got[1][0], full[1][b]), (b, chunks)
    lib = _lib.load()
    assert lib.sh_vertex_visibility_views_workspace(3, n, len(f), 5, 1) == 0
    assert lib.sh_vertex_visibility_views_workspace(3, n, len(f), 5, 3) == 3 * 3 * n * 4


def test_absent_cameras():
    x, f, views, mask = batch()
    ft = scan.FaceTable(f, x.shape[1], DEV)
    full = views_run(dev(x), ft, views, dev(mask))
    holed = views.copy()
    holed[0, 2, 1] = np.nan                                                # one absent camera among live ones
    holed[1] = np.nan                                                      # a body with no camera at all: a full scan
    holed[2, 1:] = np.nan                                                  # its neighbour keeps one camera: it sees one side only
    for chunks in (1, 3):
        vis, seen = views_run(dev(x), ft, holed, dev(mask), chunks=chunks)
        assert not bit(seen[0], 2).any() and bit(full[1][0], 2).any()
        assert np.array_equal(seen[0] | (full[1][0] & np.uint32(4)), full[1][0]) and np.array_equal(vis[0], seen[0] != 0)
        assert (seen[1] == 0).all() and np.array_equal(vis[1], mask[1])
        assert np.array_equal(seen[2], full[1][2] & np.uint32(1)) and np.array_equal(vis[2], seen[2] != 0) and not vis[2][mask[2]].all()


@functools.lru_cache(maxsize=None)
def barrel():
    """Two bodies of 300 vertices - two vertex tiles of 256, the second partial - under 600 faces - three LDS tiles of 256, the last
    partial: 15 rings of 20 on a barrel, its two caps as fans, four wall faces once more with the other winding.  With three
    viewpoints per body and a vertex mask."""
    rings, seg = 15, 20
    t, a = np.linspace(-1.0, 1.0, rings), 2 * np.pi * np.arange(seg) / seg
    r = 1.0 - 0.35 * t ** 2
    v = np.stack([np.outer(r, np.cos(a)), np.outer(r, np.sin(a)), np.repeat(t[:, None], seg, 1)], -1).reshape(-1, 3)
    i = (np.arange(rings - 1)[:, None] * seg + np.arange(seg)[None]).ravel()
    j = (np.arange(rings - 1)[:, None] * seg + (np.arange(seg)[None] + 1) % seg).ravel()
    wall = np.concatenate([np.stack([i, j, j + seg], -1), np.stack([i, j + seg, i + seg], -1)])
    k = np.arange(1, seg - 1)
    caps = np.concatenate([np.stack([0 * k, k + 1, k], -1), (rings - 1) * seg + np.stack([0 * k, k, k + 1], -1)])
    f = np.concatenate([wall, caps, wall[:4, ::-1]]).astype(np.int64)
    assert v.shape == (300, 3) and f.shape == (600, 3)
    x = np.stack([v, v * np.array([1.2, 0.8, 1.1])]).astype(np.float32)
    views = np.stack([viewpoints(x[b], 3 + b)[b:b + 3] for b in range(2)])
    mask = np.random.default_rng(5).random((2, 300)) > 0.2
    return x, f, views, mask


def sentinel_run(x, ft, view, mask, tn, cos_g, chunks):
    """The C entry point of the view's rank - [B, 3] or [B, V, 3] - on outputs and a workspace filled with a sentinel beforehand, so
    that an element left unwritten shows -> (vis uint8 [B, n], seen uint32 [B, n] - None for [B, 3]) on the host."""
    lib = _lib.load()
    B, n, nF = x.shape[0], ft.n, len(ft)
    vis = torch.full((B, n), 0xAA, dtype=torch.uint8, device=DEV)
    seen = torch.full((B, n), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if view.dim() == 3 else None
    head = (ops.ptr(x), x.stride(0), n, ops.ptr(ft.faces), nF, ops.ptr(tn), ops.ptr(view))
    if seen is None:
        nbytes = lib.sh_vertex_visibility_workspace(B, n, nF, chunks)
    else:
        nbytes = lib.sh_vertex_visibility_views_workspace(B, n, nF, view.shape[1], chunks)
    ws = torch.full((max(nbytes, 1),), 0xAA, dtype=torch.uint8, device=DEV)
    tail = (cos_g, ops.ptr(mask), n, B, chunks, ops.ptr(ws), nbytes, ops.ptr(vis))
    if seen is None:
        ops.check(lib.sh_vertex_visibility(*head, *tail, ops.stream_ptr()), "sh_vertex_visibility")
        return vis.cpu().numpy(), None
    ops.check(lib.sh_vertex_visibility_views(*head, view.shape[1], *tail, ops.ptr(seen), ops.stream_ptr()), "sh_vertex_visibility_views")
    return vis.cpu().numpy(), seen.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("chunks", [1, 3])
def test_partial_tiles_mask_grazing_and_splits_together(chunks):
    """Two vertex tiles and three face tiles, the last of each partial, two bodies, a vertex mask and a grazing angle, one chunk
    and three: a rig of one is the single-view kernel bit for bit, an absent view's bit is 0 everywhere, a body without any view
    is fully visible where active, and every output element is written."""
    xh, f, views, maskh = barrel()
    x, ft = dev(xh), scan.FaceTable(f, xh.shape[1], DEV)
    mask = dev(maskh).to(torch.uint8)
    tn, cos_g = normals_for(x, ft, 75.0)
    alone = [sentinel_run(x, ft, dev(views[:, v]), mask, tn, cos_g, chunks)[0] for v in range(3)]
    for a in alone:
        assert np.isin(a, (0, 1)).all() and not a[~maskh].any() and 0 < a.sum() < maskh.sum()
    plain = ops.vertex_visibility(x, ft.faces, ft.n, dev(views[:, 0]), mask).cpu().numpy()
    assert (plain != alone[0]).any()                                       # the grazing angle matters
    vis, seen = sentinel_run(x, ft, dev(views[:, :1]), mask, tn, cos_g, chunks)       # a rig of one
    assert np.array_equal(vis, alone[0]) and np.array_equal(seen, alone[0].astype(np.uint32))
    holed = views.copy()
    holed[:, 1] = np.nan                                                   # an absent camera between two live ones
    holed[1] = np.nan                                                      # and a body with no camera at all
    vis, seen = sentinel_run(x, ft, dev(holed), mask, tn, cos_g, chunks)
    assert not bit(seen, 1).any() and (seen >> np.uint32(3) == 0).all() and np.isin(vis, (0, 1)).all()
    assert np.array_equal(bit(seen[0], 0), alone[0][0] != 0) and np.array_equal(bit(seen[0], 2), alone[2][0] != 0)
    assert np.array_equal(vis[0] != 0, seen[0] != 0)
    assert (seen[1] == 0).all() and np.array_equal(vis[1] != 0, maskh[1])


def test_view_counts_outside_1_to_32_are_refused():
    x, f, views, _ = batch()
    ft = scan.FaceTable(f, x.shape[1], DEV)
    for count in (0, 33):
        with pytest.raises(ValueError, match="views"):
            ops.vertex_visibility_views(dev(x), ft.faces, ft.n, torch.zeros((3, count, 3), device=DEV))
        with pytest.raises(ValueError):
            scan.visible_vertices(dev(x), ft, torch.zeros((3, count, 3), device=DEV), n=ft.n)


def test_visible_vertices_takes_a_rig_and_returns_seen():
    x, f, views, mask = batch()
    ft = scan.FaceTable(f, x.shape[1], DEV)
    full = views_run(dev(x), ft, views, dev(mask), 60.0)
    vis, seen = scan.visible_vertices(dev(x), ft, dev(views), n=ft.n, vertex_mask=dev(mask), grazing_angle=60.0, return_seen=True)
    assert vis.dtype == torch.bool and np.array_equal(vis.cpu().numpy(), full[0])
    assert np.array_equal(seen.cpu().numpy().view(np.uint32), full[1])
    assert np.array_equal(scan.visible_vertices(dev(x), ft, dev(views), n=ft.n, vertex_mask=dev(mask), grazing_angle=60.0).cpu().numpy(), full[0])
    with pytest.raises(ValueError, match="device tensor"):                 # a host array of rank 3 stays refused (tests/test_visibility_host.py)
        scan.visible_vertices(dev(x), ft, views, n=ft.n)
    with pytest.raises(ValueError, match="return_seen"):
        scan.visible_vertices(dev(x), ft, views[:, 0], n=ft.n, return_seen=True)


# ------------------------------------------------------------------------------------------------ plumbing
@functools.lru_cache(maxsize=None)
def rig_inputs():
    """The three 170-vertex bodies with a two-camera rig each and their scans as a rig batch."""
    x, f = N.bodies("small_ae.npz", 3)
    n = x.shape[1] - 1
    views = np.stack([[V.viewpoint(x[b, :n], V.DIRECTIONS[b]), V.viewpoint(x[b, :n], -V.DIRECTIONS[(b + 1) % 3])] for b in range(3)]).astype(np.float32)
    clouds = R.make_scans(np.roll(x, 1, 0), n, [501, 300, 257], seed=4)
    return x, f, views, n, clouds


def loss_and_grad(x, scans, **kw):
    xt = dev(x).requires_grad_(True)
    loss = scan.chamfer(xt, scans, **kw)
    loss.sum().backward()
    return loss.detach().cpu().numpy().view(np.int32), xt.grad.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("surface", [False, True])
def test_chamfer_visibility_on_a_rig_is_the_mask(surface):
    x, f, views, n, clouds = rig_inputs()
    scans = scan.ScanBatch(clouds, DEV, rig_viewpoints=views)
    assert torch.equal(scans.viewpoints, dev(views)) and torch.equal(scans.select(slice(1, 3)).viewpoints, dev(views[1:3]))
    assert torch.equal(scan.ScanBatch(clouds, DEV, rig_viewpoints=views[0]).viewpoints, dev(np.broadcast_to(views[0], views.shape)))
    given = dev(np.random.RandomState(1).rand(3, n) > 0.2)
    tables = dict(faces=f) if surface else {}
    vis = scan.visible_vertices(dev(x), f, scans.viewpoints)
    one = scan.visible_vertices(dev(x), f, scans.viewpoints[:, 0].contiguous())
    assert (vis | ~one).all() and (vis & ~one).any()                       # the second camera adds vertices
    kw = dict(w_model_to_scan=1.0, trunc=0.5, **tables)
    (a, names) = recorded(lambda: loss_and_grad(x, scans, vertex_mask=given, visibility="viewpoint", visibility_faces=f, **kw))
    b = loss_and_grad(x, scans, vertex_mask=given & vis, **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert "vertex_visibility_views_kernel" in names and "vertex_visibility_kernel" not in names
    c = loss_and_grad(x, scans, vertex_mask=given & one, **kw)
    assert not np.array_equal(a[0], c[0])                                  # and they matter
    g = loss_and_grad(x, scans, vertex_mask=given, visibility="viewpoint", visibility_faces=f, grazing_angle=70.0, **kw)
    vg = scan.visible_vertices(dev(x), f, scans.viewpoints, grazing_angle=70.0)
    h = loss_and_grad(x, scans, vertex_mask=given & vg, **kw)
    assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1])


def test_align_on_a_rig_moves_every_viewpoint_and_ors_the_views():
    x, f, views, n, clouds = rig_inputs()
    x = dev(x[:1])
    ft = scan.FaceTable(f, n, DEV)
    rig = scan.ScanBatch(clouds[:1], DEV, rig_viewpoints=views[:1])
    iters = 4
    kw = dict(mode="rigid", w_model_to_scan=1.0, visibility="viewpoint", visibility_faces=ft)
    pose, aligned, _ = scan.align(x, rig, iters=iters, **kw)
    assert tuple(pose.visible.shape) == (iters, 1, n) and pose.visible.dtype == torch.bool
    assert tuple(aligned.viewpoints.shape) == (1, 2, 3) and torch.equal(aligned.viewpoints, pose.apply(rig.viewpoints))
    for k in range(iters):                                                 # the mask of iteration k: the OR of the two single-view runs under the pose before it
        before = scan.align(x, rig, iters=k, **kw)[0]
        posed = before.apply(rig.viewpoints)
        alone = [scan.visible_vertices(x, ft, posed[:, v].contiguous()) for v in range(2)]
        assert torch.equal(pose.visible[k], alone[0] | alone[1]), k
        assert torch.equal(pose.visible[k], scan.visible_vertices(x, ft, posed)), k


def test_fit_scan_step_on_a_rig_batch_with_gate_and_robust_term():
    """One fit_scan step with normal_angle=, robust= and visibility="viewpoint" on a rig batch made from depth images runs and
    returns finite values."""
    import os

    from semantichuman_amd.hierarchy import load_hierarchy
    from tests.test_scan import GOLD, PARTS, semantic_setup
    m, z0, z_kps, dummy = semantic_setup()[:4]
    faces = np.asarray(load_hierarchy(os.path.join(GOLD, "semantic.npz")).faces, np.int64)
    B = z0.shape[0]
    H, W = 48, 64
    intr = (70.0, 70.0, 31.5, 23.5)
    depth = (3.0 + 0.05 * np.random.default_rng(0).random((B, 2, H, W))).astype(np.float32)   # two rough walls through the origin, back to back
    front = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -3.0]], np.float32)
    back = np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 3.0]], np.float32)      # the second camera looks back at the first
    scans = scan.ScanBatch.from_depth(depth, intr, DEV, extrinsics=np.broadcast_to(np.stack([front, back]), (B, 2, 3, 4)))
    assert tuple(scans.viewpoints.shape) == (B, 2, 3) and scans.normals is not None and int(scans.host_counts.min()) == 2 * H * W
    assert torch.equal(scans.viewpoints[0], dev(np.array([[0, 0, -3.0], [0, 0, 3.0]], np.float32)))
    (z_new, final, losses), names = recorded(lambda: editing.fit_scan(
        m, z0, z_kps, scans, parts=PARTS, steps=1, lr=1e-2, trunc=5.0, dummy=dummy, w_model_to_scan=1.0, normal_angle=80.0, normal_faces=faces,
        robust="geman-mcclure", robust_scale=0.1, visibility="viewpoint"))
    assert torch.isfinite(z_new).all() and torch.isfinite(final).all() and torch.isfinite(torch.as_tensor(losses)).all()
    assert "vertex_visibility_views_kernel" in names
