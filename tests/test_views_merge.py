"""The rig merge on the GPU (sh_depth_views_overlap, sh_scan_compact, scan.views_overlap, scan.merge_views, merge_tol=) against
the host reference of tests/views_merge_ref.py, every comparison bitwise.  The reference reads the packed rows the GPU made -
they are the kernel's inputs; the rig kernels' normals agree with depth_views_ref only to one fp32 rounding, which a comparison
of two q could turn on - and is itself held to its properties in tests/test_views_merge_host.py."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import ops, scan
from tests import depth_ref as R
from tests import depth_views_ref as RV
from tests import views_merge_ref as RM
from tests import visibility_ref as VR
from tests.launch_record import launches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (1, 70), (17, 33), (48, 80)]
TOL = 3e-2                                                                    # a pixel of these images is 2 - 5 cm of surface wide
RIG_KERNELS = ["depth_views_count_kernel", "depth_scan_kernel", "depth_views_emit_kernel"]
MERGE_KERNELS = ["depth_views_overlap_kernel", "scan_compact_count_kernel", "depth_scan_kernel", "scan_compact_emit_kernel"]


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return all(u.shape == v.shape and np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


@functools.lru_cache(maxsize=None)
def body(H, W, V, seed=0):
    """One body's rig: V cameras on a ring around the ellipsoid, its depth images with seeded holes -> (depth float32 [V, H, W],
    intrinsics, extrinsics float32 [V, 3, 4]); computed once, shared, read-only."""
    exts = RM.ring(V, phase=0.3 + 0.1 * seed)
    f = max(1.1 * max(H, W), 40.0)                                            # the one pixel of a 1 x 1 image still hits the body
    intr = (f, f * 1.05, 0.5 * (W - 1) + 0.25, 0.5 * (H - 1) - 0.125)
    depth = np.stack([R.holes(RM.render(H, W, intr, e, RM.ellipsoid()), seed=10 * seed + v) for v, e in enumerate(exts)])
    return depth, intr, exts


def planes(s):
    """A rig ScanBatch -> (points, normals, pixel, view, counts, view_first) on the host, and seen as uint32 when it has one."""
    out = tuple(t.cpu().numpy() for t in (s.points, s.normals, s.pixels, s.view, s.counts, s.view_first))
    return out if s.seen is None else out + (seen_host(s.seen),)


def seen_host(t):
    return (t.view(torch.int32) if t.dtype != torch.int32 else t).cpu().numpy().view(np.uint32)


def reference(unmerged, depth, intr, ext, tol, width=None, **kw):
    """The reference's keep, seen [B, M] and merged planes for the packed rows of `unmerged` (host planes) and their images
    depth [B, V, H, W], ext [B, V, 3, 4]."""
    points, normals, pixel, view, counts = unmerged[:5]
    keeps, seens, merged = [], [], []
    opts = dict(depth_scale=kw.get("depth_scale", 1.0), z_range=kw.get("z_range"))
    for b, c in enumerate(counts):
        masks = None if kw.get("mask") is None else list(kw["mask"][b])
        k, s = RM.overlap(points[b, :c], normals[b, :c], view[b, :c], list(depth[b]), intr, ext[b], tol, masks=masks, **opts)
        keeps.append(k), seens.append(s)
        merged.append(RM.compact(points[b, :c], normals[b, :c], pixel[b, :c], view[b, :c], s, k, depth.shape[1]))
    M = points.shape[1]
    return RM.pack_planes(keeps, M), RM.pack_planes(seens, M), RM.pack(merged, width)


def run(depth, intr, ext, tol=TOL, **kw):
    """from_depth, views_overlap and merge_views on the device for depth [B, V, H, W], ext [B, V, 3, 4] -> (the unmerged batch's
    host planes, keep bool, seen uint32, the merged batch)."""
    s = scan.ScanBatch.from_depth(depth, intr, DEV, extrinsics=ext, **kw)
    keep, seen = scan.views_overlap(s, depth, intr, ext, tol=tol, **{k: v for k, v in kw.items() if k in ("depth_scale", "mask", "z_range")})
    assert keep.dtype == torch.bool and seen.dtype == torch.int32 and keep.shape == seen.shape == s.view.shape
    return planes(s), keep.cpu().numpy(), seen_host(seen), scan.merge_views(s, keep, seen)


def check(what, depth, intr, ext, tol=TOL, **kw):
    """keep and seen, then the six arrays, seen, counts and view_first after compaction, all bitwise against the reference."""
    un, keep, seen, merged = run(depth, intr, ext, tol, **kw)
    rkeep, rseen, rmerged = reference(un, depth, intr, ext, tol, **kw)
    assert np.array_equal(keep, rkeep) and np.array_equal(seen, rseen), what
    got = planes(merged)
    rp, rn, rpix, rview, rsn, rc, rfirst = rmerged
    assert same(got, (rp, rn, rpix, rview, rc, rfirst, rsn)), what
    assert np.array_equal(merged.host_counts, rc) and merged.perm is None and merged.points.shape[1] == max(int(rc.max()), 1), what
    live = np.arange(keep.shape[1])[None, :] < un[4][:, None]
    print("%s: %d rows, %d kept, %d seen by another camera" % (what, live.sum(), keep.sum(), ((seen[live] & (seen[live] - 1)) != 0).sum()))
    return un, keep, seen, merged


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("V", [1, 2, 3])
@pytest.mark.parametrize("H, W", SIZES)
def test_bitwise_against_the_reference(H, W, V):
    depth, intr, ext = body(H, W, V)
    un, keep, seen, merged = check("%d x %d, V = %d" % (H, W, V), depth[None], intr, ext[None], z_range=R.Z_RANGE)
    live = np.arange(keep.shape[1]) < un[4][0]
    if V == 1:
        assert np.array_equal(keep[0], live) and (seen[0][live] == 1).all()
    if V == 3 and H * W > 1000:
        assert 0 < (~keep[0][live]).sum() < live.sum()
        assert (np.abs(un[1][0][live]).sum(-1) == 0).any()                    # unknown normals among the rows


def test_thirty_two_views():
    depth, intr, ext = body(17, 33, 32, seed=4)
    un, keep, seen, merged = check("V = 32", depth[None], intr, ext[None], z_range=R.Z_RANGE)
    assert (seen >> 31).any() and set(np.unique(merged.view.cpu().numpy())) - {255} <= set(range(32))


@pytest.mark.parametrize("words", [False, True])
@pytest.mark.parametrize("name", ["plain", "mask", "z_range", "mask and z_range"])
def test_both_dtypes_with_and_without_mask_and_z_range(name, words):
    depth, intr, ext = body(17, 33, 4, seed=1)
    kw = {}
    if "mask" in name:
        kw["mask"] = (np.random.default_rng(5).random(depth.shape) > 0.3)[None]
    if "z_range" in name:
        kw["z_range"] = (1.0, 1.5)                                            # cuts the far flanks of the ellipsoid
    if words:
        depth = np.stack([R.to_words(d, 0.0001) for d in depth])
        kw["depth_scale"] = 0.0001
    un, keep, seen, _ = check("%s, %s" % (name, "words" if words else "fp32"), depth[None], intr, ext[None], **kw)
    assert 0 < keep.sum() < un[4][0]


def test_an_absent_view_an_empty_view_and_a_view_that_loses_every_row():
    depth, intr, ext = body(17, 33, 3, seed=2)
    gone = ext.copy()
    gone[1] = np.nan
    un, keep, seen, merged = check("absent view", depth[None], intr, gone[None], z_range=R.Z_RANGE)
    assert not ((seen >> 1) & 1).any() and merged.view_first[0, 1] == merged.view_first[0, 2]
    poisoned = depth.copy()
    poisoned[1] = 1.0                                                         # would be observed everywhere if it were looked at
    again = run(poisoned[None], intr, gone[None], z_range=R.Z_RANGE)
    assert np.array_equal(again[1], keep) and np.array_equal(again[2], seen)
    empty = depth.copy()
    empty[1] = 0.0
    un, keep, seen, merged = check("empty view", empty[None], intr, ext[None], z_range=R.Z_RANGE)
    assert not ((seen >> 1) & 1).any() and merged.view_first[0, 1] == merged.view_first[0, 2]
    twice = np.stack([depth[0], depth[0], depth[2]])                          # cameras 0 and 1 are one camera: the tie goes to 0
    un, keep, seen, merged = check("a view wholly dropped", twice[None], intr, ext[[0, 0, 2]][None], z_range=R.Z_RANGE)
    assert (un[3][0] == 1).any() and not (merged.view == 1).any() and merged.view_first[0, 1] == merged.view_first[0, 2]
    assert (merged.view == 0).sum() == (un[3][0] == 0).sum() - (~keep[0] & (un[3][0] == 0)).sum() and (merged.view == 2).any()


# ------------------------------------------------------------------------------------------------ batch, order, width
def test_ragged_batch_alone_permuted_twice_and_wider():
    parts = [body(17, 33, 3, seed=5 + b) for b in range(3)]
    depth, ext = np.stack([p[0] for p in parts]), np.stack([p[2] for p in parts])
    depth = depth.copy()
    depth[1, :, 5:, :] = np.nan                                               # body 1 keeps a third of its rows: a ragged batch
    ext[2, 0] = np.nan
    intr = parts[0][1]
    kw = dict(z_range=R.Z_RANGE)
    un, keep, seen, merged = check("ragged batch", depth, intr, ext, **kw)
    got = planes(merged)
    assert len(set(un[4].tolist())) == 3 and len(set(got[4].tolist())) == 3
    for b in range(3):                                                        # each body alone
        a_un, a_keep, a_seen, a_merged = run(depth[b:b + 1], intr, ext[b:b + 1], **kw)
        c, m = un[4][b], got[4][b]
        assert np.array_equal(a_keep[0, :c], keep[b, :c]) and np.array_equal(a_seen[0, :c], seen[b, :c])
        alone = planes(a_merged)
        assert alone[4][0] == m and np.array_equal(alone[5][0], got[5][b])
        assert same([alone[i][0, :m] for i in (0, 1, 2, 3, 6)], [got[i][b, :m] for i in (0, 1, 2, 3, 6)])
    perm = [2, 0, 1]
    p_un, p_keep, p_seen, p_merged = run(depth[perm], intr, ext[perm], **kw)
    assert np.array_equal(p_keep, keep[perm]) and np.array_equal(p_seen, seen[perm]) and same(planes(p_merged), [g[perm] for g in got])
    t_un, t_keep, t_seen, t_merged = run(depth, intr, ext, **kw)              # the same call twice
    assert np.array_equal(t_keep, keep) and np.array_equal(t_seen, seen) and same(planes(t_merged), got)
    # a wider M on both sides: the live rows unchanged, the padding correct
    d, k, e = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (depth, np.broadcast_to(np.asarray(intr, np.float32), (3, 3, 4)),
                                                                          scan.pack_extrinsics(ext)[0]))
    opts = dict(z_near=R.Z_RANGE[0], z_far=R.Z_RANGE[1])
    cnt, ws = ops.depth_views_count(d, k, e, **opts)
    most = int(cnt.max())
    wide = ops.depth_views_points(d, k, e, cnt, ws, most + 300, most, **opts)
    w_seen, w_keep = ops.depth_views_overlap(d, k, e, wide[0], wide[1], wide[3], cnt, TOL, **opts)
    assert np.array_equal(w_keep[:, :most].cpu().numpy() != 0, keep) and np.array_equal(seen_host(w_seen[:, :most].contiguous()), seen)
    assert not w_keep[:, most:].any() and not w_seen[:, most:].any()
    kept = int(got[4].max())
    out = ops.scan_compact(wide[0], wide[1], wide[2], wide[3], w_keep, cnt, 3, kept + 77, kept, w_seen)
    o = [t.cpu().numpy() for t in out]
    assert same([a[:, :kept] for a in o[:5]], [got[0], got[1], got[2], got[3], got[6].view(np.int32)]) and same(o[5:], got[4:6])
    assert (bits(o[0])[:, kept:] == 0).all() and (bits(o[1])[:, kept:] == 0).all() and (o[2][:, kept:] == -1).all() and (o[3][:, kept:] == 255).all() \
        and (o[4][:, kept:] == 0).all()
    none = ops.scan_compact(wide[0], wide[1], wide[2], wide[3], w_keep, cnt, 3, kept, kept)          # without seen
    assert none[4] is None and torch.equal(none[0], out[0][:, :kept]) and torch.equal(none[6], out[6])
    with pytest.raises(RuntimeError, match="cannot hold"):
        ops.scan_compact(wide[0], wide[1], wide[2], wide[3], w_keep, cnt, 3, kept - 1, kept)
    # a keep plane that says 1 in the padding too: it is not read there, every live row stays
    full = scan.merge_views(scan.ScanBatch.from_depth(depth, intr, DEV, extrinsics=ext, **kw), np.ones(keep.shape, bool))
    assert same(planes(full)[:6], un)


# ------------------------------------------------------------------------------------------------ edge rows
def test_rows_on_a_camera_plane_at_a_camera_centre_and_without_a_normal():
    """Hand-made rows for a rig whose camera 1 has the identity rotation and an exactly representable centre: a point with
    Q_z == 0 exactly under both cameras, one behind them, one AT camera 1's centre (len2 == 0: q = 0), and every fifth normal
    zeroed.  Bitwise against the reference; the plane and the centre are observed by no other camera."""
    H, W = 17, 33
    intr = (40.0, 40.0, 16.0, 8.0)
    ext = np.stack([np.eye(3, 4, dtype=np.float32)] * 2)
    ext[1, :, 3] = (0.5, 0.0, 0.0)
    depth = np.stack([RM.render(H, W, intr, e, RM.plane_z(1.0)) for e in ext])
    s = scan.ScanBatch.from_depth(depth[None], intr, DEV, extrinsics=ext[None])
    pts, nrm = s.points.clone(), s.normals.clone()
    edits = {0: (0.3, 0.1, 0.0), 1: (0.5, 0.0, 0.0), 2: (0.2, 0.0, -1.0), 3: (0.0, 0.0, 0.0)}
    for row, p in edits.items():
        pts[0, row] = torch.tensor(p)
    nrm[0, ::5] = 0.0
    d, k, e = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (depth[None], np.broadcast_to(np.asarray(intr, np.float32), (1, 2, 4)),
                                                                          scan.pack_extrinsics(ext)[0]))
    seen, keep = ops.depth_views_overlap(d, k, e, pts, nrm, s.view, s.counts, 1e-3)
    c = int(s.host_counts[0])
    rkeep, rseen = RM.overlap(pts[0, :c].cpu().numpy(), nrm[0, :c].cpu().numpy(), s.view[0, :c].cpu().numpy(), list(depth), intr, ext, 1e-3)
    assert np.array_equal(keep[0, :c].cpu().numpy() != 0, rkeep) and np.array_equal(seen_host(seen)[0, :c], rseen)
    assert (seen_host(seen)[0, :4] == 1).all() and keep[0, :4].all() and (s.view[0, :4] == 0).all()
    assert 0 < rkeep.sum() < c and (rseen == 3).any()


# ------------------------------------------------------------------------------------------------ the Python entry points
def test_merge_tol_is_overlap_then_merge_and_none_launches_nothing_new():
    parts = [body(48, 80, 3, seed=b) for b in range(2)]
    depth, ext, intr = np.stack([p[0] for p in parts]), np.stack([p[2] for p in parts]), parts[0][1]
    kw = dict(z_range=R.Z_RANGE, max_step=0.1)
    plain, rec = launches(lambda: scan.ScanBatch.from_depth(depth, intr, DEV, extrinsics=ext, **kw))
    assert [k for k, _ in rec] == RIG_KERNELS and plain.seen is None          # merge_tol=None: the launch list of the parent commit
    refs = [RV.unproject_views(depth[b], intr, ext[b], **kw) for b in range(2)]
    points, normals, pixel, view, counts, first = planes(plain)               # ... and its bits, against depth_views_ref
    rp, rn, rpix, rview, rc, rfirst = RV.pack(refs, width=points.shape[1])
    assert same((points, pixel, view, counts, first), (rp, rpix, rview, rc, rfirst))
    assert np.array_equal(np.abs(normals).sum(-1) == 0, np.abs(rn).sum(-1) == 0) and (np.abs(normals.astype(np.float64) - rn) <= 2.0 ** -23).all()
    six, rec = launches(lambda: scan.unproject_depth_views(depth, intr, ext, device=DEV, **kw))
    assert [k for k, _ in rec] == RIG_KERNELS and same([t.cpu().numpy() for t in six], (points, normals, pixel, view, counts, first))
    merged, rec = launches(lambda: scan.ScanBatch.from_depth(depth, intr, DEV, extrinsics=ext, merge_tol=TOL, **kw))
    assert [k for k, _ in rec] == RIG_KERNELS + MERGE_KERNELS
    keep, seen = scan.views_overlap(plain, depth, intr, ext, tol=TOL, z_range=R.Z_RANGE)
    by_hand = scan.merge_views(plain, keep, seen)
    assert same(planes(merged), planes(by_hand)) and np.array_equal(merged.host_counts, by_hand.host_counts)
    assert torch.equal(merged.viewpoints, plain.viewpoints) and merged.perm is None and 0 < merged.host_counts.sum() < plain.host_counts.sum()
    six = scan.unproject_depth_views(depth, intr, ext, device=DEV, merge_tol=TOL, **kw)
    m = planes(merged)
    assert same([t.cpu().numpy() for t in six], (m[0], m[1], m[2], m[3], m[4], m[5]))
    part = merged.select(slice(1, 2))
    assert torch.equal(part.seen, merged.seen[1:2]) and torch.equal(part.view_first, merged.view_first[1:2])
    with pytest.raises(ValueError, match="keep"):
        scan.merge_views(plain, keep[:, :-1])


def test_chamfer_and_align_read_a_merged_batch_like_any_rig_batch():
    """scan.chamfer (with faces=) and one scan.align iteration on the merged batch against the same calls on a batch built by hand
    from the reference's merged arrays: the same bits."""
    depth, intr, ext = body(48, 80, 4)
    kw = dict(z_range=R.Z_RANGE)
    un, keep, seen, merged = check("plumbing", depth[None], intr, ext[None], **kw)
    rp, rn, rpix, rview, rsn, rc, rfirst = reference(un, depth[None], intr, ext[None], TOL, **kw)[2]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)         # noqa: E731
    hand = scan.ScanBatch._from_parts(dev(rp), dev(rc), rc, None, dev(rn), viewpoints=dev(ext[None, :, :, 3]), pixels=dev(rpix), view=dev(rview),
                                      view_first=dev(rfirst), seen=dev(rsn.view(np.int32)))
    v, f = VR.icosphere(2)
    x = dev((v * np.array([0.25, 0.6, 0.18]))[None].astype(np.float32))
    n = x.shape[1]
    ft = scan.FaceTable(f, n, DEV)
    results = []
    for s in (merged, hand):
        xt = x.clone().requires_grad_(True)
        loss = scan.chamfer(xt, s, n=n, faces=ft, w_model_to_scan=1.0, visibility="viewpoint")
        loss.sum().backward()
        pose = scan.align(x, s, mode="rigid", iters=1, n=n, visibility="viewpoint", visibility_faces=ft)[0]
        results.append([loss.detach().cpu().numpy(), xt.grad.cpu().numpy(), pose.packed.cpu().numpy()])
    assert same(results[0], results[1]) and np.isfinite(results[0][0]).all() and results[0][0][0] > 0
