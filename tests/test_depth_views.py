"""Depth rigs on the GPU (sh_depth_views_count, sh_depth_views_points, scan.unproject_depth_views, ScanBatch.from_depth with
extrinsics) against the host reference of tests/depth_views_ref.py: all six outputs bitwise (normals within one fp32 rounding, and
how many were bit-equal is printed), every option, empty and absent views, V = 32, ragged batches, determinism over batch, order
and width, the single-camera call for identity extrinsics, and the untouched launch list of the call without extrinsics."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import ops, scan
from tests import depth_ref as R
from tests import depth_views_ref as RV
from tests.launch_record import launches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (1, 70), (17, 33), (48, 80)]


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


def run(depth, intr, ext, **kw):
    """scan.unproject_depth_views on the device -> its six results on the host."""
    return tuple(t.cpu().numpy() for t in scan.unproject_depth_views(depth, intr, ext, device=DEV, **kw))


@functools.lru_cache(maxsize=None)
def body(H, W, V, seed=0):
    """One body's rig: the scene at H x W with another seed (its holes in) and another random rigid transform per view ->
    (depth float32 [V, H, W], intrinsics, extrinsics float32 [V, 3, 4]); computed once, shared, read-only."""
    rng = np.random.default_rng(1000 * seed + V)
    depth = np.stack([R.scene(H, W, seed=10 * seed + v)[0] for v in range(V)])
    return depth, R.intrinsics_for(H, W), np.stack([RV.extrinsic(rng) for _ in range(V)])


def check(what, got, bodies):
    """Counts, view_first, pixel, view, points and every padding row bitwise; the unknown normals the same rows; every known
    normal within 2^-23 per component (one fp32 rounding of an fp64 value whose own error is below 1e-14)."""
    points, normals, pixel, view, counts, view_first = got
    rp, rn, rpix, rview, rc, rfirst = RV.pack(bodies, width=points.shape[1])
    assert np.array_equal(counts, rc) and np.array_equal(view_first, rfirst), what
    assert view.dtype == np.uint8 and view_first.dtype == np.int32 and pixel.dtype == np.int32, what
    assert np.array_equal(pixel, rpix) and np.array_equal(view, rview), what
    assert np.array_equal(bits(points), bits(rp)), what
    live = np.arange(points.shape[1])[None, :] < counts[:, None]
    assert (bits(normals)[~live] == 0).all() and (bits(points)[~live] == 0).all() and (pixel[~live] == -1).all() and (view[~live] == 255).all(), what
    unknown, r_unknown = np.abs(normals).sum(-1) == 0, np.abs(rn).sum(-1) == 0
    assert np.array_equal(unknown, r_unknown), what
    known = live & ~r_unknown
    err = np.abs(normals[known].astype(np.float64) - rn[known].astype(np.float64))
    print("%s: %d rows, %d known normals, largest component error %.3e, %d of them bit-equal"
          % (what, int(counts.sum()), int(known.sum()), err.max() if err.size else 0.0, int((bits(normals[known]) == bits(rn[known])).all(-1).sum())))
    assert (err <= 2.0 ** -23).all(), what


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("V", [1, 2, 3])
@pytest.mark.parametrize("H, W", SIZES)
def test_bitwise_against_the_reference(H, W, V):
    depth, intr, ext = body(H, W, V)
    got = run(depth, intr, ext, z_range=R.Z_RANGE)
    ref = RV.unproject_views(depth, intr, ext, z_range=R.Z_RANGE)
    check("%d x %d, V = %d" % (H, W, V), got, [ref])
    if H * W > 1:
        assert 0 < len(ref.pixel) < V * H * W                                 # the holes took some
    if min(H, W) > 1:
        assert any(r.known.any() for r in ref.refs)


OPTIONS = {
    "mask": lambda d: dict(mask=np.random.default_rng(5).random(d.shape) > 0.3),
    "z_range": lambda d: dict(z_range=(1.45, 5.0)),
    "max_step": lambda d: dict(max_step=0.1, z_range=R.Z_RANGE),
    "drop_isolated": lambda d: dict(drop_isolated=True, max_step=0.02, z_range=R.Z_RANGE),
    "stride=2": lambda d: dict(stride=2, z_range=R.Z_RANGE),
}


@pytest.mark.parametrize("words", [False, True])
@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_every_option_in_both_dtypes(name, words):
    depth, intr, ext = body(17, 33, 3, seed=1)
    kw = OPTIONS[name](depth)
    if words:
        depth = np.stack([R.to_words(d, 0.0001) for d in depth])              # a tenth of a millimetre per unit: the plane at 2 m is the word 20000
        depth[0, 3, 4] = 40000                                                # a word above 32767: read unsigned, 4 m, inside every z_range here
        assert depth.dtype == np.uint16 and (depth > 32767).any()
        kw["depth_scale"] = 0.0001
    got = run(depth, intr, ext, **kw)
    masks = kw.pop("mask", None)
    ref = RV.unproject_views(depth, intr, ext, masks=masks, **kw)
    check("%s, %s" % (name, "words" if words else "fp32"), got, [ref])
    assert len(ref.pixel) > 0


def test_an_empty_view_in_the_middle_repeats_view_first():
    depth, intr, ext = body(17, 33, 3, seed=2)
    depth = depth.copy()
    depth[1] = 0.0                                                            # no reading anywhere
    got = run(depth, intr, ext, z_range=R.Z_RANGE)
    ref = RV.unproject_views(depth, intr, ext, z_range=R.Z_RANGE)
    check("empty view", got, [ref])
    first = got[5][0]
    assert first[1] == first[2] and 0 < first[1] < first[3] and not (got[3] == 1).any()


def test_an_absent_camera_emits_nothing_and_is_not_read():
    depth, intr, ext = body(17, 33, 3, seed=3)
    ext = ext.copy()
    ext[1] = np.nan
    got = run(depth, intr, ext, z_range=R.Z_RANGE)
    ref = RV.unproject_views(depth, intr, ext, z_range=R.Z_RANGE)
    check("absent view", got, [ref])
    assert got[5][0][1] == got[5][0][2] and not (got[3] == 1).any() and (got[3] == 2).any()
    poisoned = depth.copy()
    poisoned[1] = 1.0                                                         # valid everywhere: would add rows if it were looked at
    assert same(run(poisoned, intr, ext, z_range=R.Z_RANGE), got)


def test_thirty_two_views():
    depth, intr, ext = body(17, 33, 32, seed=4)
    got = run(depth, intr, ext, z_range=R.Z_RANGE)
    check("V = 32", got, [RV.unproject_views(depth, intr, ext, z_range=R.Z_RANGE)])
    assert set(np.unique(got[3])) == set(range(32))


# ------------------------------------------------------------------------------------------------ batch, order, width
def test_ragged_batch_alone_permuted_twice_and_wider():
    parts = [body(17, 33, 3, seed=5 + b) for b in range(3)]
    depth, ext = np.stack([p[0] for p in parts]), np.stack([p[2] for p in parts])
    depth = depth.copy()
    depth[1, :, 5:, :] = np.nan                                               # body 1 keeps a third of its rows: a ragged batch
    ext[2, 0] = np.nan
    intr = np.stack([np.asarray(R.intrinsics_for(17, 33), np.float32) * (1 + 0.01 * v) for v in range(3)])   # [V, 4]: one camera model per view
    kw = dict(z_range=R.Z_RANGE, max_step=0.5)
    got = run(depth, intr, ext, **kw)
    refs = [RV.unproject_views(depth[b], intr, ext[b], **kw) for b in range(3)]
    check("ragged batch", got, refs)
    counts = got[4]
    assert len(set(counts.tolist())) == 3
    for b in range(3):                                                        # each body alone
        alone = run(depth[b], intr, ext[b], **kw)
        c = counts[b]
        assert alone[4][0] == c and same([a[0][:c] for a in alone[:4]], [g[b][:c] for g in got[:4]]) and np.array_equal(alone[5][0], got[5][b])
    perm = [2, 0, 1]
    assert same(run(depth[perm], intr, ext[perm], **kw), [g[perm] for g in got])
    assert same(run(depth, intr, ext, **kw), got)                             # the same call twice
    # a wider M: the live rows unchanged, the padding correct
    d, k, e = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (depth, np.broadcast_to(intr, (3, 3, 4)), scan.pack_extrinsics(ext)[0]))
    opts = dict(z_near=R.Z_RANGE[0], z_far=R.Z_RANGE[1], max_step=0.5)
    cnt, ws = ops.depth_views_count(d, k, e, **opts)
    most = int(cnt.max())
    wide = tuple(t.cpu().numpy() for t in ops.depth_views_points(d, k, e, cnt, ws, most + 300, most, **opts))
    assert wide[0].shape[1] == most + 300 and same([w[:, :most] for w in wide[:4]], got[:4]) and np.array_equal(wide[4], got[5])
    assert (bits(wide[0])[:, most:] == 0).all() and (bits(wide[1])[:, most:] == 0).all() and (wide[2][:, most:] == -1).all() and (wide[3][:, most:] == 255).all()
    with pytest.raises(RuntimeError, match="cannot hold"):
        ops.depth_views_points(d, k, e, cnt, ws, most - 1, most, **opts)


# ------------------------------------------------------------------------------------------------ the single-camera call
def test_identity_extrinsics_and_the_unchanged_single_camera_path():
    depth, intr = R.scene(48, 80, seed=7)
    one, rec = launches(lambda: scan.ScanBatch.from_depth(depth[None], intr, DEV, z_range=R.Z_RANGE))
    assert rec == [("depth_count_kernel", "B=1 H=48 W=80 u16=0"), ("depth_scan_kernel", "B=1 tiles=15"),
                   ("depth_emit_kernel", "B=1 H=48 W=80 u16=0")]              # the launch list of the parent commit
    assert tuple(one.viewpoints.shape) == (1, 3) and one.view is None and one.view_first is None
    rig, rec = launches(lambda: scan.ScanBatch.from_depth(depth[None], intr, DEV, extrinsics=np.eye(3, 4, dtype=np.float32)[None], z_range=R.Z_RANGE))
    assert [k for k, _ in rec] == ["depth_views_count_kernel", "depth_scan_kernel", "depth_views_emit_kernel"]
    for a, b in ((rig.points, one.points), (rig.normals, one.normals)):
        assert torch.equal(a + 0.0, b + 0.0)                                  # values: the sign of a zero may differ
    assert torch.equal(rig.pixels, one.pixels) and torch.equal(rig.counts, one.counts) and np.array_equal(rig.host_counts, one.host_counts)
    assert tuple(rig.viewpoints.shape) == (1, 1, 3) and (rig.viewpoints == 0).all()
    assert rig.view.dtype == torch.uint8 and (rig.view[0, :int(rig.host_counts[0])] == 0).all()
    assert rig.view_first.cpu().tolist() == [[0, int(rig.host_counts[0])]]
    part = rig.select(slice(0, 1))
    assert torch.equal(part.view, rig.view) and torch.equal(part.view_first, rig.view_first) and torch.equal(part.viewpoints, rig.viewpoints)
