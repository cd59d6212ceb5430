"""Depth images on the GPU (sh_depth_count, sh_depth_points, scan.unproject_depth, ScanBatch.from_depth) against the host
reference of tests/depth_ref.py: points, pixels, counts, padding and the set of unknown normals bitwise, known normals within
one fp32 rounding; every option; ragged batches; determinism over batch, padding and width; the plumbing into the Chamfer loss."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import ops, scan
from tests import depth_ref as R
from tests import normals_ref as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1, 1), (1, 70), (70, 1), (17, 33), (48, 80)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


def run(depth, intr, **kw):
    """scan.unproject_depth on the device -> (points, normals, pixel, counts) on the host."""
    return tuple(t.cpu().numpy() for t in scan.unproject_depth(depth, intr, device=DEV, **kw))


@functools.lru_cache(maxsize=None)
def scene_run(H, W):
    """The scene at H x W with z_range, its GPU result and its reference: computed once, shared, read-only."""
    depth, intr = R.scene(H, W)
    return depth, intr, run(depth, intr, z_range=R.Z_RANGE), R.unproject(depth, intr, z_range=R.Z_RANGE)


def check(what, got, refs):
    """Item 1 of the contract: counts, pixel, points and every padding row bitwise; the unknown normals the same rows; every known
    normal within 2^-23 per component (one fp32 rounding of an fp64 value whose own error is below 1e-14)."""
    points, normals, pixel, counts = got
    rp, rn, rpix, rc = R.pack(refs, width=points.shape[1])
    assert np.array_equal(counts, rc), what
    assert points.shape[1] == max(int(rc.max()), 1) or points.shape[1] >= rc.max(), what
    assert np.array_equal(pixel, rpix), what
    assert np.array_equal(bits(points), bits(rp)), what
    live = np.arange(points.shape[1])[None, :] < counts[:, None]
    assert (bits(normals)[~live] == 0).all() and (bits(points)[~live] == 0).all() and (pixel[~live] == -1).all(), what
    unknown, r_unknown = np.abs(normals).sum(-1) == 0, np.abs(rn).sum(-1) == 0
    assert np.array_equal(unknown, r_unknown), what
    known = live & ~r_unknown
    err = np.abs(normals[known].astype(np.float64) - rn[known].astype(np.float64))
    print("%s: %d rows, %d known normals, largest component error %.3e, %d of them bit-equal"
          % (what, int(counts.sum()), int(known.sum()), err.max() if err.size else 0.0, int((bits(normals[known]) == bits(rn[known])).all(-1).sum())))
    assert (err <= 2.0 ** -23).all(), what
    if known.any():
        assert np.abs(np.linalg.norm(normals[known].astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22, what


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("H, W", SIZES)
def test_bitwise_against_the_reference(H, W):
    depth, intr, got, ref = scene_run(H, W)
    check("%d x %d" % (H, W), got, [ref])
    if H * W > 1:
        assert 0 < len(ref.pixel) < H * W                                     # the holes took some
    if min(H, W) == 1:
        assert (np.abs(got[1]).sum(-1) == 0).all()                            # a single row or column has one tangent: every normal unknown
    else:
        assert ref.known.any()                                                # known normals are compared


# ------------------------------------------------------------------------------------------------ 2
OPTIONS = {
    "mask": dict(mask=np.random.default_rng(5).random((17, 33)) > 0.3),
    "z_range": dict(z_range=(1.45, 5.0)),
    "max_step": dict(max_step=0.1, z_range=R.Z_RANGE),
    "max_step=0": dict(max_step=0.0, z_range=R.Z_RANGE),
    "drop_isolated": dict(drop_isolated=True, z_range=R.Z_RANGE),
    "drop_isolated, max_step": dict(drop_isolated=True, max_step=0.02, z_range=R.Z_RANGE),
    "drop_isolated, max_step=0, stride=2": dict(drop_isolated=True, max_step=0.0, stride=2, z_range=R.Z_RANGE),
    "stride=2": dict(stride=2, z_range=R.Z_RANGE),
    "stride=3": dict(stride=3, z_range=R.Z_RANGE),
    "stride=40": dict(stride=40, z_range=R.Z_RANGE),
}


@pytest.mark.parametrize("name", list(OPTIONS))
def test_options(name):
    depth, intr = R.scene(17, 33)[0], R.intrinsics_for(17, 33)
    kw = OPTIONS[name]
    ref = R.unproject(depth, intr, **kw)
    check(name, run(depth, intr, **kw), [ref])
    plain = scene_run(17, 33)[3]
    assert len(ref.pixel) < len(plain.pixel) or not np.array_equal(ref.known, plain.known), name      # the option did something


@pytest.mark.parametrize("scale", [0.001, 0.00005])
def test_sixteen_bit_words(scale):
    """16-bit input gives the bits of the fp32 image that holds the same words as floats; at 0.00005 the plane's words are above
    32767 - read as unsigned."""
    depth, intr = R.scene(17, 33)
    words = R.to_words(depth, scale)
    assert (words == 0).any() and (scale == 0.001 or (words > 32767).any())
    got = run(words, intr, depth_scale=scale, z_range=R.Z_RANGE)
    check("uint16 at %g" % scale, got, [R.unproject(words, intr, depth_scale=scale, z_range=R.Z_RANGE)])
    assert same(got, run(words.astype(np.float32), intr, depth_scale=scale, z_range=R.Z_RANGE))
    carried = torch.from_numpy(words.view(np.int16)).to(DEV)                  # the words as an int16 tensor already on the device
    assert same(got, run(carried, intr, depth_scale=scale, z_range=R.Z_RANGE))
    assert got[3][0] > 0


# ------------------------------------------------------------------------------------------------ 3
@functools.lru_cache(maxsize=None)
def ragged():
    H, W = 17, 33
    intr = np.asarray([R.intrinsics_for(H, W), R.intrinsics_for(H, W + 6), R.intrinsics_for(H + 3, W)], np.float32)
    full = R.sphere_over_plane(H, W, intr[0])[0]
    images = np.stack([full, R.holes(R.sphere_over_plane(H, W, intr[1])[0], seed=2), np.zeros((H, W), np.float32)])
    return images, intr, run(images, intr, z_range=R.Z_RANGE, max_step=0.2)


def test_ragged_batch():
    images, intr, got = ragged()
    kw = dict(z_range=R.Z_RANGE, max_step=0.2)
    refs = [R.unproject(images[b], intr[b], **kw) for b in range(3)]
    check("ragged", got, refs)
    assert got[3].tolist() == [17 * 33, len(refs[1].pixel), 0] and 0 < got[3][1] < 17 * 33
    M = got[0].shape[1]
    for b in range(3):                                                        # the same bits as the image run alone
        alone = run(images[b], intr[b], **kw)
        m = max(int(got[3][b]), 1)
        assert alone[0].shape[1] == m and alone[3][0] == got[3][b]
        assert same([t[:, :m] for t in alone[:3]], [t[b:b + 1, :m] for t in got[:3]]), b
    perm = [2, 0, 1]
    assert same(run(images[perm], intr[perm], **kw), [t[perm] for t in got])
    once = run(images, intr[0], **kw)
    assert same(once, run(images, np.broadcast_to(intr[0], (3, 4)), **kw))
    assert not same(once, got)                                                # the per-body intrinsics were really read
    assert M == 17 * 33


# ------------------------------------------------------------------------------------------------ 4
def test_determinism_and_width():
    depth, intr, got, ref = scene_run(48, 80)
    assert same(got, run(depth, intr, z_range=R.Z_RANGE))
    d, k = dev(depth[None]), dev(np.asarray([intr], np.float32))
    kw = dict(z_near=R.Z_RANGE[0], z_far=R.Z_RANGE[1])
    counts, ws = ops.depth_count(d, k, **kw)
    most = int(counts.cpu()[0])
    assert most == len(ref.pixel)
    wide = tuple(t.cpu().numpy() for t in ops.depth_points(d, k, counts, ws, most + 301, most, **kw))
    assert wide[0].shape == (1, most + 301, 3)
    assert same([t[:, :most] for t in wide], [t[:, :most] for t in got[:3]])
    assert (bits(wide[0])[:, most:] == 0).all() and (bits(wide[1])[:, most:] == 0).all() and (wide[2][:, most:] == -1).all()
    with pytest.raises(RuntimeError, match="cannot hold"):
        ops.depth_points(d, k, counts, ws, most - 1, most, **kw)


# ------------------------------------------------------------------------------------------------ 5
def test_from_depth_plumbs_into_the_chamfer_loss():
    """ScanBatch.from_depth against a ScanBatch the existing constructor builds from the same rows: gated and visibility-masked
    Chamfer values and gradients bit-equal; select() keeps pixels with points."""
    depth, intr, got, ref = scene_run(48, 80)
    images = np.stack([depth, depth[::-1].copy()])
    scans = scan.ScanBatch.from_depth(images, intr, DEV, z_range=R.Z_RANGE, max_step=0.2)
    assert scans.perm is None and scans.pixels.dtype == torch.int32 and scans.pixels.shape == scans.points.shape[:2]
    assert torch.equal(scans.viewpoints, torch.zeros((2, 3), device=DEV)) and scans.host_counts.tolist() == scans.counts.cpu().tolist()
    pts, nrm = scans.points.cpu().numpy(), scans.normals.cpu().numpy()
    built = scan.ScanBatch([pts[b, :m] for b, m in enumerate(scans.host_counts)], DEV,
                           normals=[nrm[b, :m] for b, m in enumerate(scans.host_counts)], viewpoints=[0.0, 0.0, 0.0])
    assert built.pixels is None and torch.equal(built.points, scans.points) and torch.equal(built.counts, scans.counts)
    x, f = N.bodies("small_ae.npz", 2)
    n = x.shape[1] - 1
    x = (0.25 * x + np.array([0.0, 0.0, 1.6], np.float32)).astype(np.float32)          # in front of the camera, among the scan's points

    def loss_and_grad(s, **kw):
        xt = dev(x).requires_grad_(True)
        loss = scan.chamfer(xt, s, **kw)
        loss.sum().backward()
        return loss.detach().cpu().numpy(), xt.grad.cpu().numpy()

    for kw in (dict(normal_angle=60.0, trunc=0.5, normal_faces=f), dict(normal_angle=60.0, trunc=0.5, faces=f, gate_on="surface"),
               dict(visibility="viewpoint", faces=f, w_model_to_scan=1.0), dict(robust="huber", robust_scale=0.05, faces=f)):
        a, b = loss_and_grad(scans, **kw), loss_and_grad(built, **kw)
        assert np.isfinite(a[0]).all() and np.abs(a[1]).max() > 0, kw
        assert same(a, b), kw
    part = scans.select(slice(1, 2))
    assert torch.equal(part.pixels, scans.pixels[1:2]) and torch.equal(part.points, scans.points[1:2])
    m = int(part.host_counts[0])
    v, u = np.divmod(part.pixels[0, :m].cpu().numpy(), 80)
    z = part.points[0, :m, 2].cpu().numpy()
    assert np.array_equal(z, images[1][v, u])                                  # each row's pixel is where its depth came from
