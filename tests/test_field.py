"""scan.DepthField against tests/field_ref.py, bit for bit: cls, z and nearest on the sphere-over-plane scene with holes at every
shape the kernels treat differently, fp32 and 16-bit words, mask, z_range, the constructed tie masks, and a ragged batch against
each image alone and permuted."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import scan
from tests import depth_ref as D
from tests import field_ref as R
from tests.launch_record import launches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 3 x 600: a row wider than twice the row pass's 256 threads (a third, partial round per thread) and more than nine of the
# column pass's 64-thread workgroups, the last one partial.  The row pass keeps a whole row in LDS: there is no chunk edge.
SHAPES = [(1, 1), (1, 70), (70, 1), (17, 33), (48, 80), (3, 600)]


def same(got, want):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))


def check(fld, refs):
    for b, r in enumerate(refs):
        assert same(fld.cls[b], r.cls), "cls of image %d" % b
        assert same(fld.z[b], r.z), "z of image %d" % b
        assert same(fld.nearest[b], r.nearest), "nearest of image %d" % b


@functools.lru_cache(maxsize=None)
def scene(H, W):
    """The scene at H x W with a mask that cuts the sphere's left half away and a few plane pixels in, and its references."""
    depth, intr = D.scene(H, W, seed=H + W)
    on_sphere = D.sphere_over_plane(H, W, intr)[1]
    mask = (on_sphere & (np.arange(W)[None, :] >= W // 2)) | (np.random.default_rng(W).random((H, W)) < 0.02)
    return depth, intr, mask


@pytest.mark.parametrize("H, W", SHAPES)
def test_field_bits(H, W):
    depth, intr, mask = scene(H, W)
    for opts in (dict(), dict(z_range=D.Z_RANGE), dict(mask=mask), dict(mask=mask, z_range=(1.0, 1.9))):
        fld = scan.DepthField.from_depth(depth, intr, DEV, **opts)
        assert fld.shape == (H, W) and len(fld) == 1 and tuple(fld.intrinsics.shape) == (1, 4)
        check(fld, [R.field(depth, intr, **opts)])
    if H * W > 100:                                                        # the scene does hold every class
        assert set(np.unique(R.field(depth, intr, mask=mask, z_range=(1.0, 1.9)).cls)) == {0, 1, 2}


@pytest.mark.parametrize("H, W", [(17, 33), (3, 600)])
def test_field_bits_16_bit_words(H, W):
    """Words at 0.05 mm: the plane at 2 m is the word 40000, above 32767 - read unsigned."""
    depth, intr, mask = scene(H, W)
    words = D.to_words(depth, 5e-5)
    assert (words > 32767).any() and (words == 0).any()
    for opts in (dict(depth_scale=5e-5), dict(depth_scale=5e-5, z_range=(0.5, 1.9), mask=mask)):
        check(scan.DepthField.from_depth(words, intr, DEV, **opts), [R.field(words, intr, **opts)])
        as_int16 = torch.from_numpy(words.view(np.int16)).to(DEV)
        check(scan.DepthField.from_depth(as_int16, intr, **opts), [R.field(words, intr, **opts)])


def test_constructed_tie_masks():
    """A class image is made from depth alone: 2.0 is SURFACE, 9.0 beyond z_range is EMPTY, 0.0 is UNKNOWN."""
    value = np.asarray([9.0, 0.0, 2.0], np.float32)
    for name, cls in R.tie_masks().items():
        fld = scan.DepthField.from_depth(value[cls], (10.0, 10.0, 1.0, 1.0), DEV, z_range=D.Z_RANGE)
        ref = R.field_of_classes(cls, (10.0, 10.0, 1.0, 1.0), z=value[cls])
        assert same(fld.cls[0], ref.cls), name
        assert same(fld.nearest[0], ref.nearest), name
    none = scan.DepthField.from_depth(value[R.tie_masks()["none"]], (10.0, 10.0, 1.0, 1.0), DEV, z_range=D.Z_RANGE)
    assert (none.nearest == -1).all() and (none.cls == 0).all()


def test_batch_equals_each_image_alone_and_permuted():
    """Images of one shape with different content (a batch is ragged in what it holds, not in its shape): every image's planes
    are those of the image alone, wherever it stands in the batch."""
    H, W = 17, 33
    depth, intr, mask = scene(H, W)
    images = [depth, D.holes(D.fronto_plane(H, W), seed=3), np.full((H, W), 9.0, np.float32), np.roll(depth, 5, axis=1), np.zeros((H, W), np.float32)]
    intrs = np.asarray([intr] * len(images), np.float32)
    masks = np.stack([mask, ~mask, mask, np.ones_like(mask), mask])
    opts = dict(z_range=D.Z_RANGE)
    (batch, rec) = launches(lambda: scan.DepthField.from_depth(np.stack(images), intrs, DEV, mask=masks, **opts))
    assert [k for k, _ in rec] == ["depth_field_column_kernel", "depth_field_row_kernel"]
    refs = [R.field(d, intr, mask=m, **opts) for d, m in zip(images, masks)]
    check(batch, refs)
    assert (batch.nearest[2] == -1).all() and (batch.nearest[4] >= 0).all()   # all EMPTY; all UNKNOWN
    for b in range(len(images)):
        check(scan.DepthField.from_depth(images[b], intr, DEV, mask=masks[b], **opts), [refs[b]])
    perm = [3, 0, 4, 2, 1]
    check(scan.DepthField.from_depth(np.stack(images)[perm], intrs, DEV, mask=masks[perm], **opts), [refs[b] for b in perm])
    check(batch.select(slice(1, 3)), refs[1:3])
