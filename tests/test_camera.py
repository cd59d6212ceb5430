"""sh_camera_rays on the GPU against tests/camera_ref.py: the ray table, the limit and `complete` bit for bit, for the three
invertible coefficient sets and the folding one, three cameras of different intrinsics in one launch, and a camera alone against
the same camera inside the batch."""
import numpy as np
import pytest
import torch

from semantichuman_amd import ops, scan
from tests import camera_ref as C
from tests.launch_record import launches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SETS = {"azure": C.AZURE, "barrel": C.BARREL, "brown5": C.BROWN5, "folding": C.FOLDING}
INTRS = np.asarray([C.INTR, (26.5, 29.0, 18.25, 14.5), (31.0, 30.0, 16.0, 12.125)], np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("name", sorted(SETS))
def test_bits_against_the_reference(name):
    d = SETS[name] if len(SETS[name]) in (4, 5, 8) else C.pad8(SETS[name])                # brown5 goes in as 5 coefficients: padded by the wrapper
    (cr, rec) = launches(lambda: scan.camera_rays(INTRS, d, (C.H, C.W), DEV))
    assert [k for k, _ in rec] == ["camera_rays_kernel", "camera_limit_kernel"]
    assert cr.lead == (3,) and cr.shape == (C.H, C.W) and np.array_equal(cr.coeffs.cpu().numpy(), np.tile(C.pad8(d), (3, 1)))
    rays, limit = cr.rays.cpu().numpy(), cr.limit.cpu().numpy()
    _, _, complete = ops.camera_rays(cr.intrinsics, cr.coeffs, C.H, C.W)
    complete = complete.cpu().numpy()
    for c in range(3):
        r, lim, comp = C.camera_rays(INTRS[c], d, C.H, C.W)
        assert np.array_equal(bits(rays[c]), bits(r)), "rays of camera %d" % c
        assert bits(limit[c:c + 1])[0] == bits(np.asarray([lim], np.float32))[0], (limit[c], lim)
        assert complete[c] == comp
        alone = scan.camera_rays(INTRS[c], d, (C.H, C.W), DEV)
        assert alone.lead == () and torch.equal(alone.rays.view(torch.int32), cr.rays[c].view(torch.int32))
        assert torch.equal(alone.limit, cr.limit[c]) and alone.complete == bool(comp)
    assert cr.complete == (name != "folding")
    if name == "folding":
        nan = np.isnan(rays[..., 0])
        assert 0 < nan.sum() < nan.size and (limit > 0).all()


def test_a_violent_set():
    """A set that folds a few pixels from the centre: nearly every ray NaN, the limit tiny, complete 0 - the reference's words."""
    d = C.pad8((-400.0,))
    cr = scan.camera_rays(C.INTR, d, (C.H, C.W), DEV)
    r, lim, comp = C.camera_rays(C.INTR, d, C.H, C.W)
    rays = cr.rays.cpu().numpy()
    assert np.array_equal(np.isnan(rays), np.isnan(r)) and np.array_equal(bits(np.nan_to_num(rays)), bits(np.nan_to_num(r)))
    assert float(cr.limit) == float(lim) and cr.complete == bool(comp) and not cr.complete
