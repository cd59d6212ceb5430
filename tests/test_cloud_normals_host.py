"""Cloud normals on the host (no GPU): the study of how good a k-neighbour PCA normal is on surface samples of the golden
templates, pinned; the conditioning of the test inputs (no point is left out of the GPU comparison); the fixed-sweep Jacobi of
the kernel against numpy.linalg.eigh; and the argument errors that need no device."""
import numpy as np
import pytest

from semantichuman_amd import scan
from tests import cloud_normals_ref as R


@pytest.mark.parametrize("case", range(len(R.STUDY_CASES)))
def test_study_figures_are_pinned(case):
    """Unsigned angle between the estimated normal and the normal of the face the sample came from, float64 reference:
    template6890, M = 5000, k = 16: median 1.241 deg, 90th percentile 3.943 deg; the same with k = 8 and noise 0.002: 4.674 /
    10.486; small_ae, M = 1000, k = 16: 4.612 / 14.354.  No point has a relative gap (l1 - l0) / l2 below 1e-3."""
    med, p90, gap_min, share, spread = R.study_case(*R.STUDY_CASES[case])
    print("study %s: median %.3f deg, p90 %.3f deg, smallest gap %.3e, largest spread %.2f" % (R.STUDY_CASES[case], med, p90, gap_min, spread))
    assert abs(med - R.STUDY_MEDIAN[case]) <= R.STUDY_TOL and abs(p90 - R.STUDY_P90[case]) <= R.STUDY_TOL
    assert share == 0.0 and spread <= R.SPREAD_MAX


@pytest.mark.parametrize("name,M", [("small_ae.npz", 63), ("small_ae.npz", 1000)])
def test_every_point_of_the_test_inputs_can_be_compared(name, M):
    """Over every k the GPU test runs: every point has a normal, T / l2 stays below the SPREAD_MAX the angle bound's constant
    assumes, and for k >= 8 no point has a gap below GAP_MIN (smallest met: 7.9e-3, at M = 63, k = 8).  k = 3 is another matter: a
    point and its two nearest neighbours form a thin triangle often enough that 4.2 % of the M = 1000 points (5.8 % of the 5000
    template samples) have a gap below GAP_MIN, down to 4.1e-7.  The bound grows with 1 / gap and is still below 1e-5 rad there,
    so the GPU test leaves no point out instead of exempting more than its 1 % cap allows."""
    for k, (r2, cnt, S1, S2) in R.reference(name, M).items():
        n, var, gap, spread, lam = R.finish(cnt, S1, S2)
        assert (np.abs(n).sum(1) > 0).all() and (cnt >= min(k, M)).all()
        share = float((gap < R.GAP_MIN).mean())
        print("%s M=%d k=%d: smallest gap %.3e, share below %.0e: %.4f, largest spread %.2f, largest bound %.3e rad"
              % (name, M, k, gap.min(), R.GAP_MIN, share, spread.max(), R.angle_bound(cnt, gap).max()))
        assert spread.max() <= R.SPREAD_MAX and R.angle_bound(cnt, gap).max() <= 1e-5
        assert share == 0.0 or k == 3


def test_fixed_sweep_jacobi_matches_eigh():
    """The kernel's eight fixed sweeps leave nothing off the diagonal (four already reach the rounding floor), on the test
    clouds' covariances and on random, rank-one and singular matrices; its normal is eigh's to 1e-12 / gap."""
    r2, cnt, S1, S2 = R.reference("small_ae.npz", 1000)[16]
    C = R.covariance(cnt, S1, S2)
    rs = np.random.RandomState(0)
    A = rs.randn(3000, 3, 3)
    A = A + A.transpose(0, 2, 1)
    A[:1000] = np.einsum("mi,mj->mij", A[:1000, 0], A[:1000, 0])
    A[1000:2000, 2, :] = 0
    A[1000:2000, :, 2] = 0
    for mats in (C, A):
        assert np.nanmax(R.jacobi_f64(mats, 4)[2]) <= 2.0 ** -53 and np.nanmax(R.jacobi_f64(mats, R.SWEEPS)[2]) <= 2.0 ** -53
    diag, vec, _ = R.jacobi_f64(C)
    lam, ref = np.linalg.eigh(C)
    n = vec[np.arange(len(C)), :, diag.argmin(1)]
    assert np.abs(np.sort(diag, 1) - lam).max() <= 1e-14 * np.abs(lam).max()
    gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    assert (R.unsigned_angle(n, ref[:, :, 0]) <= 1e-12 / gap).all()


def test_reference_rules_on_degenerate_clouds():
    """The unknown rule and the tie rule of the reference itself: a collinear cloud has no normal, a plane has (0, 0, 1) and
    variation 0, and on the lattice every tie at the k-th distance is a member."""
    n, var, r2, cnt, gap, spread = R.estimate(R.collinear(), 8)
    assert (n == 0).all() and (var == 0).all()
    n, var, r2, cnt, gap, spread = R.estimate(R.planar(), 16)
    assert np.array_equal(n, np.tile(np.float32([0, 0, 1]), (len(n), 1))) and (var == 0).all()
    n, var, r2, cnt, gap, spread = R.estimate(R.lattice(), 16)
    assert (cnt > 16).any() and (cnt >= 16).all() and cnt[14] >= 16 and r2[14] == 2.0     # six coincident points, then the 1-ring


def test_argument_errors_need_no_device():
    cloud = [np.zeros((5, 3), np.float32)]
    for bad in (2, 65, 16.5, None):
        with pytest.raises(ValueError, match="neighbour count"):
            scan.ScanBatch(cloud, "cpu", normals="estimate", normal_k=bad)
        with pytest.raises(ValueError, match="neighbour count"):
            scan.estimate_normals(None, k=bad)
    with pytest.raises(ValueError, match="'estimate'"):
        scan.ScanBatch(cloud, "cpu", normals="pca")
    for bad in (np.zeros(4), np.zeros((2, 3)), [np.zeros((4, 3))], np.zeros((1, 5, 2)), "front"):
        with pytest.raises(ValueError, match="viewpoints"):
            scan.ScanBatch(cloud, "cpu", normals="estimate", viewpoints=bad)
    with pytest.raises(ValueError, match="NaN"):
        scan.ScanBatch(cloud, "cpu", normals="estimate", viewpoints=[np.nan, 0, 0])
    assert scan.pack_viewpoints([1, 2, 3], [5, 4], 5).shape == (2, 3)
    assert scan.pack_viewpoints(np.zeros((2, 3)), [5, 4], 5).shape == (2, 3)
    per_point = scan.pack_viewpoints([np.ones((5, 3)), np.ones((4, 3))], [5, 4], 5)
    assert per_point.shape == (2, 5, 3) and (per_point[1, 4] == 0).all()
    # normal_k and viewpoints are read only with normals="estimate": an array, or None, behaves as ever - no device needed to see it
    b = scan.ScanBatch(cloud, "cpu", normals=[np.tile([0.0, 0.0, 2.0], (5, 1))], normal_k=-1, viewpoints="ignored")
    assert np.array_equal(b.normals.numpy()[0], np.tile(np.float32([0, 0, 1]), (5, 1)))
    assert scan.ScanBatch(cloud, "cpu", normal_k=-1).normals is None
