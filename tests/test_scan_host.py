"""Fitting to point clouds, the part that needs no GPU: ScanBatch packing, argument validation of the new entry points before any
device call, the no-CPU-path errors, and the float64 check of the search test's exemption cap on the host mirror of the header's
fp32 distance expression."""
import ctypes

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, scan, synthetic
from tests import scan_ref as R


def test_scanbatch_packs_ragged_clouds():
    rs = np.random.RandomState(0)
    clouds = [rs.randn(m, 3) for m in (5, 1, 9)]
    sb = scan.ScanBatch(clouds, "cpu")
    assert len(sb) == 3 and tuple(sb.points.shape) == (3, 9, 3)
    assert sb.points.dtype == torch.float32 and sb.counts.dtype == torch.int32
    assert sb.counts.tolist() == [5, 1, 9] and sb.host_counts.tolist() == [5, 1, 9]
    for b, c in enumerate(clouds):
        assert np.array_equal(sb.points[b, :c.shape[0]].numpy(), c.astype(np.float32))
        assert float(sb.points[b, c.shape[0]:].abs().sum()) == 0.0
    one = sb.select(slice(1, 2))
    assert len(one) == 1 and one.counts.tolist() == [1] and one.points.data_ptr() == sb.points[1:2].data_ptr()


def test_scanbatch_dense_array_round_trips():
    a = np.random.RandomState(1).randn(4, 7, 3).astype(np.float32)
    sb = scan.ScanBatch(a, "cpu")
    assert np.array_equal(sb.points.numpy(), a) and sb.counts.tolist() == [7] * 4
    assert np.array_equal(scan.ScanBatch(torch.from_numpy(a), "cpu").points.numpy(), a)


@pytest.mark.parametrize("bad", [[], [np.zeros((3, 2))], [np.zeros(3)], [np.array([[0.0, np.nan, 0.0]])],
                                 [np.zeros((2, 3)), np.array([[np.inf, 0.0, 0.0]])]])
def test_scanbatch_rejects_bad_input(bad):
    with pytest.raises(ValueError):
        scan.ScanBatch(bad, "cpu")


def test_new_entry_points_validate_before_the_device():
    """Null pointers: -1 and "null pointer", for every new entry point, before any device call.  The header's contract for sizes:
    negative B / nq / nt / chunks are invalid arguments; B == 0 (and nq == 0) succeed without a launch."""
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(64)                           # never dereferenced on the host, never reaches a launch in these calls
    f = ctypes.c_float
    rc = lib.sh_nearest_points(null, 0, 0, null, null, 0, 0, null, null, 0, 0, 0, null, null, null, 0, null)
    assert rc == -1 and b"null pointer" in lib.sh_last_error()
    rc = lib.sh_chamfer_fwd(null, 0, null, null, 0, 0, null, 0, f(0), f(0), 0, null, null, null)
    assert rc == -1 and b"null pointer" in lib.sh_last_error()
    rc = lib.sh_chamfer_bwd(null, 0, 0, 0, null, 0, 0, null, null, null, null, null, null, 0, null, f(0), f(0), null, 0, null, null)
    assert rc == -1 and b"null pointer" in lib.sh_last_error()
    for B, nq, nt, chunks in ((-1, 4, 4, 0), (1, -4, 4, 0), (1, 4, -4, 0), (1, 4, 4, -1)):
        rc = lib.sh_nearest_points(some, 12, nq, null, some, 12, nt, null, null, 0, B, chunks, some, some, null, 0, null)
        assert rc == -1 and b"negative size" in lib.sh_last_error(), (B, nq, nt, chunks)
    assert lib.sh_nearest_points(some, 12, 4, null, some, 12, 4, null, null, 0, 0, 0, some, some, null, 0, null) == 0      # B == 0
    assert lib.sh_nearest_points(some, 12, 0, null, some, 12, 4, null, null, 0, 2, 0, some, some, null, 0, null) == 0      # nq == 0
    assert lib.sh_chamfer_fwd(some, 4, null, null, 5, 4, null, 0, f(1), f(0), 0, some, some, null) == 0                   # B == 0
    assert lib.sh_chamfer_fwd(some, 4, null, null, 5, 4, null, 0, f(1), f(0), -1, some, some, null) == -1
    assert lib.sh_chamfer_fwd(some, 4, null, null, 3, 4, null, 0, f(1), f(0), 1, some, some, null) == -1                  # n > rows
    assert lib.sh_chamfer_fwd(some, 4, null, null, 5, 4, null, 0, f(1), f(-1), 1, some, some, null) == -1                 # w_ms < 0
    assert lib.sh_chamfer_bwd(some, 15, 5, 4, some, 12, 4, null, some, some, null, null, null, 0, some, f(1), f(0), some, 0, some,
                              null) == 0                                                                                  # B == 0
    assert lib.sh_chamfer_bwd(some, 15, 5, 4, some, 12, 4, null, some, some, some, null, null, 0, some, f(1), f(0), some, 1, some,
                              null) == -1                                                                                 # idx_ms without d2_ms
    # a split needs its workspace: refused on the host (status -3), nothing launched
    assert lib.sh_nearest_points_workspace(1, 100, 1000, 4) == 4 * 100 * 8
    assert lib.sh_nearest_points_workspace(1, 100, 1000, 1) == 0
    rc = lib.sh_nearest_points(some, 300, 100, null, some, 3000, 1000, null, null, 0, 1, 4, some, some, null, 0, null)
    assert rc == -3 and b"workspace" in lib.sh_last_error()


def test_automatic_split_fills_the_chip_only_when_needed():
    lib = _lib.load()
    assert lib.sh_nearest_points_chunks(64, 50000, 6890) == 1           # 49 query tiles x 64 bodies already exceed the chip
    assert lib.sh_nearest_points_chunks(1, 6890, 20011) > 1
    assert lib.sh_nearest_points_chunks(1, 6890, 100) == 1              # one LDS tile of targets cannot be split
    assert lib.sh_nearest_points_chunks(0, 0, 0) == 1


def test_no_cpu_path():
    x = torch.zeros((2, 5, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        scan.nearest(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        scan.chamfer(x, [np.zeros((3, 3)), np.zeros((2, 3))])
    assert callable(editing.fit_scan)


@pytest.mark.parametrize("M", [63, 1000, 20011])
def test_exemption_cap_holds_for_the_fp32_difference_form(M):
    """The GPU search test exempts a query from the index comparison when float64's two best distinct distances lie within 1e-5
    of each other, and caps the share of such queries at 0.1 %.  Checked here on the inputs that test builds (synth_batch seed 3 on
    the box_sphere(42, 42, 20) vertices, both directions), with the header's fp32 expression evaluated in numpy: the fp32 form
    violates neither (b) nor (c), duplicates among the targets resolve to the lowest index, and the exempt share stays under
    the cap."""
    v, _ = synthetic.box_sphere(42, 42, 20)
    n = v.shape[0]
    x = R.model_points(v, 2, seed=3)
    s = R.make_scans(x, n, [M, M], seed=11)[0]
    for q, t in ((x[0, :n], s), (s, x[0, :n])):                           # model -> scan, scan -> model
        idx, d2 = R.nearest_f32(q, t)
        exempt = R.check_against_f64(q, t, idx, d2)
        assert exempt <= R.EXEMPT_CAP * q.shape[0], (exempt, q.shape[0])
