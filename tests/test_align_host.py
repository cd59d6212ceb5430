"""Scan alignment without a GPU: the new symbols and exports, argument validation before the device is touched, scan.Pose's
packing and algebra, the refusal of CPU tensors, and the float64 references of tests/align_ref.py pinned against the CPU study
the feature was specified from (moment start recovers, identity start with scan -> model only collapses)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import semantichuman_amd as sh
from semantichuman_amd import _lib, editing, ops, scan
from semantichuman_amd.hierarchy import load_hierarchy
from tests import align_ref as A
from tests import scan_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NEW = ["sh_align_ranges", "sh_align_partials_bytes", "sh_align_moments", "sh_align_solve", "sh_transform_points"]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "sh_kernels.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and ("SH_API" in header and name + "(" in header) and hasattr(lib, name), name
    for name in ("align_moments", "align_solve", "transform_points"):
        assert callable(getattr(ops, name))
    assert ops.ALIGN_MODES == {"translation": 0, "rigid": 1, "similarity": 2}
    for k, v in (("SH_ALIGN_PARTIAL", ops.ALIGN_PARTIAL), ("SH_ALIGN_MOMENTS", ops.ALIGN_MOMENTS)):
        assert "#define %s %d" % (k, v) in header
    assert sh.Pose is scan.Pose and sh.align is scan.align and sh.moment_pose is scan.moment_pose
    assert sh.register_scan is editing.register_scan and sh.fit_scan is editing.fit_scan
    assert callable(scan.pose_update)


def test_argument_validation_without_a_device():
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)                      # p: never dereferenced - validation comes first
    inf = float("inf")
    assert lib.sh_align_moments(null, 0, 1, null, p, 3, 1, 1, null, 0, p, p, null, null, inf, 0.0, 1, p, 1 << 20, null) == -1
    assert b"null pointer" in lib.sh_last_error()
    assert lib.sh_align_moments(p, 3, 1, null, p, 3, 1, 1, null, 0, p, p, null, null, inf, 0.0, -1, p, 1 << 20, null) == -1
    assert lib.sh_align_moments(p, 3, -1, null, p, 3, 1, 1, null, 0, p, p, null, null, inf, 0.0, 1, p, 1 << 20, null) == -1
    assert lib.sh_align_moments(p, 3, 1, null, p, 3, 1, 2, null, 0, p, p, null, null, inf, 0.0, 1, p, 1 << 20, null) == -1      # n > rows
    assert lib.sh_align_moments(p, 3, 1, null, p, 3, 1, 1, null, 0, p, p, null, null, inf, 0.5, 1, p, 1 << 20, null) == -1      # w_ms > 0, no idx_ms
    assert lib.sh_align_moments(p, 3, 1, null, p, 3, 1, 1, null, 0, p, p, null, null, float("nan"), 0.0, 1, p, 1 << 20, null) == -1
    assert lib.sh_align_moments(p, 3, 1, null, p, 3, 1, 1, null, 0, p, p, null, null, inf, 0.0, 0, p, 0, null) == 0             # B == 0
    assert lib.sh_align_solve(null, 1, 1, null, 0.0, 2, 1, p, p, p, p, null, null, null) == -1
    assert lib.sh_align_solve(p, 1, 1, null, 0.0, 2, 1, null, null, null, null, null, null, null) == -1                           # nothing to write
    assert lib.sh_align_solve(p, 1, 1, null, 0.0, 2, 1, null, p, p, p, null, null, null) == -1                                    # pose_out without pose_in
    assert lib.sh_align_solve(p, 1, 1, null, 0.0, 3, 1, p, p, p, p, null, null, null) == -1 and b"mode" in lib.sh_last_error()
    assert lib.sh_align_solve(p, 1, 1, null, 0.0, 2, -1, p, p, p, p, null, null, null) == -1
    assert lib.sh_align_solve(p, 1, 1, null, 0.0, 2, 0, p, p, p, p, null, null, null) == 0
    assert lib.sh_transform_points(null, 3, 1, null, p, 1, p, null) == -1
    assert lib.sh_transform_points(p, 3, -1, null, p, 1, p, null) == -1
    assert lib.sh_transform_points(p, 3, 1, null, p, -1, p, null) == -1
    assert lib.sh_transform_points(p, 3, 1, null, p, 0, p, null) == 0
    # the range count is a function of M, n and the direction setting alone
    assert lib.sh_align_ranges(0, 0, 0.0) == 0 and lib.sh_align_ranges(1, 6890, 0.0) == 1 and lib.sh_align_ranges(2048, 6890, 0.0) == 1
    assert lib.sh_align_ranges(2049, 6890, 0.0) == 2 and lib.sh_align_ranges(50000, 6890, 0.5) == 25 + 4
    assert lib.sh_align_partials_bytes(16, 50000, 6890, 0.5) == 16 * 29 * 19 * 8 and lib.sh_align_partials_bytes(0, 5, 5, 0.0) == 0


def test_pose_packing_and_algebra():
    rs = np.random.RandomState(0)
    B = 5
    Rm = np.stack([A.rotation(rs.randn(3), rs.uniform(-90, 90)) for _ in range(B)])
    c = rs.uniform(0.5, 2.0, B)
    t = rs.randn(B, 3)
    P = scan.Pose(torch.from_numpy(c[:, None, None] * Rm), torch.from_numpy(t))
    assert P.packed.dtype == torch.float32 and tuple(P.packed.shape) == (B, 12) and P.packed.is_contiguous() and len(P) == B
    assert torch.equal(P.packed[:, :9].reshape(B, 3, 3), P.A) and torch.equal(P.packed[:, 9:], P.t)
    assert P.A.data_ptr() == P.packed.data_ptr()                           # views of the one buffer the kernels read
    assert np.allclose(P.scale.numpy(), c, rtol=1e-6)                      # scale defaults to det(A)^(1/3)
    for b in range(B):
        assert np.array_equal(P.packed[b].numpy(), A.pack(c[b] * Rm[b], t[b]))
    I = scan.Pose.identity(3, "cpu")
    assert torch.equal(I.A, torch.eye(3).expand(3, 3, 3)) and not I.t.any() and torch.equal(I.scale, torch.ones(3))
    # inverse and compose against the float64 algebra of align_ref, to fp32 rounding of the stored entries
    inv, both = P.inverse(), P.inverse().compose(P)
    for b in range(B):
        Ai, ti = A.inverse(P.A[b].double().numpy(), P.t[b].double().numpy())
        assert np.allclose(inv.A[b].numpy(), Ai, rtol=0, atol=2.0 ** -23 * np.abs(Ai).max())
        assert np.allclose(inv.t[b].numpy(), ti, rtol=0, atol=2.0 ** -22 * max(1.0, np.abs(ti).max()))
        assert np.allclose(both.A[b].numpy(), np.eye(3), atol=1e-6) and np.allclose(both.t[b].numpy(), 0, atol=1e-5)
    assert np.allclose((inv.scale * P.scale).numpy(), 1.0, atol=1e-6) and np.allclose(both.scale.numpy(), 1.0, atol=1e-6)
    x = torch.from_numpy(rs.randn(B, 7, 3).astype(np.float32))
    back = P.to_scan_frame(torch.from_numpy(np.stack([A.apply(P.A[b].double().numpy(), P.t[b].double().numpy(), x[b].double().numpy())
                                                      for b in range(B)]).astype(np.float32)))
    assert np.allclose(back.numpy(), x.numpy(), atol=2e-5)
    sel = P.select(slice(1, 3))
    assert len(sel) == 2 and torch.equal(sel.packed, P.packed[1:3]) and torch.equal(P.clone().packed, P.packed)
    for bad in (lambda: scan.Pose(torch.eye(3), torch.zeros(3)), lambda: scan.Pose(torch.eye(3)[None], torch.zeros(2, 3)),
                lambda: scan.Pose(torch.eye(3)[None], torch.zeros(1, 3), torch.ones(2))):
        with pytest.raises(ValueError):
            bad()


def test_cpu_tensors_raise_and_arguments_are_validated():
    x = torch.zeros((2, 5, 3))
    clouds = [np.zeros((4, 3), np.float32)] * 2
    for call in (lambda: scan.align(x, clouds), lambda: scan.moment_pose(clouds, x), lambda: scan.Pose.identity(2, "cpu").apply(x),
                 lambda: scan.Pose.identity(2, "cpu").apply(scan.ScanBatch(clouds, "cpu"))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    z = torch.zeros((2, 17, 8))
    with pytest.raises(ValueError, match="mode"):
        editing.register_scan(None, z, z, clouds, mode="affine")
    with pytest.raises(ValueError, match="bodies"):
        editing.register_scan(None, z, z, clouds[:1])
    with pytest.raises(ValueError, match=">= 0"):
        editing.register_scan(None, z, z, clouds, align_every=-1)


def test_reference_transform_and_closed_form():
    rs = np.random.RandomState(1)
    p = rs.randn(500, 3)
    At, tt = 1.3 * A.rotation(A.AXIS, 40.0), np.array([0.3, -0.2, 0.5])
    got = A.transform_f32(A.pack(At, tt), p.astype(np.float32))
    ref = A.apply(A.pack(At, tt)[:9].reshape(3, 3), A.pack(At, tt)[9:], p.astype(np.float32).astype(np.float64))
    assert np.abs(got - ref).max() <= 4 * 2.0 ** -24 * np.abs(ref).max()   # three fused steps, each half an ulp of a partial sum
    q = A.apply(At, tt, p)
    w = rs.uniform(0.5, 1.5, 500) / 500
    mom, _ = A.moments(p, q, w)
    for mode in ("similarity", "rigid", "translation"):
        Au, tu, c, Rm = A.umeyama(mom, mode)
        assert np.allclose(Rm.T @ Rm, np.eye(3), atol=1e-12) and np.linalg.det(Rm) > 0
        if mode == "similarity":
            assert np.allclose(Au, At, atol=1e-12) and np.allclose(tu, tt, atol=1e-12) and A.residual(p, q, w, Au, tu) < 1e-24
    mirror = p * np.array([-1.0, 1.0, 1.0])                                # a reflected cloud: the answer is a rotation all the same
    _, _, _, Rm = A.umeyama(A.moments(p, mirror, w)[0], "rigid")
    assert np.linalg.det(Rm) > 0.999999
    assert np.array_equal(A.umeyama(np.zeros(20), "similarity")[0], np.eye(3))


def test_reference_icp_reproduces_the_cpu_study():
    """template6890, bodies of scan_ref.model_points(v, 4, seed=3), scan = the body's own vertices with 1 % jitter, 20 011 points,
    moved by the inverse of the four similarities.  Moment start, 40 iterations, both directions and scan -> model only: the final
    RMS scan -> model distance stays within 1.002 of the RMS at the true pose (and cannot fall far below it: seven parameters
    against 20 011 points).  Identity start, scan -> model only: three of the four cases end far from the truth."""
    v = np.asarray(load_hierarchy(os.path.join(GOLD, "template6890.npz")).verts, dtype=np.float64)
    n = v.shape[0]
    x = R.model_points(v, 4, seed=3)
    collapsed = 0
    for k, case in enumerate(A.SIMILARITY_CASES):
        xb = x[k, :n].astype(np.float64)
        s, pts, (At, _) = A.moved_scan(xb, case, seed=100 + k)
        r_true = A.rms_scan_to_model(pts, xb)
        for w in (0.0, 1.0):
            Af, tf = A.icp(xb, s, "similarity", 40, "moments", w)
            r = A.rms_scan_to_model(A.apply(Af, tf, s.astype(np.float64)), xb)
            print("reference ICP %s w=%g: RMS %.5f, at the true pose %.5f, ratio %.4f" % (case, w, r, r_true, r / r_true))
            assert 0.95 * r_true <= r <= 1.002 * r_true, (case, w, r, r_true)
        Af, _ = A.icp(xb, s, "similarity", 40, "identity", 0.0)
        U, S, Vt = np.linalg.svd(Af @ np.linalg.inv(At))
        angle = np.degrees(np.arccos(np.clip((np.trace(U @ Vt) - 1) / 2, -1, 1)))
        print("   identity start, scan -> model only: %.1f degrees and %.1f %% of scale from the truth" % (angle, 100 * abs(S.mean() - 1)))
        collapsed += angle > 10 and abs(S.mean() - 1) > 0.25
    assert collapsed == 3
