"""Point-to-surface alignment without a GPU: why the feature exists (float64 vertex ICP is biased on a scan that samples the
surface, float64 surface ICP is not - tests/align_surface_ref.py), the new symbol and its argument validation before the device
is touched, the reference's kept rule, and the Python-side argument errors that need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, ops, scan
from tests import align_ref as A
from tests import align_surface_ref as AS

GOLD = os.path.join(os.path.dirname(__file__), "golden")
U53 = 2.0 ** -53


def test_vertex_icp_is_biased_on_surface_samples_and_surface_icp_is_not():
    """small_ae.npz (170 vertices, 336 faces), 2000 noise-free samples of each body's own surface moved by the inverse of the first
    two SIMILARITY_CASES, 40 iterations, similarity, scan -> model only, moment start.  Measured (python -m tests.align_surface_ref):
    vertex ICP ends 2.9 % and 3.5 % too large with pose errors 1.7e-2 and 2.9e-2 of the extent; surface ICP ends 6e-5 and 1.8e-4 off
    in scale with pose errors 4.7e-4 and 3.1e-3 (ratios 0.027 and 0.11)."""
    x, faces, n, moved = AS.study_inputs()
    for k, case in enumerate(A.SIMILARITY_CASES[:2]):
        r = AS.study_case(x[k, :n].astype(np.float64), faces, moved[k])
        rel_v, rel_s = abs(r["c_vertex"] / r["c_true"] - 1), abs(r["c_surface"] / r["c_true"] - 1)
        L = r["log"]
        # Fixed partners, least squares over the pose, re-matching to the closest surface point: nothing rises in exact arithmetic.
        # In float64 a distance of coordinates of size <= extent carries a few roundings (16 x 2^-53 x extent at most), which moves
        # a squared distance by 2 sqrt(d2) times that and the mean by 32 x 2^-53 x extent x sqrt(L) (Cauchy-Schwarz), on either side of
        # the comparison; the 2000-term mean itself adds 2000 x 2^-53 x L.
        tol = 2 * (32 * U53 * r["extent"] * np.sqrt(L[:-1])) + 2 * 2000 * U53 * L[:-1]
        rise = L[1:] - L[:-1]
        print("%s: scale error vertex %.3g, surface %.3g; pose error vertex %.3g, surface %.3g (ratio %.3g); largest rise / tolerance %.3g"
              % (case, rel_v, rel_s, r["e_vertex"], r["e_surface"], r["e_surface"] / r["e_vertex"], float((rise / tol).max())))
        assert rel_v >= 1e-2, (case, rel_v)
        assert rel_s <= 1e-3, (case, rel_s)
        assert r["e_surface"] <= 0.25 * r["e_vertex"], (case, r["e_surface"], r["e_vertex"])
        assert (rise <= tol).all(), (case, float((rise / tol).max()))
        assert L[-1] < L[0]


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "sh_kernels.h")).read()
    lib = _lib.load()
    name = "sh_align_moments_surface"
    assert name in _lib.SIGNATURES and name + "(" in header and hasattr(lib, name)
    assert callable(ops.align_moments_surface)


def test_argument_validation_without_a_device():
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)                      # p: never dereferenced - validation comes first
    inf = float("inf")

    def call(s=p, M=1, rows=1, n=1, faces=p, nF=1, face=p, uv=p, d2=p, idx_ms=null, d2_ms=null, tau2=inf, w=0.0, B=1, part=p, nbytes=1 << 20,
             s_sb=3, x_sb=3):
        return lib.sh_align_moments_surface(s, s_sb, M, null, p, x_sb, rows, n, null, 0, faces, nF, face, uv, d2, idx_ms, d2_ms, tau2, w, B, part,
                                            nbytes, null)

    for bad in (dict(s=null), dict(faces=null), dict(face=null), dict(uv=null), dict(d2=null), dict(part=null)):
        assert call(**bad) == -1 and b"sh_align_moments_surface: null pointer" in lib.sh_last_error(), bad
    for bad in (dict(B=-1), dict(M=-1), dict(nF=-1), dict(n=2), dict(w=0.5), dict(tau2=float("nan")), dict(w=float("nan")), dict(s_sb=2),
                dict(x_sb=2)):
        assert call(**bad) == -1, bad
    assert call(nbytes=8) != 0 and b"partials too small" in lib.sh_last_error()        # one range of 19 doubles is needed
    assert call(B=0, nbytes=0) == 0                                                     # nothing launched
    assert call(B=0, faces=null, nF=0) == 0                                             # an empty table needs no pointer


def test_reference_kept_rule_and_foot_points():
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [9, 9, 9]], np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 4], [1, 2, 3]])                     # face 1 names row 4 = n: not a vertex
    s = np.array([[0.2, 0.2, 0.5], [0.1, 0.1, 0.1], [0.5, 0.5, 0.5], [0.3, 0.3, 0.3], [7, 7, 7], [1, 1, 1]], np.float32)
    face = np.array([0, 1, 2, -1, 3, 0])
    uv = np.array([[0.25, 0.5], [0.1, 0.1], [0.5, 0.25], [0, 0], [0, 0], [1, 0]], np.float32)
    d2 = np.array([0.25, 0.0, 0.1, 0.0, 0.0, 0.5], np.float32)
    p, q, w = AS.pairs_surface(s, x, 4, 5, None, faces, face, uv, d2, None, None, 0.5, 0.0)   # m = 5: row 5 is padding; tau2 strict
    assert np.array_equal(p, s[[0, 2]].astype(np.float64)) and np.array_equal(w, [0.2, 0.2])
    assert np.array_equal(q, np.array([[0.25, 0.5, 0.0], [0.25, 0.5, 0.25]]))
    p, q, w = AS.pairs_surface(s, x, 4, 6, None, faces, face, uv, d2, None, None, 0.5, 0.0)
    assert len(w) == 2                                                       # d2 == tau2 is not kept
    p, q, w = AS.pairs_surface(s, x, 4, 6, None, faces, face, uv, d2, None, None, np.inf, 0.0)
    assert len(w) == 3 and np.array_equal(q[2], [1.0, 0.0, 0.0])


def test_argument_errors_that_need_no_device():
    z = torch.zeros((2, 17, 8))
    clouds = [np.zeros((4, 3), np.float32)] * 2
    with pytest.raises(ValueError, match="faces"):
        editing.register_scan(None, z, z, clouds, align_on="surface")
    with pytest.raises(ValueError, match="align_on"):
        editing.register_scan(None, z, z, clouds, align_on="faces")
    sb = scan.ScanBatch(clouds, "cpu")
    with pytest.raises(ValueError, match="surface"):
        scan.pose_update(scan.Pose.identity(2, "cpu"), sb, sb, dict(idx_sm=None, d2_sm=None), surface=True)
