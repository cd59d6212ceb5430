"""The point-to-plane pose step without a GPU: why the feature exists (on surface samples the float64 point-to-plane loop is at the
scan's rounding floor after 10 iterations where the point-to-point loop is still above 1e-3 - tests/align_plane_ref.py), the
reference's Jacobian, solve and singular rules, the new symbols and their argument validation before the device is touched, and
the Python-side argument errors that need no device."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, ops, scan
from tests import align_ref as A
from tests import align_plane_ref as AP
from tests import align_surface_ref as AS

GOLD = os.path.join(os.path.dirname(__file__), "golden")
U53 = 2.0 ** -53
NAMES = ("sh_align_plane_partials_bytes", "sh_align_plane_moments", "sh_align_plane_moments_surface", "sh_align_plane_solve")


# ------------------------------------------------------------------------------------------------ the study
@functools.lru_cache(maxsize=None)
def study():
    """Both float64 loops on the four study cases, once: [(plane errors after 1 .. 10 updates, its log, solved, point-to-point error
    after 10 updates)]."""
    x, faces, n, moved = AS.study_inputs()
    out = []
    for k in range(len(A.SIMILARITY_CASES)):
        xb = x[k, :n].astype(np.float64)
        e, log, solved = AP.plane_errors(xb, faces, moved[k], iters=10)
        out.append((e, log, solved, float(AP.point_errors(xb, faces, moved[k], at=(10,))[0])))
    return out


@pytest.mark.parametrize("k", range(4))
def test_plane_loop_converges_where_the_point_loop_has_not(k):
    """Measured (python -m tests.align_plane_ref), pose error / extent: point-to-point after 10 iterations 5.4e-3, 1.9e-2, 1.5e-2,
    3.2e-2; point-to-plane after 10 iterations 2.0e-8, 3.9e-8, 3.1e-8, 4.1e-8 (the fp32 rounding of the scan), first below 1e-3 at
    iteration 3, 3, 4, 5; largest rise of the logged surface Chamfer value 1.3e-26."""
    e, log, solved, e_point = study()[k]
    rise = float((log[1:] - log[:-1]).max())
    print("%s: plane %s; first below 1e-3 at %s; point-to-point after 10: %.3g; largest rise %.3g"
          % (A.SIMILARITY_CASES[k], " ".join("%.2g" % v for v in e), AP.first_below(e), e_point, rise))
    assert solved.all()
    assert e[5] < 1e-3, e[5]                                               # by iteration 6
    assert e[9] < 1e-6, e[9]                                               # by iteration 10
    assert e_point > 1e-3, e_point
    assert rise < 1e-12, rise
    assert log[-1] < log[0]


# ------------------------------------------------------------------------------------------------ Jacobian, solve, singular rules
def random_pairs(seed, k=400, noise=0.02):
    rs = np.random.RandomState(seed)
    q = rs.randn(k, 3)
    nrm = rs.randn(k, 3)
    nrm /= np.sqrt((nrm * nrm).sum(1, keepdims=True))
    p = q + noise * rs.randn(k, 3)
    w = rs.rand(k) / k
    return p, q, nrm, w


def moved(p, delta):
    """The exact increment of a step delta: c R p + t with c = exp(sigma), R = exp([omega]x)."""
    return np.exp(delta[6]) * p @ AP.rodrigues(delta[3:6]).T + delta[:3]


def test_jacobian_against_central_differences_of_the_exact_increment():
    p, q, nrm, _ = random_pairs(0)
    J = AP.jacobian(p, nrm)
    h = 1e-6
    worst = 0.0
    for i in range(7):
        d = np.zeros(7)
        d[i] = h
        num = (AP.residual(moved(p, d), q, nrm) - AP.residual(moved(p, -d), q, nrm)) / (2 * h)
        # central differences: truncation h^2 |f'''| / 6 <= 1e-12 |p| and rounding 4 x 2^-53 |p| / h = 4.5e-10 |p|
        tol = 1e-9 * np.maximum(1.0, np.sqrt((p * p).sum(1)))
        worst = max(worst, float((np.abs(num - J[:, i]) / tol).max()))
        assert (np.abs(num - J[:, i]) <= tol).all(), i
    print("Jacobian against central differences: largest error / tolerance %.3g" % worst)


@pytest.mark.parametrize("mode", ["translation", "rigid", "similarity"])
def test_plane_solve_against_lstsq_on_the_raw_pairs(mode):
    k = AP.MODE_K[mode]
    for seed in range(4):
        p, q, nrm, w = random_pairs(10 + seed)
        sys, _ = AP.plane_system(p, q, nrm, w)
        assert sys.shape == (38,) and sys[37] == len(w)
        cR, t, c, Rm, solved, delta = AP.plane_solve(sys, mode)
        assert solved == 1 and (delta[k:] == 0).all()
        J, r = AP.jacobian(p, nrm)[:, :k], AP.residual(p, q, nrm)
        sw = np.sqrt(w)
        ref = np.linalg.lstsq(J * sw[:, None], -r * sw, rcond=None)[0]
        # the normal equations square the condition number of J: cond(H_scaled) 2^-53 relative, times a small constant for the
        # 7 x 7 factorisation and the 400-term sums (64); compared in the scaled unknowns, where the columns have unit size
        sd = AP.scaled_block(sys, mode)[2]
        tol = 64 * AP.condition(sys, mode) * U53 * np.abs(ref * sd).max()
        err = np.abs((delta[:k] - ref) * sd).max()
        print("plane_solve %s seed %d: cond %.3g, error %.3g (tolerance %.3g)" % (mode, seed, AP.condition(sys, mode), err, tol))
        assert err <= tol, (mode, seed, err, tol)
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-14) and np.linalg.det(Rm) > 0
        assert c == np.exp(delta[6]) and np.array_equal(t, delta[:3])
        if mode == "translation":
            assert np.array_equal(cR, np.eye(3))
        if mode != "similarity":
            assert c == 1.0
        # the step lowers the linearised residual it minimises
        assert (w * (r + J @ delta[:k]) ** 2).sum() <= (w * r * r).sum()


def test_rodrigues_series_and_closed_form_agree():
    for th in (0.0, 1e-9, 9e-5, 1.1e-4, 0.3, 3.0):
        om = th * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
        assert np.abs(AP.rodrigues(om) - A.rotation([1.0, 2.0, 3.0], np.rad2deg(th))).max() <= 4e-16, th


def is_identity(res):
    cR, t, c, Rm, solved, delta = res
    return solved == 0 and np.array_equal(cR, np.eye(3)) and not t.any() and c == 1.0 and not delta.any()


@pytest.mark.parametrize("mode", ["translation", "rigid", "similarity"])
def test_singular_systems_give_the_identity(mode):
    p, q, nrm, w = random_pairs(3)
    assert is_identity(AP.plane_solve(AP.plane_system(p[:0], q[:0], nrm[:0], w[:0])[0], mode))                  # no pairs
    for direction in ([0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [1.0, 2.0, 3.0] / np.sqrt(14.0)):                     # all normals parallel
        par = np.tile(np.asarray(direction), (len(w), 1))
        assert is_identity(AP.plane_solve(AP.plane_system(p, q, par, w)[0], mode)), direction
    assert is_identity(AP.plane_solve(AP.plane_system(p[:2], q[:2], nrm[:2], w[:2])[0], mode))                  # two pairs
    zero = AP.plane_system(p, q, np.zeros_like(nrm), w)[0]                                                      # zero normals: kept, no terms
    assert zero[0] > 0 and zero[37] == len(w) and not zero[1:37].any() and is_identity(AP.plane_solve(zero, mode))
    assert AP.plane_solve(AP.plane_system(p, q, nrm, w)[0], mode)[4] == 1


def test_reference_pairs_follow_the_kept_rule_of_the_point_step():
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [9, 9, 9]], np.float32)
    faces = np.array([[0, 1, 2], [0, 1, 4], [1, 2, 3]])
    s = np.array([[0.2, 0.2, 0.5], [0.1, 0.1, 0.1], [0.5, 0.5, 0.5], [0.3, 0.3, 0.3], [7, 7, 7], [1, 1, 1]], np.float32)
    face = np.array([0, 1, 2, -1, 3, 0])
    uv = np.array([[0.25, 0.5], [0.1, 0.1], [0.5, 0.25], [0, 0], [0, 0], [1, 0]], np.float32)
    d2 = np.array([0.25, 0.0, 0.1, 0.0, 0.0, 0.5], np.float32)
    p, q, nrm, w = AP.pairs_plane(s, x, 4, 5, None, None, None, None, None, 0.5, 0.0, surface=(faces, face, uv, d2))
    p2, q2, w2 = AS.pairs_surface(s, x, 4, 5, None, faces, face, uv, d2, None, None, 0.5, 0.0)
    assert np.array_equal(p, p2) and np.array_equal(q, q2) and np.array_equal(w, w2)
    assert np.array_equal(nrm[0], [0.0, 0.0, 1.0]) and np.allclose(nrm[1], np.ones(3) / np.sqrt(3.0), atol=1e-15)
    tn = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], np.float32)
    idx_sm, d2_sm = np.array([1, 3, -1, 2, 0, 0]), np.array([0.1, 0.1, 0.1, 0.6, 0.1, 0.1], np.float32)
    idx_ms, d2_ms = np.array([0, 5, 2, 1]), np.array([0.1, 0.1, 0.7, 0.1], np.float32)
    p, q, nrm, w = AP.pairs_plane(s, x, 4, 5, [True, True, True, False], idx_sm, d2_sm, idx_ms, d2_ms, 0.5, 0.5, tn=tn)
    p2, q2, w2 = A.pairs(s, x, 4, 5, [True, True, True, False], idx_sm, d2_sm, idx_ms, d2_ms, 0.5, 0.5)
    assert np.array_equal(p, p2) and np.array_equal(q, q2) and np.array_equal(w, w2)
    assert np.array_equal(nrm, tn[[1, 3, 0, 0]].astype(np.float64))       # scan -> model j = 0, 1, 4; model -> scan i = 0


# ------------------------------------------------------------------------------------------------ symbols and validation
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(GOLD), "..", "include", "sh_kernels.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name + "(" in header and hasattr(lib, name), name
    assert "#define SH_ALIGN_PLANE_PARTIAL %d" % ops.ALIGN_PLANE_PARTIAL in header
    assert "#define SH_ALIGN_PLANE_SYSTEM %d" % ops.ALIGN_PLANE_SYSTEM in header and AP.NSYS == ops.ALIGN_PLANE_SYSTEM
    assert lib.sh_align_plane_partials_bytes(3, 2049, 170, 0.0) == 3 * 2 * 38 * 8
    assert lib.sh_align_plane_partials_bytes(3, 2049, 170, 1.0) == 3 * 3 * 38 * 8
    assert lib.sh_align_plane_partials_bytes(0, 5, 5, 1.0) == 0


def test_argument_validation_without_a_device():
    lib = _lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(64)                      # p: never dereferenced - validation comes first
    inf = float("inf")

    def surface(s=p, M=1, rows=1, n=1, tn=null, faces=p, nF=1, face=p, uv=p, d2=p, idx_ms=null, d2_ms=null, tau2=inf, w=0.0, B=1, part=p,
                nbytes=1 << 20, s_sb=3, x_sb=3):
        return lib.sh_align_plane_moments_surface(s, s_sb, M, null, p, x_sb, rows, n, null, 0, tn, faces, nF, face, uv, d2, idx_ms, d2_ms, tau2, w, B,
                                                  part, nbytes, null)

    def vertex(s=p, M=1, rows=1, n=1, tn=p, idx_sm=p, d2_sm=p, idx_ms=null, d2_ms=null, tau2=inf, w=0.0, B=1, part=p, nbytes=1 << 20, s_sb=3,
               x_sb=3):
        return lib.sh_align_plane_moments(s, s_sb, M, null, p, x_sb, rows, n, null, 0, tn, idx_sm, d2_sm, idx_ms, d2_ms, tau2, w, B, part, nbytes,
                                          null)

    for bad in (dict(s=null), dict(faces=null), dict(face=null), dict(uv=null), dict(d2=null), dict(part=null)):
        assert surface(**bad) == -1 and b"sh_align_plane_moments_surface: null pointer" in lib.sh_last_error(), bad
    for bad in (dict(s=null), dict(idx_sm=null), dict(d2_sm=null), dict(part=null), dict(tn=null)):
        assert vertex(**bad) == -1 and b"sh_align_plane_moments: null pointer" in lib.sh_last_error(), bad
    assert surface(w=0.5, idx_ms=p, d2_ms=p) == -1 and b"null pointer (tn" in lib.sh_last_error()   # model -> scan pairs read tn
    for call in (surface, vertex):
        for bad in (dict(B=-1), dict(M=-1), dict(n=2), dict(w=0.5), dict(tau2=float("nan")), dict(w=float("nan")), dict(s_sb=2), dict(x_sb=2)):
            assert call(**bad) == -1, bad
        assert call(nbytes=37 * 8) != 0 and b"partials too small" in lib.sh_last_error()           # one range of 38 doubles is needed
        assert call(B=0, nbytes=0) == 0                                                             # nothing launched
    assert surface(nF=-1) == -1

    def solve(part=p, M=1, n=1, w=0.0, mode=2, B=1, pin=p, sin=p, pout=p, sout=p, sys=null, solved=p):
        return lib.sh_align_plane_solve(part, M, n, null, w, mode, B, pin, sin, pout, sout, sys, solved, null)

    for bad in (dict(part=null), dict(pout=null, sys=null), dict(pin=null), dict(sin=null), dict(sout=null), dict(solved=null), dict(B=-1), dict(M=-1),
                dict(n=-1), dict(w=-1.0), dict(w=float("nan")), dict(mode=3)):
        assert solve(**bad) == -1 and b"sh_align_plane_solve" in lib.sh_last_error(), bad
    assert solve(B=0) == 0


def test_argument_errors_that_need_no_device():
    z = torch.zeros((2, 17, 8))
    clouds = [np.zeros((4, 3), np.float32)] * 2
    with pytest.raises(ValueError, match="align_step"):
        editing.register_scan(None, z, z, clouds, align_step="planes")
    with pytest.raises(ValueError, match="triangles"):
        editing.register_scan(None, z, z, clouds, align_step="plane")
    sb = scan.ScanBatch(clouds, "cpu")
    with pytest.raises(ValueError, match="step"):
        scan.pose_update(scan.Pose.identity(2, "cpu"), sb, sb, dict(idx_sm=None, d2_sm=None), step="planar")
    with pytest.raises(ValueError, match="normals"):
        scan.pose_update(scan.Pose.identity(2, "cpu"), sb, sb, dict(idx_sm=None, d2_sm=None, w_ms=0.0, n=4), step="plane")
    assert scan.Pose.identity(2, "cpu").solved is None
