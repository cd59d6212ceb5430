"""The robust terms without a GPU: the reference's weight is the derivative of its penalty and both are continuous at the switch,
scan.robust_weights is the reference's weight, every argument error of the Python layer and of the C ABI, and the outlier
experiment in float64 - the condition on the inputs that tests/test_robust.py's GPU experiment relies on."""
import ctypes

import numpy as np
import pytest
import torch

from semantichuman_amd import _lib, editing, scan
from tests import robust_ref as RR

U24 = 2.0 ** -24


@pytest.mark.parametrize("form", RR.FORMS)
def test_weight_is_the_derivative_of_the_penalty(form):
    scale2 = 0.37
    u = np.concatenate([np.geomspace(1e-4, 1e3, 400) * scale2, [0.5 * scale2, 0.999 * scale2, 1.001 * scale2, 2.0 * scale2]])
    h = 1e-6 * u
    num = (RR.rho(u + h, form, scale2) - RR.rho(u - h, form, scale2)) / (2 * h)
    w = RR.weight(u, form, scale2)
    # central differences in float64: truncation h^2 rho''' / 6 ~ 1e-12 relative, rounding 2^-53 rho / h ~ 1e-10 relative.
    # Huber's second derivative jumps at u = scale2, so a stencil that straddles the switch is first order only (h rho'' / 4
    # ~ 1e-7): the grid's point at the switch is held to that, every other point to 1e-8.
    astride = (u - h <= scale2) & (u + h >= scale2) if form == "huber" else np.zeros(u.shape, bool)
    assert astride.sum() == (form == "huber")
    assert np.abs(num - w)[~astride].max() <= 1e-8 * w.max(), np.abs(num - w)[~astride].max()
    assert (np.abs(num - w)[astride] <= 0.5 * 1e-6).all()
    assert (w > 0).all() and (w <= 1.0).all() and (np.diff(w[:400]) <= 0).all()          # a weight, and it only falls
    small = 1e-9 * scale2
    assert abs(RR.rho(small, form, scale2) / small - 1) <= 2e-9 and abs(RR.weight(small, form, scale2) - 1) <= 4e-9
    assert RR.rho(0.0, form, scale2) == 0.0 and RR.weight(0.0, form, scale2) == 1.0


@pytest.mark.parametrize("form", RR.FORMS)
def test_both_forms_are_continuous_at_the_scale(form):
    scale2 = 0.37
    below, above = np.nextafter(scale2, 0.0), np.nextafter(scale2, 1.0)
    for f in (RR.rho, RR.weight):
        a, b, c = f(below, form, scale2), f(scale2, form, scale2), f(above, form, scale2)
        assert abs(a - b) <= 4e-16 and abs(c - b) <= 4e-16, (f.__name__, a, b, c)
    at = {"huber": (scale2, 1.0), "geman-mcclure": (scale2 / 2, 0.25)}[form]
    assert abs(RR.rho(scale2, form, scale2) - at[0]) <= 1e-16 and RR.weight(scale2, form, scale2) == at[1]


@pytest.mark.parametrize("trunc", [None, 0.9])
@pytest.mark.parametrize("form", RR.FORMS)
def test_robust_weights_is_the_reference_weight(form, trunc):
    sigma = 0.31
    scale2 = float(np.float32(sigma * sigma))
    rs = np.random.RandomState(5)
    d2 = np.concatenate([rs.rand(500) * 4 * scale2, [0.0, scale2, np.nextafter(np.float32(scale2), np.float32(9)), 1e-30, 1e6, np.inf]]).astype(np.float32)
    d2[5] = np.float32(scale2)
    w = scan.robust_weights(torch.from_numpy(d2), form, sigma, trunc=trunc)
    assert w.dtype == torch.float32 and tuple(w.shape) == d2.shape
    tau2 = np.inf if trunc is None else float(np.float32(trunc ** 2))
    ref = RR.pair_weights(d2, form, scale2, tau2)
    # fp32 against float64 of the same fp32 inputs: RR.W_ULPS roundings of 2^-24 at most (test_robust.py derives the count)
    assert np.abs(w.numpy() - ref).max() <= RR.W_ULPS * U24, np.abs(w.numpy() - ref).max()
    assert w[-1] == 0.0 and w[500] == 1.0                                                # +inf is truncated, d2 == 0 has weight 1
    if form == "huber":
        assert w[501] == 1.0 and w[5] == 1.0 and w[502] < 1.0                            # the switch: u == scale2 is inside
    if trunc is not None:
        assert (w.numpy()[d2 >= np.float32(tau2)] == 0).all() and (d2 >= np.float32(tau2)).any()
    plain = scan.robust_weights(torch.from_numpy(d2), None, None, trunc=trunc)
    assert np.array_equal(plain.numpy(), (d2 < np.float32(tau2)).astype(np.float32))


BAD = [dict(robust="cauchy", robust_scale=0.1), dict(robust=1, robust_scale=0.1), dict(robust_scale=0.1), dict(robust="huber"),
       dict(robust="huber", robust_scale=0.0), dict(robust="geman-mcclure", robust_scale=-1.0), dict(robust="huber", robust_scale=float("nan")),
       dict(robust="huber", robust_scale=float("inf")), dict(robust="geman-mcclure", robust_scale=1e-30), dict(robust="huber", robust_scale="wide")]


@pytest.mark.parametrize("bad", BAD, ids=[",".join("%s=%r" % kv for kv in b.items()) for b in BAD])
def test_argument_errors(bad):
    """An unknown name, a scale without a name, a name without a scale, a scale that is not positive and finite (1e-30: its
    square is not positive in fp32) - from every public function, before any device is asked for."""
    with pytest.raises(ValueError, match="robust"):
        scan.robust_weights(torch.zeros(3), bad.get("robust"), bad.get("robust_scale"))
    with pytest.raises(ValueError, match="robust"):
        scan._robust_arg("chamfer", bad.get("robust"), bad.get("robust_scale"))
    with pytest.raises(ValueError, match="pose_update: robust"):
        scan.pose_update(None, None, None, {}, **bad)
    z = torch.zeros((2, 4))
    clouds = scan.ScanBatch([np.zeros((3, 3), np.float32)] * 2, "cpu")
    with pytest.raises(ValueError, match="fit_scan: robust"):
        editing.fit_scan(None, z, None, clouds, **bad)
    with pytest.raises(ValueError, match="register_scan: robust"):
        editing.register_scan(None, z, None, clouds, **bad)


def test_match_plan_checks_the_robust_arguments_next_to_trunc():
    """chamfer and align resolve the two arguments in _MatchPlan; the plan needs no device for that."""
    sb = scan.ScanBatch([np.zeros((3, 3), np.float32)], "cpu")
    x = torch.zeros((1, 5, 3))
    pair = (sb, 1, 5, 4)

    def plan(**kw):
        return scan._MatchPlan("align", x, pair, None, 0.5, 1.0, None, None, None, "vertices", **kw)

    for bad in BAD:
        with pytest.raises(ValueError, match="align: robust"):
            plan(**bad)
    assert plan().robust is None
    form, scale2 = plan(robust="huber", robust_scale=0.5).robust
    assert (form, scale2) == (2, 0.25) and plan(robust="geman-mcclure", robust_scale=2).robust == (1, 4.0)


ROBUST_ENTRIES = ["sh_chamfer_fwd_robust", "sh_chamfer_bwd_robust", "sh_chamfer_surface_bwd_robust", "sh_align_moments_robust",
                  "sh_align_moments_surface_robust", "sh_align_plane_moments_robust", "sh_align_plane_moments_surface_robust"]


@pytest.mark.parametrize("entry", ROBUST_ENTRIES)
def test_the_c_abi_rejects_bad_robust_arguments_without_a_gpu(entry):
    lib = _lib.load()
    fn = getattr(lib, entry)
    types = _lib.SIGNATURES[entry][1]
    assert types[-2:] == [ctypes.c_int, ctypes.c_float] and types[:-2] == _lib.SIGNATURES[entry[:-7]][1]   # the namesake's, plus two
    zeros = [ctypes.c_void_p(0) if t is ctypes.c_void_p else 0 for t in types[:-2]]
    for robust, scale2, text in ((3, 1.0, b"unknown robust form"), (-1, 1.0, b"unknown robust form"), (1, 0.0, b"scale2"), (2, -1.0, b"scale2"),
                                 (1, float("nan"), b"scale2"), (2, float("inf"), b"scale2")):
        rc = fn(*zeros, robust, scale2)
        assert rc == -1 and text in lib.sh_last_error() and entry.encode() in lib.sh_last_error(), (robust, scale2, lib.sh_last_error())
    assert fn(*zeros, 0, float("nan")) == -1 and b"null pointer" in lib.sh_last_error()     # robust 0 never reads scale2: the namesake's checks


def test_outlier_experiment_in_float64():
    """15 % one-sided outliers, no trunc: each robust form's final pose error is at most a third of least squares', in rotation,
    translation and scale.  A condition on the inputs (robust_ref.OUTLIER_*), verified here.  Measured (degrees, model units,
    relative scale): plain (1.861, 0.0760, 0.1283), geman-mcclure (0.337, 0.00216, 0.00073), huber (0.536, 0.00492, 0.00811)."""
    err = RR.outlier_reference()
    for form in (None,) + RR.FORMS:
        print("outlier experiment, float64, %s: angle %.4g deg, translation %.4g, scale %.4g" % ((form,) + err[form]))
    assert min(err[None]) > 0
    for form in RR.FORMS:
        for k in range(3):
            assert err[form][k] <= err[None][k] / 3.0, (form, k, err[form][k], err[None][k])
