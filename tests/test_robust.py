"""The robust terms on the GPU (include/sh_kernels.h, "Robust terms"): value and gradient of scan.chamfer(..., robust=) against
tests/robust_ref.py on the kernels' own recorded matches, the shapes at which the walks change path, the bitwise properties, the
pose steps against the reference's weighted solve, and the outlier experiment of tests/test_robust_host.py through scan.align.

Tolerances.  The plain value and gradient are held to 1e-6 and 1e-5 relative by tests/test_scan.py and to KERNEL_FACTOR *
F32_GRAD_REL by tests/test_surface.py.  The robust forms add fp32 roundings of 2^-24 relative each, counted from the header's
expressions:
    Geman-McClure   t = s / (s + u): the sum and the quotient, 2;  rho = u t: 3;  w = t t: 2 + 2 + 1 = 5
    Huber           a = 2 sqrt(s u): the product, half of it through the root, the root, 1.5; rho = a - s with s <= a / 2, so
                    rho >= a / 2 and the error of a doubles relative to rho: 3, plus the difference: 4;  w = sqrt(s / u): 1.5
so rho carries at most RHO_ULPS = 4 and w at most W_ULPS = 5 units of 2^-24.  Every term of the value is positive: the value's
relative bound grows by 4 x 2^-24.  A gradient element is a signed sum: its bound grows by 5 x 2^-24 times the sum of the
absolute values of its terms (`mag` of the reference).  A moment is the same kind of sum: 5 x 2^-24 x sum w |term| on top of
the fp64 summation bound of tests/test_align.py and tests/test_align_plane.py."""
import functools

import numpy as np
import pytest
import torch

from semantichuman_amd import ops, scan
from tests import align_plane_ref as AP
from tests import align_ref as A
from tests import robust_ref as RR
from tests import scan_ref as R
from tests import surface_ref as S
from tests.launch_record import launches
from tests.test_align_surface import mesh, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24, U53 = 2.0 ** -24, 2.0 ** -53
FORM_ID = {"geman-mcclure": 1, "huber": 2}
PLAIN = {"chamfer_fwd_kernel", "chamfer_bwd_kernel", "surface_bwd_kernel", "align_moments_kernel", "align_moments_surface_kernel",
         "align_plane_moments_kernel", "align_plane_moments_surface_kernel"}


@functools.lru_cache(maxsize=None)
def small(B=3, counts=(300, 257, 0), seed=3):
    """The 170-vertex model: B bodies with the dummy row, the faces, ragged clouds sampled with noise from a neighbour body's
    surface (one of count 0), a vertex mask."""
    v, faces = mesh("small_ae.npz")
    n = v.shape[0]
    x = R.model_points(v, B, seed=seed)
    extent = float((x[0, :n].max(0) - x[0, :n].min(0)).max())
    clouds = [S.sample_surface(x[(b + 1) % B, :n], faces, c, seed=90 + b, sigma=0.02 * extent) for b, c in enumerate(counts)]
    vmask = np.random.RandomState(7).rand(n) < 0.8
    return x, faces, n, clouds, vmask, extent


def sigma_for(d2):
    """The robust_scale whose fp32 square is exactly the fp32 value d2."""
    sigma = float(np.sqrt(np.float64(d2)))
    assert np.float32(sigma * sigma) == np.float32(d2)
    return sigma


def run_chamfer(x, clouds, n, faces, vmask, trunc, w, form, sigma, gL=None):
    sb = scan.ScanBatch(clouds, DEV)
    xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
    ft = None if faces is None else scan.FaceTable(faces, n, DEV)
    matches = {}
    kw = {} if form is None else dict(robust=form, robust_scale=sigma)
    L = scan.chamfer(xd, sb, vertex_mask=vmask, trunc=trunc, w_model_to_scan=w, faces=ft, matches=matches, **kw)
    gL = torch.ones(len(clouds), device=DEV) if gL is None else gL
    g, = torch.autograd.grad(L, xd, gL)
    return L.detach(), g, matches, sb


def check_against_reference(x, clouds, n, faces, vmask, trunc, w, form, sigma, L, g, m, gL):
    """Value and gradient of every body against robust_ref on the recorded matches; returns the weights' range seen."""
    tau2 = np.inf if trunc is None else float(np.float32(trunc ** 2))
    scale2 = float(np.float32(sigma * sigma))
    Lh, gn, gLn = L.cpu().numpy(), g.cpu().numpy(), gL.cpu().numpy().astype(np.float64)
    mh = {k: (t.cpu().numpy() if torch.is_tensor(t) else t) for k, t in m.items()}
    lo, hi = 1.0, 0.0
    for b, c in enumerate(clouds):
        mb = c.shape[0]
        d_sm = mh["d2_sm"][b] if faces is None else mh["d2_surface"][b]
        d_ms = None if w == 0 else mh["d2_ms"][b]
        ref = RR.chamfer_value(d_sm, mb, d_ms, n, vmask, tau2, w, form, scale2)
        assert abs(float(Lh[b]) - ref) <= (1e-6 + RR.RHO_ULPS * U24) * ref, (b, float(Lh[b]), ref)
        surface = None if faces is None else (faces, mh["face"][b], mh["uv"][b], mh["d2_surface"][b])
        g64, mag = RR.chamfer_grad(x[b], c, n, mb, vmask, tau2, w, form, scale2, None if w == 0 else mh["idx_ms"][b], d_ms,
                                   idx_sm=mh["idx_sm"][b], d2_sm=mh["d2_sm"][b], surface=surface)
        g64, mag = g64 * gLn[b], mag * abs(gLn[b])
        base = 1e-5 if faces is None else S.KERNEL_FACTOR * S.F32_GRAD_REL
        err, top = np.abs(gn[b] - g64).max(), np.abs(g64).max()
        print("robust %s b=%d m=%d: value %.9g vs %.9g, gradient error %.3g of %.3g" % (form, b, mb, float(Lh[b]), ref, err, top))
        assert err <= base * top + RR.W_ULPS * U24 * mag.max(), (b, err, top)
        assert not gn[b, n:].any() and (vmask is None or not gn[b, :n][~np.asarray(vmask)].any())
        if mb == 0:
            assert Lh[b] == 0.0 and not gn[b].any()
        else:
            wts = RR.pair_weights(d_sm[:mb], form, scale2, tau2)
            lo, hi = min(lo, wts[wts > 0].min() if (wts > 0).any() else lo), max(hi, wts.max())
    return lo, hi


# ------------------------------------------------------------------------------------------------ 1. value and gradient
@pytest.mark.parametrize("truncate", [False, True])
@pytest.mark.parametrize("w", [0.0, 0.5])
@pytest.mark.parametrize("surface", [False, True])
@pytest.mark.parametrize("form", RR.FORMS)
def test_value_and_gradient_against_the_reference(form, surface, w, truncate):
    """rows = n + 1 (the dummy row), a vertex mask, ragged counts with an empty cloud.  sigma and trunc as shares of the extent,
    (0.02, 0.06) for vertex partners and (0.01, 0.03) for foot points: on these clouds (float64 searches on the host) a fifth to
    a half of the points is truncated and the kept weights run from about 0.01 (Geman-McClure) or 0.33 (Huber) up to 0.57 .. 1."""
    x, faces, n, clouds, vmask, extent = small()
    sigma, trunc = (0.01 if surface else 0.02) * extent, ((0.03 if surface else 0.06) * extent if truncate else None)
    gL = torch.from_numpy(np.random.RandomState(2).randn(len(clouds)).astype(np.float32)).to(DEV)
    L, g, m, sb = run_chamfer(x, clouds, n, faces if surface else None, vmask, trunc, w, form, sigma, gL)
    assert x.shape[1] == n + 1
    lo, hi = check_against_reference(x, clouds, n, faces if surface else None, vmask, trunc, w, form, sigma, L, g, m, gL)
    assert lo < 0.5 < hi, (lo, hi)                                                       # the robust branch is exercised on both sides
    if truncate:
        d = (m["d2_surface"] if surface else m["d2_sm"])[0, :clouds[0].shape[0]].cpu().numpy()
        assert 0.02 <= (d >= np.float32(trunc ** 2)).mean() <= 0.98                      # and so is the truncation


# ------------------------------------------------------------------------------------------------ 2. shapes and special pairs
@pytest.mark.parametrize("M", [1, 255, 256, 257, 300, 2049, 4097])
@pytest.mark.parametrize("form", RR.FORMS)
def test_tile_and_range_edges(form, M):
    """M around the gradient's tiles of 256 and the pose step's ranges of 2048, B = 3 ragged with an empty cloud; a pair with
    d2 == 0 (a scan point on a vertex), one with d2 == scale2 exactly (sigma is taken from the distance the plain run records
    for a point put 1 % of the extent off a vertex, per partner kind) and pairs with d2 > tau2."""
    x, faces, n, _, vmask, extent = small()
    clouds = [S.sample_surface(x[(b + 1) % 3, :n], faces, c, seed=M + b, sigma=0.02 * extent) for b, c in enumerate((M, max(M - 3, 1), 0))]
    first = int(np.nonzero(vmask)[0][0])
    clouds[0][0] = x[0, first]                                                           # d2 == 0 against an active vertex
    clouds[1][0] = x[1, first] + np.float32(0.01 * extent) * np.array([1, 1, 1], np.float32)   # a kept pair a little off a vertex
    trunc = 0.05 * extent
    for surface in (False, True):
        _, _, m0, _ = run_chamfer(x, clouds, n, faces if surface else None, vmask, trunc, 0.5, None, None)
        pick = d_of(m0, surface)[1, 0]                                                   # what the plain run records for that pair
        assert d_of(m0, surface)[0, 0] == 0.0 and 0 < pick < np.float32(trunc ** 2), pick
        sigma = sigma_for(pick)
        L, g, m, sb = run_chamfer(x, clouds, n, faces if surface else None, vmask, trunc, 0.5, form, sigma)
        gL = torch.ones(3, device=DEV)
        check_against_reference(x, clouds, n, faces if surface else None, vmask, trunc, 0.5, form, sigma, L, g, m, gL)
        d = d_of(m, surface)
        assert d[0, 0] == 0.0 and d[1, 0] == np.float32(sigma * sigma)                   # the pair at the switch is there
        assert M < 255 or (d[0, :M] >= np.float32(trunc ** 2)).any()                     # and so are truncated ones
        # the pose steps on the same matches, every slot finite, the weight slot the sum of the weights
        part = pose_partials(sb, torch.from_numpy(x).to(DEV), n, vmask, m, trunc, 0.5, form, sigma, surface, plane=False)
        kept = part[:, :, 0].sum(1).cpu().numpy()
        scale2, tau2 = float(np.float32(sigma * sigma)), float(np.float32(trunc ** 2))
        for b, c in enumerate(clouds):
            mb = c.shape[0]
            ws = RR.pair_weights(d_of(m, surface)[b, :mb], form, scale2, tau2)
            act = np.asarray(vmask, bool)
            dm, im = m["d2_ms"][b, :n].cpu().numpy(), m["idx_ms"][b, :n].cpu().numpy()
            wm = RR.pair_weights(dm, form, scale2, tau2)[act & (im >= 0) & (im < mb)] if mb else np.zeros(0)
            ref = ws.sum() + wm.sum()
            assert abs(kept[b] - ref) <= RR.W_ULPS * U24 * ref + 1e-12, (b, kept[b], ref)


def d_of(m, surface):
    return (m["d2_surface"] if surface else m["d2_sm"]).cpu().numpy()


def pose_partials(sb, xd, n, vmask, m, trunc, w, form, sigma, surface, plane, tn=None):
    B = xd.shape[0]
    vm, vsb = ops._mask_arg(vmask, B, n, xd.device)
    tau2 = float("inf") if trunc is None else float(np.float32(trunc ** 2))
    rb = None if form is None else (FORM_ID[form], sigma * sigma)
    kw = {} if rb is None else dict(robust=rb)
    ims, dms = (m["idx_ms"], m["d2_ms"]) if w > 0 else (None, None)
    if surface:
        args = (m["faces"], m["face"], m["uv"], m["d2_surface"], ims, dms, tau2, w)
        if plane:
            return ops.align_plane_moments_surface(sb.points, sb.counts, xd, n, vm, vsb, tn if w > 0 else None, *args, **kw)
        return ops.align_moments_surface(sb.points, sb.counts, xd, n, vm, vsb, *args, **kw)
    args = (m["idx_sm"], m["d2_sm"], ims, dms, tau2, w)
    if plane:
        return ops.align_plane_moments(sb.points, sb.counts, xd, n, vm, vsb, tn, *args, **kw)
    return ops.align_moments(sb.points, sb.counts, xd, n, vm, vsb, *args, **kw)


@pytest.mark.parametrize("form", RR.FORMS)
def test_gated_run_with_points_without_a_partner(form):
    """Under a 5 degree gate on random scan normals most scan points have no compatible vertex: idx -1, d2 +inf.  They count as truncated - rho of
    tau2 in the value, nothing in the gradient - exactly as without the robust term."""
    x, faces, n, clouds, vmask, extent = small()
    clouds = [c for c in clouds[:2]]
    rs = np.random.RandomState(4)
    normals = [rs.randn(*c.shape) for c in clouds]
    sb = scan.ScanBatch(clouds, DEV, normals=normals)
    ft = scan.FaceTable(faces, n, DEV)
    xd = torch.from_numpy(x[:2]).to(DEV).requires_grad_(True)
    sigma, trunc = 0.02 * extent, 0.05 * extent
    matches = {}
    L = scan.chamfer(xd, sb, trunc=trunc, w_model_to_scan=0.5, normal_angle=5, normal_faces=ft, matches=matches, robust=form, robust_scale=sigma)
    g, = torch.autograd.grad(L.sum(), xd)
    none = (matches["idx_sm"] < 0) & (torch.arange(sb.points.shape[1], device=DEV)[None] < sb.counts[:, None])
    assert none.any() and torch.isinf(matches["d2_sm"][none]).all()
    assert torch.isfinite(L).all() and torch.isfinite(g).all()
    check_against_reference(x[:2], clouds, n, None, None, trunc, 0.5, form, sigma, L.detach(), g, matches, torch.ones(2, device=DEV))


# ------------------------------------------------------------------------------------------------ 3. bitwise properties
@pytest.mark.parametrize("surface", [False, True])
@pytest.mark.parametrize("form", RR.FORMS)
def test_same_bits_alone_in_a_batch_and_for_every_split(form, surface):
    x, faces, n, clouds, vmask, extent = small()
    f = faces if surface else None
    L, g, m, sb = run_chamfer(x, clouds, n, f, vmask, 0.05 * extent, 0.5, form, 0.02 * extent)
    L2, g2, _, _ = run_chamfer(x, clouds, n, f, vmask, 0.05 * extent, 0.5, form, 0.02 * extent)
    assert same(L, L2) and same(g, g2)
    for b in (0, 1):
        L1, g1, _, _ = run_chamfer(x[b:b + 1], [clouds[b]], n, f, vmask, 0.05 * extent, 0.5, form, 0.02 * extent)      # alone, M = its own count
        assert same(L1[0], L[b]) and same(g1[0], g[b]), b
    xd = torch.from_numpy(x).to(DEV)
    ft = None if f is None else scan.FaceTable(f, n, DEV)
    akw = dict(mode="similarity", iters=3, w_model_to_scan=1.0, trunc=0.2 * extent, vertex_mask=vmask, faces=ft, robust=form, robust_scale=0.02 * extent)
    for step in ("point", "plane"):
        skw = dict(akw, step=step, normal_faces=None if surface else scan.FaceTable(faces, n, DEV))
        p0, a0, l0 = scan.align(xd, sb, chunks=0, **skw)
        for chunks in (1, 3):
            p, a, l = scan.align(xd, sb, chunks=chunks, **skw)
            assert same(p.packed, p0.packed) and same(p.scale, p0.scale) and same(l, l0) and same(a.points, a0.points), (step, chunks)
        p1, a1, l1 = scan.align(xd[1:2], scan.ScanBatch([clouds[1]], DEV), chunks=0, **skw)
        assert same(p1.packed[0], p0.packed[1]) and same(l1[:, 0], l0[:, 1]) and same(a1.points[0], a0.points[1, :clouds[1].shape[0]]), step


def test_robust_none_is_the_call_without_the_argument_and_launches_the_plain_kernels():
    x, faces, n, clouds, vmask, extent = small()
    sb = scan.ScanBatch(clouds, DEV)
    ft = scan.FaceTable(faces, n, DEV)
    xd = torch.from_numpy(x).to(DEV)

    def chamfer(**kw):
        xg = xd.clone().requires_grad_(True)
        L = scan.chamfer(xg, sb, vertex_mask=vmask, trunc=0.05 * extent, w_model_to_scan=0.5, **kw)
        return [L.detach(), torch.autograd.grad(L.sum(), xg)[0]]

    def align(**kw):
        p, a, l = scan.align(xd, sb, iters=2, trunc=0.2 * extent, vertex_mask=vmask, **kw)
        return [p.packed, p.scale, a.points, l]

    seen = set()
    for fn, base in ((chamfer, {}), (chamfer, dict(faces=ft)), (align, {}), (align, dict(faces=ft)), (align, dict(step="plane", normal_faces=ft)),
                     (align, dict(step="plane", faces=ft))):
        ref, rec_ref = launches(lambda: fn(**base))
        off, rec_off = launches(lambda: fn(robust=None, robust_scale=None, **base))
        assert rec_off == rec_ref and all(same(u, v) for u, v in zip(ref, off)), base
        assert not any("robust" in k for k, _ in rec_off)
        seen |= {k for k, _ in rec_off}
        on, rec_on = launches(lambda: fn(robust="huber", robust_scale=0.02 * extent, **base))
        names_on = [k for k, _ in rec_on]
        assert [k.replace("_robust", "") for k in names_on] == [k for k, _ in rec_ref], base      # the same launches, the robust forms of these
        assert {k for k in names_on if "robust" in k} == {k.replace("_kernel", "_robust_kernel") for k, _ in rec_ref if k in PLAIN}
        assert not all(same(u, v) for u, v in zip(ref, on))
    assert PLAIN <= seen, PLAIN - seen


# ------------------------------------------------------------------------------------------------ 4. pose steps
@pytest.mark.parametrize("surface", [False, True])
@pytest.mark.parametrize("step", ["point", "plane"])
@pytest.mark.parametrize("form", RR.FORMS)
def test_pose_step_against_the_weighted_reference(form, step, surface):
    """The moments of one robust step against float64 sums over the same matches with the reference's weights, then
    scan.pose_update against the reference's solve (Umeyama / plane_solve) of the kernel's own joined system - the split and
    the tolerances of tests/test_align.py and tests/test_align_plane.py."""
    x, faces, n, clouds, vmask, extent = small()
    plane = step == "plane"
    sigma, trunc, w = 0.02 * extent, 0.05 * extent, 0.5
    L, g, m, sb = run_chamfer(x, clouds, n, faces, vmask, trunc, w, form, sigma)
    xd = torch.from_numpy(x).to(DEV)
    ft = scan.FaceTable(faces, n, DEV)
    tn = scan.vertex_normals(xd, ft)
    part = pose_partials(sb, xd, n, vmask, m, trunc, w, form, sigma, surface, plane, tn)
    B, M = len(clouds), sb.points.shape[1]
    scale2, tau2 = float(np.float32(sigma * sigma)), float(np.float32(trunc ** 2))
    mh = {k: (t.cpu().numpy() if torch.is_tensor(t) else t) for k, t in m.items()}
    start = scan.Pose.identity(B, DEV)
    out, sc = torch.full((B, 12), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV)
    if plane:
        joined = torch.full((B, 37), float("nan"), dtype=torch.float64, device=DEV)
        solved = ops.align_plane_solve(part, M, n, sb.counts, w, "similarity", start.packed, start.scale, out, sc, joined)
    else:
        joined = torch.full((B, 20), float("nan"), dtype=torch.float64, device=DEV)
        ops.align_solve(part, M, n, sb.counts, w, "similarity", start.packed, start.scale, out, sc, None, joined)
    joined, out = joined.cpu().numpy(), out.cpu().numpy().astype(np.float64)
    for b, c in enumerate(clouds):
        mb = c.shape[0]
        sf = (faces, mh["face"][b], mh["uv"][b], mh["d2_surface"][b]) if surface else None
        pr = RR.weighted_pairs(c, x[b], n, mb, vmask, mh["idx_ms"][b], mh["d2_ms"][b], tau2, w, form, scale2, idx_sm=mh["idx_sm"][b],
                               d2_sm=mh["d2_sm"][b], surface=sf, tn=tn[b].cpu().numpy(), plane=plane)
        K = len(pr[-1])
        ref, mag = AP.plane_system(*pr) if plane else A.moments(*pr)
        k = 37 if plane else 18
        # the fp64 summation bound of the plain tests, plus the fp32 weight's W_ULPS roundings on every term
        bound = (2 * (K + 16) * U53 + RR.W_ULPS * U24) * mag[:k]
        err = np.abs(joined[b, :k] - ref[:k])
        assert (err <= bound).all(), (b, (err / np.maximum(bound, 1e-300)).max())
        if mb == 0:
            assert not joined[b, :k].any() and np.array_equal(out[b], start.packed[b].cpu().numpy())
            continue
        p = c.astype(np.float64)
        if plane:
            cR, t, _, _, ok, _ = AP.plane_solve(joined[b], "similarity")
            assert ok == 1 and int(solved[b]) == 1
            tol = np.sqrt(3.0) * 4 * U24 * extent + 64 * AP.condition(joined[b], "similarity") * U53 * extent
        else:
            cR, t, _, _ = A.umeyama(joined[b], "similarity")
            tol = np.sqrt(3.0) * 8 * U24 * extent
        got, want = A.apply(out[b, :9].reshape(3, 3), out[b, 9:], p), A.apply(cR, t, p)
        ext = max(np.abs(want).max(), np.abs(p).max())                                   # the plain tests' "extent": the largest coordinate
        tol *= ext / extent
        disp = float(np.sqrt(((got - want) ** 2).sum(1).max()))
        print("robust %s %s surface=%s b=%d: displacement %.3g (bound %.3g)" % (form, step, surface, b, disp, tol))
        assert disp <= tol, (b, disp, tol)
    # scan.pose_update takes the same step
    pose = scan.Pose.identity(B, DEV)
    aligned = pose.apply(sb)
    scan.pose_update(pose, sb, aligned, m, "similarity", surface=surface, step=step, robust=form, robust_scale=sigma)
    assert np.array_equal(pose.packed.cpu().numpy().astype(np.float64), out)


# ------------------------------------------------------------------------------------------------ 5. the outlier experiment
def test_outlier_experiment_through_align():
    """tests/test_robust_host.py's inputs through scan.align: each robust form ends within 1.5 times the float64 loop's pose
    error plus the fp32 floor, and the plain run stays at least as biased as the float64 plain loop within the same margin - the
    feature, not the inputs, removes the bias.  Floor: the pose is stored in fp32 and the scan's coordinates are fp32 - 8 x
    2^-24 relative on scale and translation (per extent) and that angle in radians on the rotation, as tests/test_align.py
    bounds a solved pose."""
    v, _ = mesh("small_ae.npz")
    x = R.model_points(v, 1, seed=3)
    n = v.shape[0]
    xb = x[0, :n].astype(np.float64)
    cloud, truth, sigma, extent = RR.outlier_inputs(xb)
    ref = RR.outlier_reference()
    xd = torch.from_numpy(x).to(DEV)
    sb = scan.ScanBatch([cloud], DEV)
    floor = (np.degrees(8 * U24), 8 * U24 * extent, 8 * U24)
    got = {}
    for form in (None,) + RR.FORMS:
        kw = {} if form is None else dict(robust=form, robust_scale=sigma)
        pose, _, _ = scan.align(xd, sb, mode="similarity", iters=RR.OUTLIER_ITERS, w_model_to_scan=1.0, n=n, **kw)
        got[form] = RR.pose_error(pose.A[0].double().cpu().numpy(), pose.t[0].double().cpu().numpy(), truth)
        print("outlier experiment, GPU, %s: angle %.4g deg, translation %.4g, scale %.4g (float64: %.4g, %.4g, %.4g)" % ((form,) + got[form] + ref[form]))
    for form in RR.FORMS:
        for k in range(3):
            assert got[form][k] <= 1.5 * ref[form][k] + floor[k], (form, k, got[form][k], ref[form][k])
    for k in range(3):
        assert 1.5 * got[None][k] + floor[k] >= ref[None][k], (k, got[None][k], ref[None][k])
